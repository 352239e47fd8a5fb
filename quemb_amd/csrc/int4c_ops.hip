// int4c_ops.hip -- the four-centre AO Coulomb integrals (mu nu|lambda sigma) on the device (dev_ops.h: dev_int4c_pairs, dev_int4c_class; driver in int4c.cpp;
// arithmetic in int4c_core.h, which reuses the Boys function, the Hermite coefficients and the R table of int3c_core.h).
//
// Two kernel families.  int4c_pair_kernel<la, lb> (6 instantiations): one thread per (shell pair, primitive pair) writes p, P and the Hermite expansion of
// the pair's real-spherical products to a work buffer.  int4c_class_kernel<la, lb, lc, ld> (the 21 canonical classes la >= lb, lc >= ld, bra pair class >=
// ket pair class): one thread per (shell quartet, ket component pair) -- a block is split over up to 25 threads, a thread carries at most 25 accumulators, the
// 35 folded Hermite integrals G and the R table of the class (10 to 165 numbers; the compiler's per-class register and scratch figures are in DESIGN.md
// section 4, "AO integrals on the device").  Every output element is stored once by plain stores.  l_a + l_b + l_c + l_d >= 4 runs in 64-thread workgroups.
// int4c_jk_kernel<la, lb, lc, ld> is the digest form of the class kernel (dev_int4c_jk_class): the same items and primitive loops, the unique integrals
// contracted with the density into the lower triangles of J and K by FP64 atomic adds instead of stored ("Integral-direct J and K").
// The class kernel also writes a tile of the 4-fold packed tensor (kTile, a runtime branch of the same 21 instantiations); int4c_pairprod_kernel and
// int4c_addt_kernel are the two element-wise passes of the transform that consumes the tiles ("Integral-direct AO -> fragment transform").
// Runtime (la, lb | lc, ld) become template arguments in int_dispatch.h (shared with the mock's restatement); every class goes through one launcher (launch_items).
#include "hip_common.h"
#include "int_dispatch.h"

namespace qemb {
namespace {

using namespace int4c;

template <int LA, int LB>
__global__ void __launch_bounds__(128) int4c_pair_kernel(const PairArgs g, const long long nitem) {
  const long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= nitem) return;
  pair_item<LA, LB>(g, item);
}

template <int LA, int LB, int LC, int LD>
__global__ void __launch_bounds__(LA + LB + LC + LD >= 4 ? 64 : 128) int4c_class_kernel(const ClassArgs g, const long long nitem) {
  const long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= nitem) return;
  quartet_item<LA, LB, LC, LD>(g, item);
}

template <int LA, int LB, int LC, int LD>
__global__ void __launch_bounds__(LA + LB + LC + LD >= 4 ? 64 : 128) int4c_jk_kernel(const JkArgs g, const long long nitem) {
  const long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= nitem) return;
  quartet_jk_item<LA, LB, LC, LD>(g, item);
}

__global__ void __launch_bounds__(128) int4c_dmax_kernel(const Shell* sh, const int nshell, const long long N, const double* dm, double* out) {
  const long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= (long long)nshell * nshell) return;
  dmax_item(sh, nshell, N, dm, out, item);
}

// one thread per element of P, x along pq: a wavefront stores 512 contiguous bytes; the two TA rows of a tile row are read from cache
__global__ void __launch_bounds__(256) int4c_pairprod_kernel(const PairProdArgs g) {
  const long long pq = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (pq >= g.npq) return;
  for (long long r = blockIdx.y; r < g.rows; r += gridDim.y) pairprod_item(g, r, pq);
}

__global__ void __launch_bounds__(256) int4c_addt_kernel(double* A, const long long m) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  for (long long i = blockIdx.y; i < m; i += gridDim.y) addt_item(A, m, i, j);
}

constexpr int quartet_block(int L) { return L >= 4 ? 64 : 128; }      // the launch bound of the class and digest kernels

}  // namespace

int dev_int4c_pairs(int la, int lb, const int4c::PairArgs& g) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (int rc = int4c_check_pairs(la, lb, g)) return rc;
  return dispatch_pair(pair_class(la, lb), [&](auto A, auto B) {
    return launch_items(int4c_pair_kernel<A(), B()>, 128, g, (long long)g.pairs.n * kPrimPairs, "dev_int4c_pairs", st);
  });
}

// the stored forms and the digest form: two callers of one dispatcher and one launcher, which differ in kernel and item count
int dev_int4c_class(int la, int lb, int lc, int ld, const int4c::ClassArgs& g) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (int rc = int4c_check_class(la, lb, lc, ld, g)) return rc;
  return dispatch_quartet(pair_class(la, lb), pair_class(lc, ld), "dev_int4c_class", [&](auto A, auto B, auto C, auto D) {
    return launch_items(int4c_class_kernel<A(), B(), C(), D()>, quartet_block(A() + B() + C() + D()), g, (long long)class_items<C(), D()>(g), "dev_int4c_class", st);
  });
}

int dev_int4c_jk_class(int la, int lb, int lc, int ld, const int4c::JkArgs& g) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (int rc = int4c_check_jk(la, lb, lc, ld, g)) return rc;
  return dispatch_quartet(pair_class(la, lb), pair_class(lc, ld), "dev_int4c_jk_class", [&](auto A, auto B, auto C, auto D) {
    return launch_items(int4c_jk_kernel<A(), B(), C(), D()>, quartet_block(A() + B() + C() + D()), g, (long long)jk_items<C(), D()>(g), "dev_int4c_jk_class", st);
  });
}

int dev_int4c_pairprod(const int4c::PairProdArgs& g) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (int rc = int4c_check_pairprod(g)) return rc;
  if (g.rows == 0) return QEMB_OK;
  const long long gy = g.rows < 65535 ? g.rows : 65535;
  return launch("dev_int4c_pairprod", int4c_pairprod_kernel, dim3((unsigned)((g.npq + 255) / 256), (unsigned)gy), dim3(256), 0, st, g);
}

int dev_int4c_add_transpose(int64_t m, double* A) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (m <= 0 || m > 0x7fffffffLL || !A) { set_error("dev_int4c_add_transpose: bad arguments"); return QEMB_ERR_ARG; }
  const long long gy = m < 65535 ? m : 65535;
  return launch("dev_int4c_add_transpose", int4c_addt_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)gy), dim3(256), 0, st, A, m);
}

int dev_int4c_dmax(const int3c::Shell* sh, int nshell, int64_t N, const double* dm, double* out) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (!sh || nshell <= 0 || N <= 0 || !dm || !out) { set_error("dev_int4c_dmax: bad arguments"); return QEMB_ERR_ARG; }
  const long long nitem = (long long)nshell * nshell;
  return launch("dev_int4c_dmax", int4c_dmax_kernel, dim3((unsigned)((nitem + 127) / 128)), dim3(128), 0, st, sh, nshell, N, dm, out);
}

}  // namespace qemb
