// int3c_ops.hip -- the 3-centre (mu nu|P) and 2-centre (P|Q) Coulomb integrals of density fitting on the device (dev_ops.h: dev_boys, dev_int3c_class;
// driver in int3c.cpp; arithmetic in int3c_core.h).
//
// One kernel instantiation per angular class (l_a >= l_b, l_P); one thread per (shell pair, auxiliary shell) block of the class, so a wavefront runs one
// class and its lanes differ in geometry and exponents only.  A thread loops over the primitive triples, keeps the Cartesian block in private memory,
// applies the Cartesian -> spherical matrices and stores each element of its block once.  The shells are read in place (const Shell&).  Per the compiler's
// resource report the classes (0,0|0..2), (1,0|0..1), (1,1|0) and (2,0|0) use no scratch memory; all others keep part of their private arrays there (256 bytes to
// 7.6 kB per lane, 256 VGPRs, one wave per SIMD for the high classes); l_a + l_b + l_P >= 4 runs in 64-thread workgroups ("DF integrals on the device").
// Runtime (la, lb | lP) become template arguments in int_dispatch.h (shared with the mock's restatement); the launcher is launch_items of hip_common.h.
#include "hip_common.h"
#include "int_dispatch.h"

namespace qemb {
namespace {

using namespace int3c;

template <int LA, int LB, int LP>
__global__ void __launch_bounds__(LA + LB + LP >= 4 ? 64 : 128) int3c_class_kernel(const ClassArgs g, const long long nitem) {
  const long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= nitem) return;
  class_item<LA, LB, LP>(g, item);
}

__global__ void __launch_bounds__(128) boys_kernel(int m_max, long long n, const double* __restrict__ x, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double F[2 * kMaxL + 2 * 2 + 1];
  boys(m_max, x[i], F);
  for (int m = 0; m <= m_max; ++m) out[i * (m_max + 1) + m] = F[m];
}

}  // namespace

int dev_boys(int m_max, int64_t n, const double* x, double* out) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (int rc = int3c_check_boys(m_max, n, x, out)) return rc;
  if (n == 0) return QEMB_OK;
  return launch("dev_boys", boys_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, m_max, n, x, out);
}

int dev_int3c_class(int la, int lb, int lp, const int3c::ClassArgs& g) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (int rc = int3c_check_class(la, lb, lp, g)) return rc;
  return dispatch_int3c(la, lb, lp, [&](auto A, auto B, auto P) {
    return launch_items(int3c_class_kernel<A(), B(), P()>, A() + B() + P() >= 4 ? 64 : 128, g, (long long)g.npair * g.naux_sh, "dev_int3c_class", st);
  });
}

}  // namespace qemb
