// ccsd_t_ops.hip -- the assembly / energy kernel of the perturbative triples correction and its fixed-order sums (dev_ops.h: dev_ccsd_t_assemble,
// dev_ccsd_t_sum, dev_ccsd_t_total; driver in ccsd_t.cpp, the arithmetic in ccsd_t_core.h).
//
// One workgroup per (a,b,c) of a tile triple; a workgroup whose element is not a >= b >= c, or is a = b = c (identically zero), writes 0 and leaves.  The others
//   1. form W and V of every (i,j,k) -- six permuted reads of the product buffers, three t1 terms --, k fastest over the lanes: the reads of G_ACB and G_BCA
//      are contiguous over a wave, those of the other four buffers stride o or o^2 doubles (their o^3 cube of 64 KB at o = 20 is read once by the workgroup),
//   2. after a barrier read the five other ijk arrangements of V for r3(V), and add W r3(V) / D.
// V lives in LDS and W in registers (at most kCcsdTPerThread elements per thread) while o^3 doubles fit kCcsdTLdsBytes = 64 KiB -- two workgroups in a CU's
// 160 KiB: o <= 20; above that both go through 2 o^3 doubles of global memory per workgroup.
// The block has 64 .. 1024 threads, the smallest multiple of 64 with at most kCcsdTPerThread elements each (o = 5: one wave, o = 10: two, o >= 20: sixteen).
// No atomics: a shuffle tree per wave, the waves in ascending order, one partial per (a,b,c); dev_ccsd_t_sum adds the partials of a tile triple in one fixed
// order and dev_ccsd_t_total the tile triples in ascending order -- the same bits on every call and on any execution context.
#include "hip_common.h"
#include "ccsd_t_core.h"

namespace qemb {
namespace {

__device__ __forceinline__ double t_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

template <bool LDSV>
__global__ void __launch_bounds__(1024) ccsd_t_assemble_kernel(CcsdTArgs A) {
  extern __shared__ __attribute__((aligned(16))) double t_smem[];
  __shared__ double red[16];
  const int o = A.o, oo = o * o, o3 = oo * o;
  const int nth = blockDim.x, tid = threadIdx.x;
  const int lc = blockIdx.x % A.tc, lb = (blockIdx.x / A.tc) % A.tb, la = blockIdx.x / (A.tc * A.tb);
  const int a = A.a0 + la, b = A.b0 + lb, c = A.c0 + lc;
  if (!ccsd_t_evaluated(a, b, c)) {      // (the same for every thread of the workgroup)
    if (tid == 0) A.partial[blockIdx.x] = 0.0;
    return;
  }
  const double eabc = (A.ev[a] + A.ev[b]) + A.ev[c];
  double acc = 0.0;
  if constexpr (LDSV) {
    double* Vs = t_smem;
    double Wr[kCcsdTPerThread];
#pragma unroll
    for (int u = 0; u < kCcsdTPerThread; ++u) {
      const int e = tid + u * nth;
      Wr[u] = 0.0;
      if (e < o3) {
        const int i = e / oo, j = (e - i * oo) / o, k = e - i * oo - j * o;
        double Vv;
        ccsd_t_element(A, la, lb, lc, i, j, k, &Wr[u], &Vv);
        Vs[e] = Vv;
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kCcsdTPerThread; ++u) {
      const int e = tid + u * nth;
      if (e < o3) {
        const int i = e / oo, j = (e - i * oo) / o, k = e - i * oo - j * o;
        const double D = ((A.eo[i] + A.eo[j]) + A.eo[k]) - eabc;
        acc += Wr[u] * ccsd_t_r3(Vs, o, i, j, k) / D;
      }
    }
  } else {
    double* Wg = A.scratch + (long long)blockIdx.x * 2 * o3;
    double* Vg = Wg + o3;
    for (int e = tid; e < o3; e += nth) {
      const int i = e / oo, j = (e - i * oo) / o, k = e - i * oo - j * o;
      double Wv, Vv;
      ccsd_t_element(A, la, lb, lc, i, j, k, &Wv, &Vv);
      Wg[e] = Wv;
      Vg[e] = Vv;
    }
    __threadfence_block();
    __syncthreads();      // the workgroup's own stores, read back by other lanes of the same CU
    for (int e = tid; e < o3; e += nth) {
      const int i = e / oo, j = (e - i * oo) / o, k = e - i * oo - j * o;
      const double D = ((A.eo[i] + A.eo[j]) + A.eo[k]) - eabc;
      acc += Wg[e] * ccsd_t_r3(Vg, o, i, j, k) / D;
    }
  }
  acc = t_wave_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < (nth >> 6); ++w) s += red[w];
    A.partial[blockIdx.x] = s * (ccsd_t_weight(a, b, c) / 3.0);
  }
}

// out[slot] = the sum of m partials in one fixed order: 256 strided sums, a shuffle tree per wave, the four waves in order
__global__ void __launch_bounds__(256) ccsd_t_sum_kernel(long long m, const double* __restrict__ in, double* __restrict__ out, long long slot) {
  __shared__ double red[4];
  double acc = 0.0;
  for (long long k = threadIdx.x; k < m; k += 256) acc += in[k];
  acc = t_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[slot] = ((red[0] + red[1]) + red[2]) + red[3];
}

// out[0] = in[0] + in[1] + ... in ascending order (one lane: a few thousand tile triples at the most)
__global__ void __launch_bounds__(64) ccsd_t_total_kernel(long long m, const double* __restrict__ in, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (long long k = 0; k < m; ++k) s += in[k];
  out[0] = s;
}

template <bool LDSV>
int launch_assemble(const CcsdTArgs& A, int nth, size_t lds, hipStream_t st) {
  auto kern = ccsd_t_assemble_kernel<LDSV>;
  static bool attr_set = false;     // (benign if two threads both set it once)
  if (!attr_set) {
    HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCcsdTLdsBytes));
    attr_set = true;
  }
  return launch("dev_ccsd_t_assemble", kern, dim3((unsigned)(A.ta * A.tb * A.tc)), dim3(nth), lds, st, A);
}

}  // namespace

int dev_ccsd_t_assemble(const CcsdTArgs& A) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (const char* bad = ccsd_t_args_error(A)) { set_error(bad); return QEMB_ERR_ARG; }
  const long long o3 = (long long)A.o * A.o * A.o;
  long long nth = ((o3 + kCcsdTPerThread - 1) / kCcsdTPerThread + 63) / 64 * 64;
  if (nth > 1024) nth = 1024;
  if (ccsd_t_lds_form(A.o)) return launch_assemble<true>(A, (int)nth, (size_t)ccsd_t_lds_bytes(A.o), st);
  return launch_assemble<false>(A, 1024, 0, st);
}

int dev_ccsd_t_sum(int64_t m, const double* in, double* out, int64_t slot) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (m <= 0 || !in || !out || slot < 0) { set_error("dev_ccsd_t_sum: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_ccsd_t_sum", ccsd_t_sum_kernel, dim3(1), dim3(256), 0, st, m, in, out, slot);
}

int dev_ccsd_t_total(int64_t m, const double* in, double* out) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (m <= 0 || !in || !out) { set_error("dev_ccsd_t_total: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_ccsd_t_total", ccsd_t_total_kernel, dim3(1), dim3(64), 0, st, m, in, out);
}

}  // namespace qemb
