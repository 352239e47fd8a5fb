// mp2_ops.hip -- the one HBM pass of the MP2 path (dev_ops.h: dev_mp2_amplitudes; driver in mp2.cpp).
//
// Between the product ovov = Lov^T Lov and the finished amplitudes the CCSD set-up spends six passes over o^2 v^2 data (perm4, dcopy, axpby, perm4,
// div_denom, dot).  Here each 32 x 32 tile of the (a,b) matrix of an occupied pair (i,j) and its (a <-> b) partner tile are read ONCE by one workgroup,
// which writes both tiles of t2[i,j,:,:] and both tiles of G[i,:,j,:] in rows of 256 bytes and keeps its share of the energy in a register:
// 8 o^2 v^2 bytes read, 2 x 8 o^2 v^2 written.  The partner values pass through LDS (padded rows: no bank conflicts on the transposed read).
#include "hip_common.h"

namespace qemb {
namespace {

__device__ __forceinline__ double mp2_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

// grid (npair(nt) tile pairs ta >= tb, min(o^2, 4096) occupied pairs): a workgroup walks the occupied pairs ij = y, y + gridDim.y, ...
__global__ void __launch_bounds__(256) mp2_amplitudes_kernel(long long o, long long v, const double* __restrict__ ovov, const double* __restrict__ eo,
                                                             const double* __restrict__ ev, double* __restrict__ t2, double* __restrict__ G,
                                                             double* __restrict__ partials) {
  __shared__ double tS[32][33], tP[32][33];
  __shared__ double red[4];
  const uint3 GD = make_uint3(gridDim.x, gridDim.y, gridDim.z);
  const uint3 LB = xcd_logical_block(make_uint3(blockIdx.x, blockIdx.y, blockIdx.z), GD);
  long long ta = (long long)((sqrt(8.0 * (double)LB.x + 1.0) - 1.0) * 0.5);
  while (ta * (ta + 1) / 2 > (long long)LB.x) --ta;
  while ((ta + 1) * (ta + 2) / 2 <= (long long)LB.x) ++ta;
  const long long tb = (long long)LB.x - ta * (ta + 1) / 2;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const long long ov = o * v, vv = v * v, oo = o * o;
  double acc = 0.0;
  for (long long ij = LB.y; ij < oo; ij += GD.y) {
    const long long i = ij / o, j = ij - i * o;
    const double eij = eo[i] + eo[j];
    const double* Mij = ovov + i * v * ov + j * v;      // (x,y) of the pair's matrix at Mij[x * ov + y]
    double* Gij = G + i * v * ov + j * v;
    double* Tij = t2 + ij * vv;
    double s[4], p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {      // the tile (ta,tb) in rows of a, and the tile (tb,ta) in rows of b
      const int r = ty + 8 * k;
      const long long a = ta * 32 + r, b = tb * 32 + tx;
      s[k] = (a < v && b < v) ? Mij[a * ov + b] : 0.0;
      const long long b2 = tb * 32 + r, a2 = ta * 32 + tx;
      p[k] = (a2 < v && b2 < v) ? Mij[b2 * ov + a2] : 0.0;
      tS[r][tx] = s[k];
      tP[r][tx] = p[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {      // t2[i,j,a,b], G[i,a,j,b] on the tile (ta,tb)
      const int aa = ty + 8 * k;
      const long long a = ta * 32 + aa, b = tb * 32 + tx;
      if (a < v && b < v) {
        const double pt = tP[tx][aa];                            // ovov[i,b,j,a]
        const double d = (eij - ev[a]) - ev[b];
        const double t = s[k] / d;
        const double tp = pt / d;                                // t2[j,i,a,b] = (ja|ib) / d, read as its twin (ib|ja)
        Tij[a * v + b] = t;
        Gij[a * ov + b] = fma(2.0, t, -tp);
        acc += t * (2.0 * s[k] - pt);
      }
    }
    if (ta != tb) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {    // ... and on the partner tile (tb,ta), rows of b
        const int bb = ty + 8 * k;
        const long long b = tb * 32 + bb, a = ta * 32 + tx;
        if (a < v && b < v) {
          const double st = tS[tx][bb];                          // ovov[i,a,j,b]
          const double d = (eij - ev[b]) - ev[a];
          const double t = p[k] / d;
          const double tp = st / d;
          Tij[b * v + a] = t;
          Gij[b * ov + a] = fma(2.0, t, -tp);
          acc += t * (2.0 * p[k] - st);
        }
      }
    }
    __syncthreads();      // the next pair overwrites the tiles
  }
  acc = mp2_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[(long long)LB.y * GD.x + LB.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// the partial sums of the workgroups in a fixed order: the same bits run to run and in every sweep mode
__global__ void __launch_bounds__(256) mp2_energy_sum_kernel(long long np, const double* __restrict__ partials, double* __restrict__ out) {
  __shared__ double red[4];
  double acc = 0.0;
  for (long long k = threadIdx.x; k < np; k += 256) acc += partials[k];
  acc = mp2_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace

int dev_mp2_amplitudes(int64_t o, int64_t v, const double* ovov, const double* eo, const double* ev, double* t2, double* G, double* partials, double* e_dev) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (o <= 0 || v <= 0 || !ovov || !eo || !ev || !t2 || !G || !partials || !e_dev) { set_error("dev_mp2_amplitudes: bad arguments"); return QEMB_ERR_ARG; }
  if (t2 == ovov || G == ovov) { set_error("dev_mp2_amplitudes: the outputs may not alias ovov"); return QEMB_ERR_ARG; }
  const long long nt = (v + 31) / 32, ntp = nt * (nt + 1) / 2, oo = o * o;
  const long long gy = oo < 4096 ? oo : 4096;
  if (ntp > 0x7fffffffLL) { set_error("dev_mp2_amplitudes: too many virtual tiles"); return QEMB_ERR_ARG; }
  QTRY(launch("dev_mp2_amplitudes", mp2_amplitudes_kernel, dim3((unsigned)ntp, (unsigned)gy), dim3(256), 0, st, o, v, ovov, eo, ev, t2, G, partials));
  return launch("dev_mp2_amplitudes", mp2_energy_sum_kernel, dim3(1), dim3(256), 0, st, ntp * gy, partials, e_dev);
}

}  // namespace qemb
