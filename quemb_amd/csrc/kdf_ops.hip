// kdf_ops.hip -- the three HBM passes of the k-point density-fitted transform (dev_ops.h: dev_kdf_split / dev_kdf_stack / dev_kdf_pack; driver in kdf.cpp).
//
// Both quarter transforms of KdfContext::transform are FP64 MFMA products (dev_gemm) over operands whose real and imaginary parts are stacked along K,
// so a complex product is one real product.  What is left around them is data movement:
//   split  an uploaded interleaved complex128 pair block becomes the planar image [row][re (ld) | im (ld)]: a wave reads 1 KiB of (re, im) pairs (16 bytes per lane)
//          and writes two runs of 512 bytes; ld is a multiple of 16 doubles, so every written run starts on a 128-byte line.  One read, one write.
//   stack  the coefficient operands of all k-points from TA_k (small: nk (2 ld + 2 nao) 2 n doubles).
//   pack   M^q[P] = [Re | Im][p][q] becomes rows of the fragment's real factor: each 32 x 32 tile (ta >= tb) of a plane and its transposed partner are read once by one
//          workgroup, the lower triangle is written scaled in runs of up to 256 bytes, and the partner (through LDS, padded rows) only feeds the symmetry check.
//          The two maxima leave the workgroup as one partial pair; a second launch reduces the partials in a fixed order.
// No atomics; every output element is written exactly once.
#include "hip_common.h"

namespace qemb {
namespace {

__device__ __forceinline__ double kdf_wave_max(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_down(x, off, 64));
  return x;
}

// grid: ceil(rows / 4) workgroups of 4 waves, one row per wave
__global__ void __launch_bounds__(256) kdf_split_kernel(long long rows, long long nao, long long ld, const double2* __restrict__ z, double* __restrict__ planes) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const double2* zr = z + r * nao;
  double* re = planes + r * 2 * ld;
  double* im = re + ld;
  for (long long nu = threadIdx.x & 63; nu < ld; nu += 64) {
    const double2 v = nu < nao ? zr[nu] : make_double2(0.0, 0.0);
    re[nu] = v.x;
    im[nu] = v.y;
  }
}

__global__ void __launch_bounds__(256) kdf_stack_kernel(long long nk, long long nao, long long n, long long ld, const double* __restrict__ ta, double* __restrict__ Cs,
                                                        double* __restrict__ Dk) {
  const long long csz = 4 * ld * n, dsz = 4 * nao * n, per = csz + dsz, total = nk * per;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long k = idx / per, e = idx - k * per;
    if (e < csz) {
      const long long row = e / (2 * n), col = e - row * 2 * n;
      const int half = row >= ld, cpart = col >= n;
      const long long nu = row - half * ld, j = col - cpart * n;
      double val = 0.0;
      if (nu < nao) {
        const double* c = ta + ((k * nao + nu) * n + j) * 2;
        val = (half == cpart) ? c[0] : (half ? -c[1] : c[1]);
      }
      Cs[k * csz + e] = val;
    } else {
      const long long d = e - csz, row = d / (2 * n), col = d - row * 2 * n;
      const long long mu = row >> 1, j = col >= n ? col - n : col;
      const int c1 = (int)(row & 1), c2 = col >= n;
      const double* c = ta + ((k * nao + mu) * n + j) * 2;
      Dk[k * dsz + d] = (c1 == c2) ? c[0] : (c2 ? -c[1] : c[1]);
    }
  }
}

// grid (npair(nt) tile pairs ta >= tb, min(naux, 1024)): a workgroup walks the auxiliary rows P = y, y + gridDim.y, ...
__global__ void __launch_bounds__(256) kdf_pack_kernel(long long naux, long long n, const double* __restrict__ M, int paired, double w, double* __restrict__ F,
                                                       long long ldf, double* __restrict__ partials) {
  __shared__ double tP[32][33];
  __shared__ double red[2][4];
  const uint3 GD = make_uint3(gridDim.x, gridDim.y, gridDim.z);
  const uint3 LB = xcd_logical_block(make_uint3(blockIdx.x, blockIdx.y, blockIdx.z), GD);
  long long ta = (long long)((sqrt(8.0 * (double)LB.x + 1.0) - 1.0) * 0.5);
  while (ta * (ta + 1) / 2 > (long long)LB.x) --ta;
  while ((ta + 1) * (ta + 2) / 2 <= (long long)LB.x) ++ta;
  const long long tb = (long long)LB.x - ta * (ta + 1) / 2;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const long long nn = n * n;
  double asym = 0.0, amax = 0.0;
  for (long long P = LB.y; P < naux; P += GD.y) {
    for (int c = 0; c < 2; ++c) {
      const double* Mp = M + (P * 2 + c) * nn;
      double s[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {      // the tile (ta,tb) in rows of p, and the tile (tb,ta) in rows of q
        const int r = ty + 8 * k;
        const long long a = ta * 32 + r, b = tb * 32 + tx;
        s[k] = (a < n && b < n) ? Mp[a * n + b] : 0.0;
        const long long b2 = tb * 32 + r, a2 = ta * 32 + tx;
        const double pv = (a2 < n && b2 < n) ? Mp[b2 * n + a2] : 0.0;
        tP[r][tx] = pv;
        amax = fmax(amax, fmax(fabs(s[k]), fabs(pv)));
      }
      __syncthreads();
      const bool keep = c == 0 || paired;
      double* Fr = F + ((long long)c * naux + P) * ldf;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int aa = ty + 8 * k;
        const long long a = ta * 32 + aa, b = tb * 32 + tx;
        if (a < n && b < n && a >= b) {
          asym = fmax(asym, fabs(s[k] - tP[tx][aa]));      // M[P,p,q] - M[P,q,p]
          if (keep) Fr[a * (a + 1) / 2 + b] = w * s[k];
          else asym = fmax(asym, fabs(s[k]));               // a self-conjugate class: Im M^q is dropped, so it has to vanish
        }
      }
      __syncthreads();      // the next plane overwrites the tile
    }
  }
  asym = kdf_wave_max(asym);
  amax = kdf_wave_max(amax);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = asym; red[1][threadIdx.x >> 6] = amax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = partials + 2 * ((long long)LB.y * GD.x + LB.x);
    o[0] = fmax(fmax(red[0][0], red[0][1]), fmax(red[0][2], red[0][3]));
    o[1] = fmax(fmax(red[1][0], red[1][1]), fmax(red[1][2], red[1][3]));
  }
}

// the partial pairs of the workgroups in a fixed order
__global__ void __launch_bounds__(256) kdf_pack_max_kernel(long long np, const double* __restrict__ partials, double* __restrict__ out2) {
  __shared__ double red[2][4];
  double asym = 0.0, amax = 0.0;
  for (long long k = threadIdx.x; k < np; k += 256) { asym = fmax(asym, partials[2 * k]); amax = fmax(amax, partials[2 * k + 1]); }
  asym = kdf_wave_max(asym);
  amax = kdf_wave_max(amax);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = asym; red[1][threadIdx.x >> 6] = amax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out2[0] = fmax(fmax(red[0][0], red[0][1]), fmax(red[0][2], red[0][3]));
    out2[1] = fmax(fmax(red[1][0], red[1][1]), fmax(red[1][2], red[1][3]));
  }
}

}  // namespace

int dev_kdf_split(int64_t rows, int64_t nao, const double* z, double* planes) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (rows <= 0 || nao <= 0 || !z || !planes) { set_error("dev_kdf_split: bad arguments"); return QEMB_ERR_ARG; }
  const long long nb = (rows + 3) / 4;
  if (nb > 0x7fffffffLL || ((uintptr_t)z & 15)) { set_error("dev_kdf_split: too many rows or a source that is not 16-byte aligned"); return QEMB_ERR_ARG; }
  return launch("dev_kdf_split", kdf_split_kernel, dim3((unsigned)nb), dim3(256), 0, st, rows, nao, kdf_ld(nao), reinterpret_cast<const double2*>(z), planes);
}

int dev_kdf_stack(int64_t nk, int64_t nao, int64_t n, const double* ta, double* Cs, double* Dk) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (nk <= 0 || nao <= 0 || n <= 0 || !ta || !Cs || !Dk) { set_error("dev_kdf_stack: bad arguments"); return QEMB_ERR_ARG; }
  const long long ld = kdf_ld(nao), total = nk * (4 * ld * n + 4 * nao * n);
  long long nb = (total + 255) / 256;
  if (nb > 4096) nb = 4096;
  return launch("dev_kdf_stack", kdf_stack_kernel, dim3((unsigned)nb), dim3(256), 0, st, nk, nao, n, ld, ta, Cs, Dk);
}

int dev_kdf_pack(int64_t naux, int64_t n, const double* M, int paired, double w, double* F, int64_t ldf, double* partials, double* out2_dev) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (int rc = kdf_check_pack(naux, n, M, F, ldf, partials, out2_dev)) return rc;
  const long long nt = (n + 31) / 32, ntp = nt * (nt + 1) / 2, gy = naux < 1024 ? naux : 1024;
  QTRY(launch("dev_kdf_pack", kdf_pack_kernel, dim3((unsigned)ntp, (unsigned)gy), dim3(256), 0, st, naux, n, M, paired, w, F, ldf, partials));
  return launch("dev_kdf_pack", kdf_pack_max_kernel, dim3(1), dim3(256), 0, st, ntp * gy, partials, out2_dev);
}

}  // namespace qemb
