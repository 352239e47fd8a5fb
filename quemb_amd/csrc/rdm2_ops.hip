// rdm2_ops.hip -- the fragment 2-RDM in the fragment-MO basis (dev_ops.h: dev_rdm2_assemble; driver: Fragment::rdm2, fragment.cpp).
//
// Reference: make_rdm2_urlx (shared/external/ccsd_rdm.py:23-55, unrelaxed CCSD) and PySCF's mp2.make_rdm2 (unrelaxed MP2).  Both place an ovov block
// and its vovo image into an n^4 tensor that is zero elsewhere and, with_dm1, add products of the correlation 1-RDM with the HF determinant and the HF
// 2-RDM.  The reference forms goovv, dovov and the block as o^2 v^2 temporaries, zero-fills n^4 and then revisits it per statement (4 o + 2 strided
// n^2-sized updates).  Here every element of the n^4 tensor is WRITTEN ONCE, in rows of n^2 contiguous doubles: a workgroup owns rows (p,q); the ovov /
// vovo value is formed from the amplitudes on the fly (four reads of t2 for CCSD, two for MP2 -- 8 o^2 v^2 bytes against 8 n^4 written, so they come from
// L2 / MALL after the first touch) and the 1-RDM terms from the n x n matrix.  Bytes: 8 n^4 written, no read-modify-write, no zero-fill pass.
// Every element is a fixed expression of its inputs: the same bits run to run and in any sweep mode.
#include "hip_common.h"

namespace qemb {
namespace {

// the ovov block of the unrelaxed CCSD 2-RDM at [i,a,j,b]: dovov + dovov^T(2,3,0,1), dovov[i,a,j,b] = 2 g[i,j,a,b] - g[j,i,a,b], g = (t1 (x) t1 + t2) / 2
__device__ __forceinline__ double rdm2_ccsd_ovov(long long o, long long v, const double* __restrict__ t1, const double* __restrict__ t2,
                                                 long long i, long long a, long long j, long long b) {
  const double ia = t1[i * v + a], jb = t1[j * v + b], ib = t1[i * v + b], ja = t1[j * v + a];
  const long long ij = (i * o + j) * v, ji = (j * o + i) * v;
  const double g_ijab = 0.5 * (ia * jb + t2[(ij + a) * v + b]);
  const double g_jiab = 0.5 * (ja * ib + t2[(ji + a) * v + b]);
  const double g_jiba = 0.5 * (jb * ia + t2[(ji + b) * v + a]);
  const double g_ijba = 0.5 * (ib * ja + t2[(ij + b) * v + a]);
  return (2.0 * g_ijab - g_jiab) + (2.0 * g_jiba - g_ijba);
}
// the ovov block of mp2.make_rdm2 at [i,a,j,b]: 2 (2 t2[i,j,a,b] - t2[i,j,b,a])
__device__ __forceinline__ double rdm2_mp2_ovov(long long o, long long v, const double* __restrict__ t2, long long i, long long a, long long j, long long b) {
  const long long ij = (i * o + j) * v;
  return 2.0 * (2.0 * t2[(ij + a) * v + b] - t2[(ij + b) * v + a]);
}

// grid: min(n^2, 2^20) workgroups, each walking the rows pq = x, x + gridDim.x, ...; a thread walks the row in steps of 256 and keeps (r,s) by increments
template <int KIND>
__global__ void __launch_bounds__(256) rdm2_assemble_kernel(long long o, long long v, const double* __restrict__ t1, const double* __restrict__ t2,
                                                            const double* __restrict__ d, double* __restrict__ out) {
  const long long n = o + v, n2 = n * n;
  const long long dr = 256 / n, ds = 256 - dr * n;
  for (long long pq = blockIdx.x; pq < n2; pq += gridDim.x) {
    const long long p = pq / n, q = pq - p * n;
    const bool row_ov = p < o && q >= o, row_vo = p >= o && q < o;
    const bool pq_occ = p == q && p < o;                     // (row-uniform parts of the with_dm1 statements)
    const double dpq2 = d ? 2.0 * d[p * n + q] : 0.0;
    double* __restrict__ row = out + pq * n2;
    long long r = (long long)threadIdx.x / n, s = (long long)threadIdx.x - r * n;
    for (long long rs = threadIdx.x; rs < n2; rs += 256) {
      double x = 0.0;
      if (row_ov) { if (r < o && s >= o) x = KIND == QEMB_RDM2_CCSD ? rdm2_ccsd_ovov(o, v, t1, t2, p, q - o, r, s - o) : rdm2_mp2_ovov(o, v, t2, p, q - o, r, s - o); }
      else if (row_vo) { if (r >= o && s < o) x = KIND == QEMB_RDM2_CCSD ? rdm2_ccsd_ovov(o, v, t1, t2, q, p - o, s, r - o) : rdm2_mp2_ovov(o, v, t2, q, p - o, s, r - o); }
      if (d) {      // with_dm1 (ccsd_rdm.py:40-53), d = dm1 - 2 I_occ; the statements in the reference's order
        const bool rs_occ = r == s && r < o;
        if (pq_occ) x += 2.0 * d[r * n + s];
        if (rs_occ) x += dpq2;
        if (q == r && q < o) x -= d[p * n + s];
        if (p == s && p < o) x -= d[r * n + q];
        if (pq_occ && rs_occ) x += 4.0;
        if (p == s && q == r && p < o && q < o) x -= 2.0;
      }
      row[rs] = x;
      r += dr; s += ds;
      if (s >= n) { s -= n; ++r; }
    }
  }
}

// ---- full-basis passes (quemb_amd/rdm_full.py; reference molbe/mbe.py:543-620) ------------------------------------------------------------------------
// X[i,j,k,l] += alpha (g[i,j] g[k,l] - g[i,l] g[j,k] / 2): the non-connected part of a 2-RDM ("ij,kl->ijkl" - "ij,kl->iklj" / 2 of mbe.py:553-557).  One read and one
// write of X per element, rows of m^2 contiguous doubles; g (m x m) stays in cache.
__global__ void __launch_bounds__(256) rdm2_add_nc_kernel(long long m, const double* __restrict__ g, double alpha, double* __restrict__ X) {
  const long long m2 = m * m;
  const long long dr = 256 / m, ds = 256 - dr * m;
  for (long long pq = blockIdx.x; pq < m2; pq += gridDim.x) {
    const long long p = pq / m, q = pq - p * m;
    const double gpq = g[pq];
    double* __restrict__ row = X + pq * m2;
    long long r = (long long)threadIdx.x / m, s = (long long)threadIdx.x - r * m;
    for (long long rs = threadIdx.x; rs < m2; rs += 256) {
      row[rs] += alpha * (gpq * g[rs] - 0.5 * g[p * m + s] * g[q * m + r]);
      r += dr; s += ds;
      if (s >= m) { s -= m; ++r; }
    }
  }
}

// X = (X + X^T) / 2 over all four indices (X^T[p,q,r,s] = X[s,r,q,p], mbe.py:601) in place, plus the non-connected part of g when g != null (mbe.py:603-620).
// The element idx and its image rev(idx) form a pair that ONE thread owns (the one with idx <= rev): both are read, both are written, nothing races.
__global__ void __launch_bounds__(256) rdm2_symmetrize_kernel(long long m, const double* __restrict__ g, double* __restrict__ X) {
  const long long m2 = m * m;
  const long long dr = 256 / m, ds = 256 - dr * m;
  for (long long pq = blockIdx.x; pq < m2; pq += gridDim.x) {
    const long long p = pq / m, q = pq - p * m;
    const long long qp = q * m + p;
    long long r = (long long)threadIdx.x / m, s = (long long)threadIdx.x - r * m;
    for (long long rs = threadIdx.x; rs < m2; rs += 256) {
      const long long idx = pq * m2 + rs, rev = (s * m + r) * m2 + qp;
      if (idx <= rev) {
        const double h = 0.5 * (X[idx] + X[rev]);
        double a = h, b = h;
        if (g) {
          a += g[pq] * g[rs] - 0.5 * g[p * m + s] * g[q * m + r];
          b += g[s * m + r] * g[qp] - 0.5 * g[s * m + p] * g[r * m + q];
        }
        X[idx] = a;
        if (rev != idx) X[rev] = b;
      }
      r += dr; s += ds;
      if (s >= m) { s -= m; ++r; }
    }
  }
}

// sum_pqrs eri[pqrs] K[pqrs] with the AO integrals unpacked on the fly: sym 1 = [m]^4, 4 = [npair][npair], 8 = 1-D npair(npair) (PySCF's mf._eri forms).
// Stage 1: workgroup b walks the rows pq = b, b + grid, ... of K (coalesced), every thread adds its elements in a fixed order, a fixed tree adds the 256
// thread sums -> partials[b].  Stage 2 (one workgroup) adds the partials the same way.  The partition depends on m alone: the same bits on every run.
__device__ __forceinline__ long long rdm2_pair(long long a, long long b) { return a >= b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; }
__device__ __forceinline__ double rdm2_block_sum(double x, double* sh) {
  sh[threadIdx.x] = x;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  return sh[0];
}
__global__ void __launch_bounds__(256) rdm2_eri_dot_kernel(long long m, int sym, const double* __restrict__ eri, const double* __restrict__ K, double* __restrict__ partials) {
  __shared__ double sh[256];
  const long long m2 = m * m, np = m * (m + 1) / 2;
  const long long dr = 256 / m, ds = 256 - dr * m;
  double acc = 0.0;
  for (long long pq = blockIdx.x; pq < m2; pq += gridDim.x) {
    const long long p = pq / m, q = pq - p * m;
    const long long PQ = rdm2_pair(p, q);
    const double* __restrict__ row = K + pq * m2;
    long long r = (long long)threadIdx.x / m, s = (long long)threadIdx.x - r * m;
    for (long long rs = threadIdx.x; rs < m2; rs += 256) {
      long long e;
      if (sym == 1) e = pq * m2 + rs;
      else { const long long RS = rdm2_pair(r, s); e = sym == 4 ? PQ * np + RS : rdm2_pair(PQ, RS); }
      acc += eri[e] * row[rs];
      r += dr; s += ds;
      if (s >= m) { s -= m; ++r; }
    }
  }
  const double t = rdm2_block_sum(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
__global__ void __launch_bounds__(256) rdm2_sum_partials_kernel(long long count, const double* __restrict__ partials, double* __restrict__ out) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (long long k = threadIdx.x; k < count; k += 256) acc += partials[k];
  const double t = rdm2_block_sum(acc, sh);
  if (threadIdx.x == 0) out[0] = t;
}

}  // namespace

int dev_rdm2_assemble(int kind, int64_t o, int64_t v, const double* t1, const double* t2, const double* dm1c, double* out) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (int rc = rdm2_check_args(kind, o, v, t1, t2, out)) return rc;
  const long long n = o + v, n2 = n * n;
  const unsigned grid = (unsigned)(n2 < (1LL << 20) ? n2 : (1LL << 20));
  if (kind == QEMB_RDM2_CCSD) return launch("dev_rdm2_assemble", rdm2_assemble_kernel<QEMB_RDM2_CCSD>, dim3(grid), dim3(256), 0, st, o, v, t1, t2, dm1c, out);
  return launch("dev_rdm2_assemble", rdm2_assemble_kernel<QEMB_RDM2_MP2>, dim3(grid), dim3(256), 0, st, o, v, t1, t2, dm1c, out);
}

int dev_rdm2_add_nc(int64_t m, const double* g, double alpha, double* X) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (int rc = rdm2_check_full(m, g, X)) return rc;
  return launch("dev_rdm2_add_nc", rdm2_add_nc_kernel, dim3((unsigned)rdm2_full_grid(m)), dim3(256), 0, st, m, g, alpha, X);
}

int dev_rdm2_symmetrize(int64_t m, const double* g, double* X) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (int rc = rdm2_check_full(m, X, X)) return rc;
  return launch("dev_rdm2_symmetrize", rdm2_symmetrize_kernel, dim3((unsigned)rdm2_full_grid(m)), dim3(256), 0, st, m, g, X);
}

int dev_rdm2_eri_dot(int64_t m, int sym, const double* eri, const double* K, double* partials, double* out_dev) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (int rc = rdm2_check_full(m, eri, K)) return rc;
  if ((sym != 1 && sym != 4 && sym != 8) || !partials || !out_dev) { set_error("dev_rdm2_eri_dot: sym must be 1, 4 or 8 and the outputs non-null"); return QEMB_ERR_ARG; }
  const int64_t grid = rdm2_full_grid(m);
  QTRY(launch("dev_rdm2_eri_dot", rdm2_eri_dot_kernel, dim3((unsigned)grid), dim3(256), 0, st, m, sym, eri, K, partials));
  return launch("dev_rdm2_eri_dot", rdm2_sum_partials_kernel, dim3(1), dim3(256), 0, st, grid, partials, out_dev);
}

}  // namespace qemb
