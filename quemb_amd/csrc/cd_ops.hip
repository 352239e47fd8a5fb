// cd_ops.hip -- the kernels of the pivoted Cholesky decomposition of the AO integrals that have no counterpart elsewhere (driver: int4c.cpp, int4c_cholesky;
// arithmetic: cd_core.h, shared with the scalar restatement cd_ops_hostcheck.cpp):
//   gather_cols   out[k][c] = in[k][idx[c]]: the diagonal out of the kDiag buffers, the factor's columns at a panel's rows, the canonical packed order at the end
//   panel_factor  pivoted, rank-revealing Cholesky of a panel's own n x n block -- ONE workgroup, factor and residual diagonal in LDS up to n = 86
//   new_rows      the r new vectors at every AO pair: forward substitution against the panel's triangular factor, one thread per pair
//   diag_update   d -= sum_k Lnew[k]^2 (pivots exactly 0, negative residue clamped), the per-shell-pair maxima and their maximum in two stages
//   unpack        the factor from plan-row order straight to the [M][N][N] image of a DF context, every element once
// No atomics anywhere: each output element has one writer and every sum one fixed order, so a decomposition gives the same bits on every run and context.
#include "hip_common.h"
#include "cd_core.h"

namespace qemb {
using namespace cd;

namespace {

__global__ void __launch_bounds__(256) cd_gather_kernel(const long long rows, const long long ncols, const double* __restrict__ in, const long long ldi,
                                                        const int32_t* __restrict__ idx, double* __restrict__ out, const long long ldo) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncols) return;
  for (long long k = blockIdx.y; k < rows; k += gridDim.y) gather_item(k, c, in, ldi, idx, out, ldo);
}

// x along nu: a wavefront stores 512 contiguous bytes of one (k, mu) row
__global__ void __launch_bounds__(256) cd_unpack_kernel(const long long M, const long long N, const double* __restrict__ L, const long long ld, const int32_t* __restrict__ pos,
                                                        double* __restrict__ out) {
  const long long nu = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (nu >= N) return;
  for (long long km = blockIdx.y; km < M * N; km += gridDim.y) unpack_item(km / N, km % N, nu, N, L, ld, pos, out);
}

// One workgroup.  Per step: the pivot search (a strided scan and a tree over 256 candidates, ordered by pivot_better), then every thread's columns of the new
// vector (panel_col: reads the earlier vectors at the pivot column and its own).  T and dd live in LDS (use_lds) or in the global output and work buffer; either
// way a step's stores are separated from the next step's loads by the workgroup barrier.
__global__ void __launch_bounds__(kPanelThreads) cd_panel_kernel(const double* __restrict__ E, const long long ld, const int32_t* __restrict__ srow, const int n, const double thr,
                                                                 const double* __restrict__ d, double* T, int32_t* __restrict__ piv, int32_t* __restrict__ rank, double* work,
                                                                 const int use_lds) {
  extern __shared__ double cd_dyn[];
  __shared__ double rv[kPanelThreads];
  __shared__ int ri[kPanelThreads];
  double* Tw = use_lds ? cd_dyn : T;
  double* dd = use_lds ? cd_dyn + (size_t)n * n : work;
  const int tid = threadIdx.x;
  for (int c = tid; c < n; c += kPanelThreads) dd[c] = panel_diag0(E, ld, srow, d, c);
  __syncthreads();
  int j = 0;
  for (; j < n; ++j) {
    double bv = -1.0;
    int bi = n;
    for (int c = tid; c < n; c += kPanelThreads)
      if (pivot_better(dd[c], c, bv, bi)) { bv = dd[c]; bi = c; }
    rv[tid] = bv; ri[tid] = bi;
    __syncthreads();
    for (int w = kPanelThreads / 2; w > 0; w >>= 1) {
      if (tid < w && pivot_better(rv[tid + w], ri[tid + w], rv[tid], ri[tid])) { rv[tid] = rv[tid + w]; ri[tid] = ri[tid + w]; }
      __syncthreads();
    }
    const double best = rv[0];
    const int p = ri[0];
    __syncthreads();      // rv / ri are rewritten by the next step
    if (!(best > thr)) break;      // the same value in every thread: the whole workgroup leaves together
    const double s = sqrt(best);
    if (tid == 0) piv[j] = p;
    for (int c = tid; c < n; c += kPanelThreads) panel_col(E, ld, srow, n, j, p, s, c, Tw, dd);
    __syncthreads();
  }
  if (tid == 0) rank[0] = j;
  if (use_lds)
    for (long long e = tid; e < (long long)j * n; e += kPanelThreads) T[e] = Tw[e];
}

__global__ void __launch_bounds__(128) cd_newrows_kernel(const long long np, const int n, const int r, const double* __restrict__ E, const long long ld, const double* __restrict__ T,
                                                         const int32_t* __restrict__ piv, double* Lnew, const long long ldl) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= np) return;
  newrows_item(row, n, r, E, ld, T, piv, Lnew, ldl);
}

__global__ void __launch_bounds__(256) cd_diag_kernel(const long long np, const int r, const double* __restrict__ Lnew, const long long ldl, const int32_t* __restrict__ piv,
                                                      const int32_t* __restrict__ srow, double* __restrict__ d) {
  const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= np) return;
  diag_item(row, r, Lnew, ldl, piv, srow, d);
}

__device__ __forceinline__ double cd_block_max(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] = sh[threadIdx.x + w] > sh[threadIdx.x] ? sh[threadIdx.x + w] : sh[threadIdx.x];
    __syncthreads();
  }
  return sh[0];
}
// stage one: the maximum of every shell pair and one partial per workgroup; stage two (one workgroup): the maximum of the partials
__global__ void __launch_bounds__(256) cd_pairmax_kernel(const long long nsp, const int32_t* __restrict__ row0, const int32_t* __restrict__ cnt, const double* __restrict__ d,
                                                         double* __restrict__ spmax, double* __restrict__ partials) {
  __shared__ double sh[256];
  const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  double m = 0.0;
  if (w < nsp) { m = pairmax_item(w, row0, cnt, d); spmax[w] = m; }
  const double t = cd_block_max(m, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
__global__ void __launch_bounds__(256) cd_max_partials_kernel(const long long count, const double* __restrict__ partials, double* __restrict__ out) {
  __shared__ double sh[256];
  double m = 0.0;
  for (long long k = threadIdx.x; k < count; k += 256) m = partials[k] > m ? partials[k] : m;
  const double t = cd_block_max(m, sh);
  if (threadIdx.x == 0) out[0] = t;
}

#define CD_STREAM(st)                                                                                  \
  hipStream_t st = hip_stream();                                                                       \
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }

}  // namespace

int dev_cd_gather_cols(int64_t rows, int64_t ncols, const double* in, int64_t ldi, const int32_t* idx, double* out, int64_t ldo) {
  CD_STREAM(st);
  if (int rc = check_gather(rows, ncols, in, ldi, idx, out, ldo)) return rc;
  if (rows == 0 || ncols == 0) return QEMB_OK;
  const long long gy = rows < 65535 ? rows : 65535;
  return launch("dev_cd_gather_cols", cd_gather_kernel, dim3((unsigned)((ncols + 255) / 256), (unsigned)gy), dim3(256), 0, st, rows, ncols, in, ldi, idx, out, ldo);
}

int dev_cd_unpack(int64_t M, int64_t N, const double* L, int64_t ld, const int32_t* pos, double* out) {
  CD_STREAM(st);
  if (int rc = check_unpack(M, N, L, ld, pos, out)) return rc;
  if (M == 0) return QEMB_OK;
  const long long gy = M * N < 65535 ? M * N : 65535;
  return launch("dev_cd_unpack", cd_unpack_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)gy), dim3(256), 0, st, M, N, L, ld, pos, out);
}

int dev_cd_panel_factor(const double* E, int64_t ld, const int32_t* srow, int n, double thr, const double* d, double* T, int32_t* piv, int32_t* rank, double* work) {
  CD_STREAM(st);
  if (int rc = check_panel(E, ld, srow, n, thr, T, piv, rank, work)) return rc;
  const int use_lds = panel_in_lds(n) ? 1 : 0;
  const size_t lds = use_lds ? sizeof(double) * ((size_t)n * n + n) : 0;
  return launch("dev_cd_panel_factor", cd_panel_kernel, dim3(1), dim3(kPanelThreads), lds, st, E, ld, srow, n, thr, d, T, piv, rank, work, use_lds);
}

int dev_cd_new_rows(int64_t np, int n, int r, const double* E, int64_t ld, const double* T, const int32_t* piv, double* Lnew, int64_t ldl) {
  CD_STREAM(st);
  if (int rc = check_new_rows(np, n, r, E, ld, T, piv, Lnew, ldl)) return rc;
  if (r == 0) return QEMB_OK;
  return launch("dev_cd_new_rows", cd_newrows_kernel, dim3((unsigned)((np + 127) / 128)), dim3(128), 0, st, np, n, r, E, ld, T, piv, Lnew, ldl);
}

int dev_cd_diag_update(int64_t np, int r, const double* Lnew, int64_t ldl, const int32_t* piv, const int32_t* srow, double* d, int64_t nsp, const int32_t* row0, const int32_t* cnt,
                       double* spmax, double* partials, double* dmax) {
  CD_STREAM(st);
  if (int rc = check_diag_update(np, r, Lnew, ldl, piv, srow, d, nsp, row0, cnt, spmax, partials, dmax)) return rc;
  if (r > 0) QTRY(launch("dev_cd_diag_update", cd_diag_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, np, r, Lnew, ldl, piv, srow, d));
  const int64_t nb = pair_max_partials(nsp);
  QTRY(launch("dev_cd_diag_update", cd_pairmax_kernel, dim3((unsigned)nb), dim3(256), 0, st, nsp, row0, cnt, d, spmax, partials));
  return launch("dev_cd_diag_update", cd_max_partials_kernel, dim3(1), dim3(256), 0, st, nb, partials, dmax);
}

}  // namespace qemb
