// cd_core.h -- the arithmetic of the element-wise and panel passes of the pivoted Cholesky decomposition of the AO integrals (int4c.cpp: int4c_cholesky),
// written once for the kernels of cd_ops.hip (one item per thread) and their scalar restatement for the mock device layer (cd_ops_hostcheck.cpp: the items in a
// loop).  Rows are AO pairs in the order of the pair plan ("plan rows"); a panel is a set S of n of them (srow[c]: the plan row of panel column c) and
// E[row * ld + c] the residual integrals (row | srow[c]).  All index arrays are int32 on the device.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include "dev_ops.h"

#if defined(__HIPCC__)
#define QEMB_CD_HD __host__ __device__ __forceinline__
#else
#define QEMB_CD_HD inline
#endif

namespace qemb {
namespace cd {

// The in-panel factorisation keeps its factor (n x n) and the panel's residual diagonal (n) in LDS up to this n: 86 * 86 + 86 doubles = 59856 bytes, with the
// 3 KiB of the pivot search under the 64 KiB per workgroup that leave a CU (160 KiB) room for a second one.  Larger panels work in the global output.
constexpr int kPanelLdsMax = 86;
constexpr int kPanelThreads = 256;
inline bool panel_in_lds(int n) { return n <= kPanelLdsMax; }
inline int64_t pair_max_partials(int64_t nsp) { return (nsp + 255) / 256; }

// out[k * ldo + c] = in[k * ldi + idx[c]]
QEMB_CD_HD void gather_item(int64_t k, int64_t c, const double* in, int64_t ldi, const int32_t* idx, double* out, int64_t ldo) { out[k * ldo + c] = in[k * ldi + idx[c]]; }

// out[k][mu][nu] = L[k * ld + pos[mu (mu + 1) / 2 + nu]] (mu >= nu; the other triangle from the same value): every element of the [M][N][N] image once
QEMB_CD_HD void unpack_item(int64_t k, int64_t mu, int64_t nu, int64_t N, const double* L, int64_t ld, const int32_t* pos, double* out) {
  const int64_t ij = mu >= nu ? mu * (mu + 1) / 2 + nu : nu * (nu + 1) / 2 + mu;
  out[(k * N + mu) * N + nu] = L[k * ld + pos[ij]];
}

// ---- in-panel factorisation: left-looking pivoted Cholesky of A[c][c'] = E[srow[c] * ld + c'], T[j][c] the j-th new vector at panel column c ----
// order of the pivot search: the larger residual diagonal, the lower column on a tie (a total order: any reduction tree finds the same column)
QEMB_CD_HD bool pivot_better(double va, int ia, double vb, int ib) { return va > vb || (va == vb && ia < ib); }
// the panel's residual diagonal at the start: the running diagonal d of the decomposition (or, without one, the diagonal of the block), rounding residue clamped
QEMB_CD_HD double panel_diag0(const double* E, int64_t ld, const int32_t* srow, const double* d, int c) {
  const double v = d ? d[srow[c]] : E[(int64_t)srow[c] * ld + c];
  return v > 0.0 ? v : 0.0;
}
// Column c of step j with pivot column p, s = sqrt(dd[p]).  dd[c] < 0 marks a column that was a pivot: its entries of later vectors are exact zeros.
QEMB_CD_HD void panel_col(const double* E, int64_t ld, const int32_t* srow, int n, int j, int p, double s, int c, double* T, double* dd) {
  double* Tj = T + (int64_t)j * n;
  if (c == p) { Tj[c] = s; dd[c] = -1.0; return; }
  if (dd[c] < 0.0) { Tj[c] = 0.0; return; }
  double v = E[(int64_t)srow[p] * ld + c];
  for (int i = 0; i < j; ++i) v -= T[(int64_t)i * n + p] * T[(int64_t)i * n + c];
  const double t = v / s, r = dd[c] - t * t;
  Tj[c] = t;
  dd[c] = r > 0.0 ? r : 0.0;
}

// The r new vectors at one plan row: forward substitution of the row's residual integrals with the pivot columns against the triangular factor
//   Lnew[j][row] = (E[row][piv[j]] - sum_{i < j} Lnew[i][row] T[i][piv[j]]) / T[j][piv[j]]
QEMB_CD_HD void newrows_item(int64_t row, int n, int r, const double* E, int64_t ld, const double* T, const int32_t* piv, double* Lnew, int64_t ldl) {
  for (int j = 0; j < r; ++j) {
    const int p = piv[j];
    double v = E[row * ld + p];
    for (int i = 0; i < j; ++i) v -= Lnew[(int64_t)i * ldl + row] * T[(int64_t)i * n + p];
    Lnew[(int64_t)j * ldl + row] = v / T[(int64_t)j * n + p];
  }
}

// d[row] -= sum_k Lnew[k][row]^2; a pivot row becomes exactly 0, negative rounding residue (and a NaN) 0
QEMB_CD_HD void diag_item(int64_t row, int r, const double* Lnew, int64_t ldl, const int32_t* piv, const int32_t* srow, double* d) {
  double acc = 0.0;
  bool is_piv = false;
  for (int k = 0; k < r; ++k) {
    const double l = Lnew[(int64_t)k * ldl + row];
    acc += l * l;
    is_piv = is_piv || srow[piv[k]] == row;
  }
  const double v = d[row] - acc;
  d[row] = (is_piv || !(v > 0.0)) ? 0.0 : v;
}
// the largest residual diagonal of shell pair w (its plan rows are row0[w] .. row0[w] + cnt[w] - 1)
QEMB_CD_HD double pairmax_item(int64_t w, const int32_t* row0, const int32_t* cnt, const double* d) {
  double m = 0.0;
  for (int e = 0; e < cnt[w]; ++e) m = d[row0[w] + e] > m ? d[row0[w] + e] : m;
  return m;
}

// ---- argument checks shared by the two device layers ----
inline int check_gather(int64_t rows, int64_t ncols, const void* in, int64_t ldi, const void* idx, const void* out, int64_t ldo) {
  if (rows < 0 || ncols < 0 || rows > 0x7fffffffLL || ncols > 0x7fffffffLL || !in || !idx || !out || ldi <= 0 || ldo < ncols) { set_error("dev_cd_gather_cols: bad arguments"); return QEMB_ERR_ARG; }
  return 0;
}
inline int check_panel(const void* E, int64_t ld, const void* srow, int n, double thr, const void* T, const void* piv, const void* rank, const void* work) {
  if (!E || !srow || !T || !piv || !rank || !work || n <= 0 || ld < n || !(thr >= 0.0)) { set_error("dev_cd_panel_factor: bad arguments (n = " + std::to_string(n) + ")"); return QEMB_ERR_ARG; }
  return 0;
}
inline int check_new_rows(int64_t np, int n, int r, const void* E, int64_t ld, const void* T, const void* piv, const void* Lnew, int64_t ldl) {
  if (np <= 0 || np > 0x7fffffffLL || n <= 0 || r < 0 || r > n || !E || ld < n || !T || !piv || !Lnew || ldl < np) { set_error("dev_cd_new_rows: bad arguments"); return QEMB_ERR_ARG; }
  return 0;
}
inline int check_diag_update(int64_t np, int r, const void* Lnew, int64_t ldl, const void* piv, const void* srow, const void* d, int64_t nsp, const void* row0, const void* cnt,
                             const void* spmax, const void* partials, const void* dmax) {
  if (np <= 0 || np > 0x7fffffffLL || r < 0 || (r > 0 && (!Lnew || ldl < np || !piv || !srow)) || !d || nsp <= 0 || nsp > np || !row0 || !cnt || !spmax || !partials || !dmax) {
    set_error("dev_cd_diag_update: bad arguments");
    return QEMB_ERR_ARG;
  }
  return 0;
}
inline int check_unpack(int64_t M, int64_t N, const void* L, int64_t ld, const void* pos, const void* out) {
  if (M < 0 || M > 0x7fffffffLL || N <= 0 || N > 32767 || !L || ld < N * (N + 1) / 2 || !pos || !out) { set_error("dev_cd_unpack: bad arguments"); return QEMB_ERR_ARG; }
  return 0;
}

}  // namespace cd
}  // namespace qemb
