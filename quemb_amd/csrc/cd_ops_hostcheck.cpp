// cd_ops_hostcheck.cpp -- scalar restatement of the device operations of the Cholesky decomposition of the AO integrals for the mock device layer of
// tests/hostcheck.  Everything below is compiled only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and cd_ops.hip provides the
// operations.  The arithmetic of one item is the inline code of cd_core.h that the kernels instantiate per thread; here the items run in a loop, and the pivot
// search of the panel factorisation walks the columns in order with the same total order (pivot_better) the kernel's reduction tree uses.
#ifdef QEMB_HOSTCHECK
#include "cd_core.h"

namespace qemb {
using namespace cd;

int dev_cd_gather_cols(int64_t rows, int64_t ncols, const double* in, int64_t ldi, const int32_t* idx, double* out, int64_t ldo) {
  if (int rc = check_gather(rows, ncols, in, ldi, idx, out, ldo)) return rc;
  for (int64_t k = 0; k < rows; ++k)
    for (int64_t c = 0; c < ncols; ++c) gather_item(k, c, in, ldi, idx, out, ldo);
  return 0;
}

int dev_cd_unpack(int64_t M, int64_t N, const double* L, int64_t ld, const int32_t* pos, double* out) {
  if (int rc = check_unpack(M, N, L, ld, pos, out)) return rc;
  for (int64_t k = 0; k < M; ++k)
    for (int64_t mu = 0; mu < N; ++mu)
      for (int64_t nu = 0; nu < N; ++nu) unpack_item(k, mu, nu, N, L, ld, pos, out);
  return 0;
}

int dev_cd_panel_factor(const double* E, int64_t ld, const int32_t* srow, int n, double thr, const double* d, double* T, int32_t* piv, int32_t* rank, double* work) {
  if (int rc = check_panel(E, ld, srow, n, thr, T, piv, rank, work)) return rc;
  double* dd = work;
  for (int c = 0; c < n; ++c) dd[c] = panel_diag0(E, ld, srow, d, c);
  int j = 0;
  for (; j < n; ++j) {
    double best = -1.0;
    int p = n;
    for (int c = 0; c < n; ++c)
      if (pivot_better(dd[c], c, best, p)) { best = dd[c]; p = c; }
    if (!(best > thr)) break;
    const double s = std::sqrt(best);
    piv[j] = p;
    for (int c = 0; c < n; ++c) panel_col(E, ld, srow, n, j, p, s, c, T, dd);
  }
  rank[0] = j;
  return 0;
}

int dev_cd_new_rows(int64_t np, int n, int r, const double* E, int64_t ld, const double* T, const int32_t* piv, double* Lnew, int64_t ldl) {
  if (int rc = check_new_rows(np, n, r, E, ld, T, piv, Lnew, ldl)) return rc;
  for (int64_t row = 0; row < np; ++row) newrows_item(row, n, r, E, ld, T, piv, Lnew, ldl);
  return 0;
}

int dev_cd_diag_update(int64_t np, int r, const double* Lnew, int64_t ldl, const int32_t* piv, const int32_t* srow, double* d, int64_t nsp, const int32_t* row0, const int32_t* cnt,
                       double* spmax, double* partials, double* dmax) {
  if (int rc = check_diag_update(np, r, Lnew, ldl, piv, srow, d, nsp, row0, cnt, spmax, partials, dmax)) return rc;
  for (int64_t row = 0; row < np && r > 0; ++row) diag_item(row, r, Lnew, ldl, piv, srow, d);
  const int64_t nb = pair_max_partials(nsp);
  for (int64_t b = 0; b < nb; ++b) partials[b] = 0.0;
  for (int64_t w = 0; w < nsp; ++w) {
    spmax[w] = pairmax_item(w, row0, cnt, d);
    if (spmax[w] > partials[w / 256]) partials[w / 256] = spmax[w];
  }
  double m = 0.0;
  for (int64_t b = 0; b < nb; ++b) m = partials[b] > m ? partials[b] : m;
  dmax[0] = m;
  return 0;
}

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
