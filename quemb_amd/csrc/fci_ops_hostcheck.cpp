// fci_ops_hostcheck.cpp -- scalar restatement of the device operations of the determinant-space FCI for the mock device layer of tests/hostcheck.
// Everything below is compiled only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and fci_ops.hip provides the operations.
// Written as scatters over the links (zero, then one statement per link), not determinant by determinant like the kernels.
#ifdef QEMB_HOSTCHECK
#include <cmath>
#include "dev_ops.h"

namespace qemb {

int dev_fci_gather_slab(int n, int64_t ns, int nlink, const int32_t* links, const double* c, int64_t a0, int64_t a1, double* Ds) {
  if (int rc = fci_check_args("dev_fci_gather_slab", n, ns, nlink, links, c, Ds)) return rc;
  if (int rc = fci_check_slab("dev_fci_gather_slab", ns, a0, a1)) return rc;
  const int64_t Ns = (a1 - a0) * ns, n2 = (int64_t)n * n;
  for (int64_t k = 0; k < n2 * Ns; ++k) Ds[k] = 0.0;
  for (int l = 0; l < nlink; ++l) for (int64_t I = 0; I < ns; ++I) {
    const int32_t w = links[(int64_t)l * ns + I];
    const int64_t J = w >> 9, pq = (w >> 1) & 255;
    const double sg = (w & 1) ? -1.0 : 1.0;
    if (I >= a0 && I < a1) for (int64_t K = 0; K < ns; ++K) Ds[pq * Ns + (I - a0) * ns + K] += sg * c[J * ns + K];      // alpha: the link's own string is the row
    for (int64_t K = a0; K < a1; ++K) Ds[pq * Ns + (K - a0) * ns + I] += sg * c[K * ns + J];                              // beta: every row of the slab
  }
  return 0;
}

int dev_fci_sigma_slab(int n, int64_t ns, int nlink, const int32_t* links, const double* k, int64_t a0, int64_t a1, const double* Ds, const double* Gs, double* sigma) {
  if (int rc = fci_check_args("dev_fci_sigma_slab", n, ns, nlink, links, Ds, sigma)) return rc;
  if (int rc = fci_check_slab("dev_fci_sigma_slab", ns, a0, a1)) return rc;
  if (!k || !Gs) { set_error("dev_fci_sigma_slab: bad arguments"); return QEMB_ERR_ARG; }
  const int64_t N = ns * ns, Ns = (a1 - a0) * ns, n2 = (int64_t)n * n;
  if (a0 == 0) for (int64_t I = 0; I < N; ++I) sigma[I] = 0.0;
  for (int64_t pq = 0; pq < n2; ++pq) for (int64_t t = 0; t < Ns; ++t) sigma[a0 * ns + t] += k[pq] * Ds[pq * Ns + t];
  for (int l = 0; l < nlink; ++l) for (int64_t I = 0; I < ns; ++I) {
    const int32_t w = links[(int64_t)l * ns + I];
    const int64_t J = w >> 9, pq = (w >> 1) & 255;
    const double sg = (w & 1) ? -0.5 : 0.5;
    if (J >= a0 && J < a1) for (int64_t K = 0; K < ns; ++K) sigma[I * ns + K] += sg * Gs[pq * Ns + (J - a0) * ns + K];      // alpha: the source row lies in the slab
    for (int64_t K = a0; K < a1; ++K) sigma[K * ns + I] += sg * Gs[pq * Ns + (K - a0) * ns + J];                             // beta: the row is its own source row
  }
  return 0;
}

int dev_fci_diag(int n, int64_t ns, const int32_t* strings, const double* h, const double* V, double* hdiag) {
  if (int rc = fci_check_args("dev_fci_diag", n, ns, 1, strings, h, hdiag)) return rc;
  if (!V) { set_error("dev_fci_diag: bad arguments"); return QEMB_ERR_ARG; }
  const int64_t n2 = (int64_t)n * n;
  auto Jm = [&](int i, int j) { return V[(int64_t)(i * n + i) * n2 + j * n + j]; };
  auto Km = [&](int i, int j) { return V[(int64_t)(i * n + j) * n2 + j * n + i]; };
  for (int64_t Ia = 0; Ia < ns; ++Ia) for (int64_t Ib = 0; Ib < ns; ++Ib) {
    const unsigned a = (unsigned)strings[Ia], b = (unsigned)strings[Ib];
    double e = 0.0;
    for (int i = 0; i < n; ++i) {
      const int ai = (a >> i) & 1, bi = (b >> i) & 1;
      e += (ai + bi) * h[i * n + i];
      for (int j = 0; j < n; ++j) {
        const int aj = (a >> j) & 1, bj = (b >> j) & 1;
        e += 0.5 * (ai * aj + bi * bj) * (Jm(i, j) - Km(i, j)) + ai * bj * Jm(i, j);
      }
    }
    hdiag[Ia * ns + Ib] = e;
  }
  return 0;
}

int dev_fci_precond(int64_t N, const double* r, const double* hdiag, double theta, double* out) {
  if (N <= 0 || N > kFciMaxDet || !r || !hdiag || !out) { set_error("dev_fci_precond: bad arguments"); return QEMB_ERR_ARG; }
  for (int64_t I = 0; I < N; ++I) {
    double d = hdiag[I] - theta;
    if (std::fabs(d) < 1e-8) d = d < 0.0 ? -1e-8 : 1e-8;
    out[I] = r[I] / d;
  }
  return 0;
}

int dev_fci_dm2(int n, int o_cum, const double* A, const double* dm1, double* out) {
  if (n <= 0 || n > kFciMaxOrb || o_cum > n || !A || !dm1 || !out) { set_error("dev_fci_dm2: bad arguments"); return QEMB_ERR_ARG; }
  const int64_t n2 = (int64_t)n * n, n3 = n2 * n;
  auto at = [&](int64_t p, int64_t q, int64_t r, int64_t s) -> double& { return out[p * n3 + q * n2 + r * n + s]; };
  for (int p = 0; p < n; ++p) for (int q = 0; q < n; ++q) for (int r = 0; r < n; ++r) for (int s = 0; s < n; ++s) at(p, q, r, s) = A[(q * n + p) * n2 + r * n + s];
  for (int p = 0; p < n; ++p) for (int q = 0; q < n; ++q) for (int s = 0; s < n; ++s) at(p, q, q, s) -= dm1[p * n + s];
  if (o_cum >= 0) {      // the statements of molbe/solver.py:513-527
    auto hf = [&](int i, int j) { return (i == j && i < o_cum) ? 2.0 : 0.0; };
    auto del = [&](int i, int j) { return dm1[i * n + j] - hf(i, j); };
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) for (int k = 0; k < n; ++k) for (int l = 0; l < n; ++l) {
      at(i, j, k, l) -= hf(i, j) * hf(k, l) + hf(i, j) * del(k, l) + del(i, j) * hf(k, l);
      at(i, k, l, j) += 0.5 * (hf(i, j) * hf(k, l) + hf(i, j) * del(k, l) + del(i, j) * hf(k, l));
    }
  }
  return 0;
}

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
