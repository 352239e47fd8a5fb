// rdm2_ops_hostcheck.cpp -- scalar restatement of the device operation of the fragment 2-RDM for the mock device layer of tests/hostcheck.
// Everything below is compiled only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and rdm2_ops.hip provides the operation.
// Written statement by statement like the reference (zero-fill, block placement, then the dm1 updates), not element by element like the kernel.
#ifdef QEMB_HOSTCHECK
#include <vector>
#include "dev_ops.h"

namespace qemb {

int dev_rdm2_assemble(int kind, int64_t o, int64_t v, const double* t1, const double* t2, const double* dm1c, double* out) {
  if (int rc = rdm2_check_args(kind, o, v, t1, t2, out)) return rc;
  const int64_t n = o + v, n2 = n * n, n3 = n2 * n;
  auto at = [&](int64_t p, int64_t q, int64_t r, int64_t s) -> double& { return out[p * n3 + q * n2 + r * n + s]; };
  auto T2 = [&](int64_t i, int64_t j, int64_t a, int64_t b) { return t2[((i * o + j) * v + a) * v + b]; };
  for (int64_t k = 0; k < n2 * n2; ++k) out[k] = 0.0;
  std::vector<double> dovov((size_t)(o * v * o * v));
  auto D = [&](int64_t i, int64_t a, int64_t j, int64_t b) -> double& { return dovov[(size_t)(((i * v + a) * o + j) * v + b)]; };
  for (int64_t i = 0; i < o; ++i) for (int64_t a = 0; a < v; ++a) for (int64_t j = 0; j < o; ++j) for (int64_t b = 0; b < v; ++b) {
    if (kind == QEMB_RDM2_CCSD) {
      const double g_ijab = 0.5 * (t1[i * v + a] * t1[j * v + b] + T2(i, j, a, b)), g_jiab = 0.5 * (t1[j * v + a] * t1[i * v + b] + T2(j, i, a, b));
      D(i, a, j, b) = 2.0 * g_ijab - g_jiab;
    } else {
      D(i, a, j, b) = 2.0 * (2.0 * T2(i, j, a, b) - T2(i, j, b, a));
    }
  }
  for (int64_t i = 0; i < o; ++i) for (int64_t a = 0; a < v; ++a) for (int64_t j = 0; j < o; ++j) for (int64_t b = 0; b < v; ++b) {
    const double x = kind == QEMB_RDM2_CCSD ? D(i, a, j, b) + D(j, b, i, a) : D(i, a, j, b);
    at(i, o + a, j, o + b) = x;
    at(o + a, i, o + b, j) = x;
  }
  if (dm1c) {
    auto d = [&](int64_t p, int64_t q) { return dm1c[p * n + q]; };
    for (int64_t i = 0; i < o; ++i) for (int64_t p = 0; p < n; ++p) for (int64_t q = 0; q < n; ++q) {
      at(i, i, p, q) += 2.0 * d(p, q);
      at(p, q, i, i) += 2.0 * d(p, q);
      at(p, i, i, q) -= d(p, q);
      at(i, p, q, i) -= d(q, p);
    }
    for (int64_t i = 0; i < o; ++i) for (int64_t j = 0; j < o; ++j) { at(i, i, j, j) += 4.0; at(i, j, j, i) -= 2.0; }
  }
  return 0;
}

int dev_rdm2_add_nc(int64_t m, const double* g, double alpha, double* X) {
  if (int rc = rdm2_check_full(m, g, X)) return rc;
  for (int64_t i = 0; i < m; ++i) for (int64_t j = 0; j < m; ++j) for (int64_t k = 0; k < m; ++k) for (int64_t l = 0; l < m; ++l)
    X[((i * m + j) * m + k) * m + l] += alpha * (g[i * m + j] * g[k * m + l] - 0.5 * g[i * m + l] * g[j * m + k]);
  return 0;
}

int dev_rdm2_symmetrize(int64_t m, const double* g, double* X) {
  if (int rc = rdm2_check_full(m, X, X)) return rc;
  const int64_t m4 = m * m * m * m;
  std::vector<double> Y(X, X + m4);
  for (int64_t p = 0; p < m; ++p) for (int64_t q = 0; q < m; ++q) for (int64_t r = 0; r < m; ++r) for (int64_t s = 0; s < m; ++s) {
    double x = 0.5 * (Y[((p * m + q) * m + r) * m + s] + Y[((s * m + r) * m + q) * m + p]);
    if (g) x += g[p * m + q] * g[r * m + s] - 0.5 * g[p * m + s] * g[q * m + r];
    X[((p * m + q) * m + r) * m + s] = x;
  }
  return 0;
}

int dev_rdm2_eri_dot(int64_t m, int sym, const double* eri, const double* K, double* partials, double* out_dev) {
  if (int rc = rdm2_check_full(m, eri, K)) return rc;
  if ((sym != 1 && sym != 4 && sym != 8) || !partials || !out_dev) { set_error("dev_rdm2_eri_dot: sym must be 1, 4 or 8 and the outputs non-null"); return QEMB_ERR_ARG; }
  auto pair = [](int64_t a, int64_t b) { return a >= b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; };
  const int64_t np = m * (m + 1) / 2;
  double e = 0.0;
  for (int64_t p = 0; p < m; ++p) for (int64_t q = 0; q < m; ++q) for (int64_t r = 0; r < m; ++r) for (int64_t s = 0; s < m; ++s) {
    const int64_t full = ((p * m + q) * m + r) * m + s;
    const int64_t at = sym == 1 ? full : sym == 4 ? pair(p, q) * np + pair(r, s) : pair(pair(p, q), pair(r, s));
    e += eri[at] * K[full];
  }
  out_dev[0] = e;
  return 0;
}

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
