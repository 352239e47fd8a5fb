// kdf_ops_hostcheck.cpp -- scalar restatement of the device operations of the k-point density-fitted transform for the mock device layer of tests/hostcheck.
// Everything below is compiled only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and kdf_ops.hip provides the operations.
#ifdef QEMB_HOSTCHECK
#include <cmath>
#include "dev_ops.h"

namespace qemb {

int dev_kdf_split(int64_t rows, int64_t nao, const double* z, double* planes) {
  if (rows <= 0 || nao <= 0 || !z || !planes) { set_error("dev_kdf_split: bad arguments"); return QEMB_ERR_ARG; }
  const int64_t ld = kdf_ld(nao);
  for (int64_t r = 0; r < rows; ++r) for (int64_t nu = 0; nu < ld; ++nu) {
    planes[r * 2 * ld + nu] = nu < nao ? z[(r * nao + nu) * 2] : 0.0;
    planes[r * 2 * ld + ld + nu] = nu < nao ? z[(r * nao + nu) * 2 + 1] : 0.0;
  }
  return 0;
}

int dev_kdf_stack(int64_t nk, int64_t nao, int64_t n, const double* ta, double* Cs, double* Dk) {
  if (nk <= 0 || nao <= 0 || n <= 0 || !ta || !Cs || !Dk) { set_error("dev_kdf_stack: bad arguments"); return QEMB_ERR_ARG; }
  const int64_t ld = kdf_ld(nao);
  for (int64_t k = 0; k < nk; ++k) {
    double* cs = Cs + k * 4 * ld * n;
    double* dk = Dk + k * 4 * nao * n;
    for (int64_t i = 0; i < 4 * ld * n; ++i) cs[i] = 0.0;
    for (int64_t nu = 0; nu < nao; ++nu) for (int64_t j = 0; j < n; ++j) {
      const double re = ta[((k * nao + nu) * n + j) * 2], im = ta[((k * nao + nu) * n + j) * 2 + 1];
      cs[nu * 2 * n + j] = re;            cs[nu * 2 * n + n + j] = im;
      cs[(ld + nu) * 2 * n + j] = -im;    cs[(ld + nu) * 2 * n + n + j] = re;
      dk[(2 * nu) * 2 * n + j] = re;      dk[(2 * nu) * 2 * n + n + j] = -im;
      dk[(2 * nu + 1) * 2 * n + j] = im;  dk[(2 * nu + 1) * 2 * n + n + j] = re;
    }
  }
  return 0;
}

int dev_kdf_pack(int64_t naux, int64_t n, const double* M, int paired, double w, double* F, int64_t ldf, double* partials, double* out2_dev) {
  if (int rc = kdf_check_pack(naux, n, M, F, ldf, partials, out2_dev)) return rc;
  double asym = 0.0, amax = 0.0;
  for (int64_t P = 0; P < naux; ++P) for (int c = 0; c < 2; ++c) {
    const double* Mp = M + (P * 2 + c) * n * n;
    for (int64_t a = 0; a < n; ++a) for (int64_t b = 0; b < n; ++b) {
      amax = std::fmax(amax, std::fabs(Mp[a * n + b]));
      if (a < b) continue;
      asym = std::fmax(asym, std::fabs(Mp[a * n + b] - Mp[b * n + a]));
      if (c == 0 || paired) F[((int64_t)c * naux + P) * ldf + a * (a + 1) / 2 + b] = w * Mp[a * n + b];
      else asym = std::fmax(asym, std::fabs(Mp[a * n + b]));
    }
  }
  partials[0] = asym; partials[1] = amax;
  out2_dev[0] = asym; out2_dev[1] = amax;
  return 0;
}

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
