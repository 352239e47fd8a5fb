// ccsd_t_ops_hostcheck.cpp -- scalar restatement of the device operations of the perturbative triples correction for the mock device layer of tests/hostcheck.
// Everything below is compiled only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and ccsd_t_ops.hip provides the operations.
// The elements of a tile triple one after another through the arithmetic of ccsd_t_core.h (W and V of every ijk in two host arrays -- the kernel's global form); the sums are plain ascending loops.
#ifdef QEMB_HOSTCHECK
#include <vector>
#include "ccsd_t_core.h"

namespace qemb {

int dev_ccsd_t_assemble(const CcsdTArgs& A) {
  if (const char* bad = ccsd_t_args_error(A)) { set_error(bad); return QEMB_ERR_ARG; }
  const int o = A.o, oo = o * o, o3 = oo * o;
  std::vector<double> W((size_t)o3), V((size_t)o3);
  for (int la = 0; la < A.ta; ++la) for (int lb = 0; lb < A.tb; ++lb) for (int lc = 0; lc < A.tc; ++lc) {
    const int a = A.a0 + la, b = A.b0 + lb, c = A.c0 + lc;
    double& out = A.partial[((int64_t)la * A.tb + lb) * A.tc + lc];
    out = 0.0;
    if (!ccsd_t_evaluated(a, b, c)) continue;
    for (int e = 0; e < o3; ++e) {
      const int i = e / oo, j = (e - i * oo) / o, k = e - i * oo - j * o;
      ccsd_t_element(A, la, lb, lc, i, j, k, &W[(size_t)e], &V[(size_t)e]);
    }
    const double eabc = (A.ev[a] + A.ev[b]) + A.ev[c];
    double acc = 0.0;
    for (int e = 0; e < o3; ++e) {
      const int i = e / oo, j = (e - i * oo) / o, k = e - i * oo - j * o;
      acc += W[(size_t)e] * ccsd_t_r3(V.data(), o, i, j, k) / (((A.eo[i] + A.eo[j]) + A.eo[k]) - eabc);
    }
    out = acc * (ccsd_t_weight(a, b, c) / 3.0);
  }
  return 0;
}

int dev_ccsd_t_sum(int64_t m, const double* in, double* out, int64_t slot) {
  if (m <= 0 || !in || !out || slot < 0) { set_error("dev_ccsd_t_sum: bad arguments"); return QEMB_ERR_ARG; }
  double s = 0.0;
  for (int64_t k = 0; k < m; ++k) s += in[k];
  out[slot] = s;
  return 0;
}

int dev_ccsd_t_total(int64_t m, const double* in, double* out) {
  if (m <= 0 || !in || !out) { set_error("dev_ccsd_t_total: bad arguments"); return QEMB_ERR_ARG; }
  double s = 0.0;
  for (int64_t k = 0; k < m; ++k) s += in[k];
  out[0] = s;
  return 0;
}

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
