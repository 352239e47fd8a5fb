// loc_ops_hostcheck.cpp -- scalar restatement of the joint diagonalisation of loc_ops.hip for the mock device layer of tests/hostcheck.  Everything below is compiled
// only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and loc_ops.hip provides the operation.  The arithmetic of one item is the inline code
// of loc_core.h that the kernels instantiate per thread; here the items run in a loop.  The variant is chosen as on the device (in_lds) and its partial sums are added
// in the variant's own order: part s = k mod kLdsParts in the one-workgroup variant, slab b = k / kSlab in the launch-per-round variant.
#ifdef QEMB_HOSTCHECK
#include <vector>
#include "loc_core.h"

namespace qemb {
using namespace loc;

namespace {
void stack_sums(int K, int m, const double* Q, bool lds, double* f, double* n2) {
  const int nparts = lds ? kThreads : (int)slabs(K);
  std::vector<double> pf(nparts, 0.0), pn(nparts, 0.0);
  if (lds) {
    for (int k = 0; k < K; ++k) matrix_sums(Q + (int64_t)k * m * m, m, pf[k % kThreads], pn[k % kThreads]);
  } else {
    for (int b = 0; b < nparts; ++b)
      for (int k = b * kSlab; k < K && k < (b + 1) * kSlab; ++k) {
        double fa = 0.0, na = 0.0;      // the rows t, t + 256, .. of the matrix per thread, the 256 partials in order
        for (int t = 0; t < kThreads; ++t) {
          double a = 0.0, c = 0.0;
          matrix_sums_rows(Q + (int64_t)k * m * m, m, t, kThreads, a, c);
          fa += a; na += c;
        }
        pf[b] += fa; pn[b] += na;
      }
  }
  *f = 0.0; *n2 = 0.0;
  for (int b = 0; b < nparts; ++b) { *f += pf[b]; *n2 += pn[b]; }
}
}  // namespace

int dev_joint_diag(int64_t K64, int64_t m64, double* Q, double* U, double stop_angle, int max_sweeps, int* sweeps_out, double* f_out, int* converged_out) {
  if (int rc = check_joint_diag("dev_joint_diag", K64, m64, Q != nullptr, U != nullptr, stop_angle, max_sweeps)) return rc;
  const int K = (int)K64, m = (int)m64;
  int sweeps = 0, converged = 1;
  double f = 0.0, n2 = 0.0;
  for (int e = 0; e < m * m; ++e) U[e] = (e / m == e % m) ? 1.0 : 0.0;
  const bool lds = in_lds(K, m);
  if (K > 0 && m > 0) {
    stack_sums(K, m, Q, lds && m > 1 && max_sweeps > 0, &f, &n2);
    converged = m == 1;
  }
  if (K > 0 && m > 1 && max_sweeps > 0) {
    const int np = (m + 1) & ~1, npairs = np / 2;
    const int nparts = lds ? kLdsParts : (int)slabs(K);
    std::vector<double> cs(2 * npairs);
    std::vector<int> pq(2 * npairs);
    while (sweeps < max_sweeps) {
      double thmax = 0.0;
      for (int r = 0; r < np - 1; ++r) {
        for (int j = 0; j < npairs; ++j) {
          int p, q;
          rr_pair(np, r, j, p, q);
          double theta = 0.0;
          if (q < m) {
            double saa = 0.0, sdd = 0.0, sad = 0.0;
            for (int s = 0; s < nparts; ++s) {
              double paa = 0.0, pdd = 0.0, pad = 0.0;
              if (lds)
                for (int k = s; k < K; k += kLdsParts) pair_terms(Q + (int64_t)k * m * m, m, p, q, paa, pdd, pad);
              else
                for (int k = s * kSlab; k < K && k < (s + 1) * kSlab; ++k) pair_terms(Q + (int64_t)k * m * m, m, p, q, paa, pdd, pad);
              saa += paa; sdd += pdd; sad += pad;
            }
            theta = pair_angle(saa, sdd, sad, n2);
          }
          pq[2 * j] = p; pq[2 * j + 1] = q;
          cs[2 * j] = std::cos(theta); cs[2 * j + 1] = std::sin(theta);
          if (!(std::fabs(theta) <= thmax)) thmax = std::fabs(theta);
        }
        for (int k = 0; k < K; ++k)
          for (int j = 0; j < npairs; ++j)
            for (int x = 0; x < m; ++x)
              if (pq[2 * j + 1] < m && cs[2 * j + 1] != 0.0) rotate_rows(Q + (int64_t)k * m * m, m, pq[2 * j], pq[2 * j + 1], x, cs[2 * j], cs[2 * j + 1]);
        for (int k = 0; k <= K; ++k)
          for (int x = 0; x < m; ++x)
            for (int j = 0; j < npairs; ++j)
              if (pq[2 * j + 1] < m && cs[2 * j + 1] != 0.0) rotate_cols(k < K ? Q + (int64_t)k * m * m : U, m, pq[2 * j], pq[2 * j + 1], x, cs[2 * j], cs[2 * j + 1]);
      }
      ++sweeps;
      if (thmax < stop_angle) { converged = 1; break; }
    }
    double n2_end;
    stack_sums(K, m, Q, lds, &f, &n2_end);
  }
  if (!std::isfinite(f)) { set_error("dev_joint_diag: the stack holds a NaN or an infinity"); return QEMB_ERR_NUMERIC; }
  if (sweeps_out) *sweeps_out = sweeps;
  if (f_out) *f_out = f;
  if (converged_out) *converged_out = converged;
  return QEMB_OK;
}

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
