// mp2_ops_hostcheck.cpp -- scalar restatement of the device operations of the MP2 path for the mock device layer of tests/hostcheck.
// Everything below is compiled only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and mp2_ops.hip provides the operation.
#ifdef QEMB_HOSTCHECK
#include "dev_ops.h"

namespace qemb {

int dev_mp2_amplitudes(int64_t o, int64_t v, const double* ovov, const double* eo, const double* ev, double* t2, double* G, double* partials, double* e_dev) {
  if (o <= 0 || v <= 0 || !ovov || !eo || !ev || !t2 || !G || !partials || !e_dev) { set_error("dev_mp2_amplitudes: bad arguments"); return QEMB_ERR_ARG; }
  if (t2 == ovov || G == ovov) { set_error("dev_mp2_amplitudes: the outputs may not alias ovov"); return QEMB_ERR_ARG; }
  const int64_t ov = o * v;
  auto iajb = [&](int64_t i, int64_t a, int64_t j, int64_t b) { return (i * v + a) * ov + j * v + b; };
  long double e = 0.0L;
  for (int64_t i = 0; i < o; ++i) for (int64_t j = 0; j < o; ++j) for (int64_t a = 0; a < v; ++a) for (int64_t b = 0; b < v; ++b) {
    const double eij = eo[i] + eo[j];
    const double s = ovov[iajb(i, a, j, b)], p = ovov[iajb(i, b, j, a)];
    const double d = (eij - ev[a]) - ev[b], t = s / d, tp = p / d;      // tp = t2[j,i,a,b]
    t2[((i * o + j) * v + a) * v + b] = t;
    G[iajb(i, a, j, b)] = 2.0 * t - tp;
    e += (long double)(t * (2.0 * s - p));
  }
  partials[0] = (double)e;
  e_dev[0] = (double)e;
  return 0;
}

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
