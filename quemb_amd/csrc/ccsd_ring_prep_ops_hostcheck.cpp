// ccsd_ring_prep_ops_hostcheck.cpp -- scalar restatement of the one-pass ring preparation (dev_ops.h: dev_ccsd_ring_prep) for the mock device layer of
// tests/hostcheck.  Everything below is compiled only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and ccsd_ring_prep_ops.hip
// provides the operation.
#ifdef QEMB_HOSTCHECK
#include "dev_ops.h"

namespace qemb {

int dev_ccsd_ring_prep(int64_t o, int64_t v, const double* t1, const double* P1, const double* W1base, const double* W2base, const double* ZB, const double* ZC,
                       const double* OB, const double* OC, double* R, double* W2) {
  if (!ccsd_ring_prep_shape_ok(o, v)) { set_error("dev_ccsd_ring_prep: shape outside the kernel's limits (ccsd_ring_prep_shape_ok)"); return QEMB_ERR_ARG; }
  if (!t1 || !P1 || !W1base || !W2base || !ZB || !ZC || !OB || !OC || !R || !W2) { set_error("dev_ccsd_ring_prep: bad arguments"); return QEMB_ERR_ARG; }
  for (int64_t i = 0; i < o; ++i) for (int64_t a = 0; a < v; ++a) for (int64_t k = 0; k < o; ++k) for (int64_t c = 0; c < v; ++c) {
    const double* ob = OB + ((k * o + i) * o) * v + c;
    const double* oc = OC + ((k * o + i) * o) * v + c;
    double sB = 0.0, sC = 0.0;      // from zero, ascending l: the order of the kernel
    for (int64_t l = 0; l < o; ++l) { sB += t1[l * v + a] * ob[l * v]; sC += t1[l * v + a] * oc[l * v]; }
    const int64_t off = ((i * v + a) * o + k) * v + c;
    const double w = (W2base[off] + ZC[((k * o + i) * v + a) * v + c]) - sC;
    W2[off] = w;
    R[off] = (((P1[off] + W1base[off]) + ZB[((k * v + c) * v + a) * o + i]) - sB) - 0.5 * w;
  }
  return 0;
}

int dev_ccsd_u_update(int64_t o, int64_t v, const double* A, const double* t1, const double* Z, double* U) {
  if (!ccsd_ring_prep_shape_ok(o, v)) { set_error("dev_ccsd_u_update: shape outside the kernel's limits (ccsd_ring_prep_shape_ok)"); return QEMB_ERR_ARG; }
  if (!A || !t1 || !Z || !U) { set_error("dev_ccsd_u_update: bad arguments"); return QEMB_ERR_ARG; }
  for (int64_t i = 0; i < o; ++i) for (int64_t j = 0; j < o; ++j) for (int64_t a = 0; a < v; ++a) for (int64_t b = 0; b < v; ++b) {
    double s = 0.0;      // from zero, ascending k: the order of the kernel
    for (int64_t k = 0; k < o; ++k) s += A[((i * o + j) * o + k) * v + a] * t1[k * v + b];
    double& u = U[((i * o + j) * v + a) * v + b];
    u = (u + Z[((i * v + a) * v + b) * o + j]) - s;
  }
  return 0;
}

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
