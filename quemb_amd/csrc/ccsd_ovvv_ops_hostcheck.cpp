// ccsd_ovvv_ops_hostcheck.cpp -- scalar restatement of the one-pass ovvv operations (dev_ops.h: dev_ccsd_ovvv_pass, dev_ccsd_ovvv_slabs,
// dev_ccsd_ph_layouts_ring) for the mock device layer of tests/hostcheck.
// Everything below is compiled only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and ccsd_ovvv_ops.hip / dev_ops_hip.hip
// provide the operations.
#ifdef QEMB_HOSTCHECK
#include <algorithm>
#include "dev_ops.h"

namespace qemb {

// (a handful of "workgroups": more than the slabs of the smallest shapes, so that idle ones occur here too)
int dev_ccsd_ovvv_slabs(int64_t o, int64_t v) { return ccsd_ovvv_shape_ok(o, v) ? 6 : 0; }

int dev_ccsd_ovvv_pass(int64_t o, int64_t v, const double* ovvv, const double* t1, const double* Thk, double* ZB, double* PA) {
  if (!ccsd_ovvv_shape_ok(o, v)) { set_error("dev_ccsd_ovvv_pass: shape outside the kernel's limits (ccsd_ovvv_shape_ok)"); return QEMB_ERR_ARG; }
  if (!ovvv || !t1 || !Thk || !ZB || !PA) { set_error("dev_ccsd_ovvv_pass: bad arguments"); return QEMB_ERR_ARG; }
  const int64_t G = dev_ccsd_ovvv_slabs(o, v), nslab = o * v;
  for (int64_t g = 0; g < G; ++g) {
    double* pa = PA + g * o * v;
    std::fill(pa, pa + o * v, 0.0);
    for (int64_t s = g * nslab / G; s < (g + 1) * nslab / G; ++s) {
      const double* A = ovvv + s * v * v;
      const double* Th = Thk + s * o * v;
      for (int64_t a = 0; a < v; ++a) for (int64_t i = 0; i < o; ++i) {
        double zb = 0.0, p = 0.0;
        for (int64_t d = 0; d < v; ++d) { zb += A[a * v + d] * t1[i * v + d]; p += A[a * v + d] * Th[i * v + d]; }
        ZB[(s * v + a) * o + i] = zb;
        pa[i * v + a] += p;
      }
    }
  }
  return 0;
}

int dev_ccsd_ph_layouts_ring(int64_t o, int64_t v, const double* t2, const double* t1, double* Tp, double* S, double* Ut, double* Tpt) {
  for (int64_t k = 0; k < o; ++k) for (int64_t j = 0; j < o; ++j) for (int64_t c = 0; c < v; ++c) for (int64_t b = 0; b < v; ++b) {
    const double x = t2[((k * o + j) * v + c) * v + b], xp = t2[((k * o + j) * v + b) * v + c], tt = 2.0 * t1[j * v + c] * t1[k * v + b];
    const int64_t off = ((k * v + c) * o + j) * v + b;
    Tp[off] = xp;
    S[off] = 2.0 * x - xp;
    Ut[off] = 2.0 * x - xp - tt;
    Tpt[off] = xp + tt;
  }
  return 0;
}

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
