// mo_blocks_ops_hostcheck.cpp -- scalar restatement of the device operations of the lean factor-route set-up (gathers from the pair product S, T in its
// (j,b) rows, OVp / OVm from ovvv in place) for the mock device layer of tests/hostcheck.
// Everything below is compiled only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and dev_ops_hip.hip provides the operations.
#ifdef QEMB_HOSTCHECK
#include <algorithm>
#include "dev_ops.h"

namespace qemb {

static inline int64_t pidx(int64_t i, int64_t j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

int dev_extract_pf_t_compact(int64_t n, const double* T, int64_t x0, int64_t c0, int64_t sx, int64_t sr, int64_t ss, int64_t sc, double* out, int64_t slab) {
  if (slab <= 0) slab = n * n;
  for (int64_t x = 0; x < sx; ++x) for (int64_t r = 0; r < sr; ++r) for (int64_t s = 0; s < ss; ++s) for (int64_t c = 0; c < sc; ++c)
    out[((x * sr + r) * ss + s) * sc + c] = T[(r * ss + s) * slab + (c0 + c) * n + (x0 + x)];
  return 0;
}
int dev_gather_pair_cols(int64_t rows, int64_t n, const double* in, int64_t r0, int64_t s0, int64_t sr, int64_t ss, double* out) {
  const int64_t np = n * (n + 1) / 2;
  for (int64_t L = 0; L < rows; ++L) for (int64_t r = 0; r < sr; ++r) for (int64_t s = 0; s < ss; ++s) out[(L * sr + r) * ss + s] = in[L * np + pidx(r0 + r, s0 + s)];
  return 0;
}
int dev_extract_ps(int64_t n, const double* S, int64_t p0, int64_t q0, int64_t r0, int64_t s0, int64_t sp, int64_t sq, int64_t sr, int64_t ss, double* out) {
  const int64_t np = n * (n + 1) / 2;
  for (int64_t p = 0; p < sp; ++p) for (int64_t q = 0; q < sq; ++q) for (int64_t r = 0; r < sr; ++r) for (int64_t s = 0; s < ss; ++s)
    out[((p * sq + q) * sr + r) * ss + s] = S[pidx(p0 + p, q0 + q) * np + pidx(r0 + r, s0 + s)];
  return 0;
}
int dev_extract_ps_packed(int64_t n, const double* S, int64_t p0, int64_t q0, int64_t r0, int64_t sp, int64_t sq, int64_t sr, double* out) {
  const int64_t np = n * (n + 1) / 2, npr = sr * (sr + 1) / 2;
  for (int64_t p = 0; p < sp; ++p) for (int64_t q = 0; q < sq; ++q) for (int64_t r = 0; r < sr; ++r) for (int64_t s = 0; s <= r; ++s)
    out[(p * sq + q) * npr + pidx(r, s)] = S[pidx(p0 + p, q0 + q) * np + pidx(r0 + r, r0 + s)];
  return 0;
}
int dev_unpack_pair_block(int64_t n, int64_t o, const double* S, double* Mv, int64_t ld) {
  const int64_t v = n - o, np = n * (n + 1) / 2;
  for (int64_t a = 0; a < v; ++a) for (int64_t c = 0; c <= a; ++c) for (int64_t b = 0; b < v; ++b) for (int64_t d = 0; d < v; ++d)
    Mv[(pidx(a, c) * v + b) * ld + d] = S[pidx(o + a, o + c) * np + pidx(o + b, o + d)];
  return 0;
}
int dev_ladder_pack_vvvv_pf_ld(int64_t n, int64_t o, const double* Mp, int64_t ld, double* Vp, int64_t ldp, double* Vm, int64_t ldm) {
  const int64_t v = n - o;
  for (int64_t a = 0; a < v; ++a) for (int64_t b = 0; b <= a; ++b) {
    double* vp = Vp + (a * (a + 1) / 2 + b) * ldp; std::fill(vp, vp + ldp, 0.0);
    double* vm = a > b ? Vm + (a * (a - 1) / 2 + b) * ldm : nullptr; if (vm) std::fill(vm, vm + ldm, 0.0);
    for (int64_t c = 0; c < v; ++c) for (int64_t d = 0; d <= c; ++d) {
      const double x = Mp[(pidx(o + a, o + c) * n + (o + b)) * ld + (o + d)], y = Mp[(pidx(o + b, o + c) * n + (o + a)) * ld + (o + d)];
      vp[c * (c + 1) / 2 + d] = x + y;
      if (vm && c > d) vm[c * (c - 1) / 2 + d] = x - y;
    }
  }
  return 0;
}
int dev_pack_pm_ovvv(int64_t o, int64_t v, const double* in, double* Op, int64_t ldp, double* Om, int64_t ldm) {
  if (v < 32) { set_error("dev_pack_pm_ovvv: tiled pass only (v >= 32)"); return QEMB_ERR_ARG; }
  for (int64_t k = 0; k < o; ++k) for (int64_t a = 0; a < v; ++a) {
    double* tp = Op + (k * v + a) * ldp; std::fill(tp, tp + ldp, 0.0);
    double* tm = Om + (k * v + a) * ldm; std::fill(tm, tm + ldm, 0.0);
    for (int64_t c = 0; c < v; ++c) for (int64_t d = 0; d <= c; ++d) {
      const double x = in[((k * v + d) * v + a) * v + c], y = in[((k * v + c) * v + a) * v + d];
      tp[c * (c + 1) / 2 + d] = x + y;
      if (c > d) tm[c * (c - 1) / 2 + d] = x - y;
    }
  }
  return 0;
}

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
