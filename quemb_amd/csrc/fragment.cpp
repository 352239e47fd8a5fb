#include <atomic>
// fragment.cpp -- the per-fragment pipeline on the device:
//   fragment RHF (helper.py:73-151) -> embedding->MO integrals (solver.py:900) -> RCCSD (solver.py:907)
//   -> unrelaxed 1-RDM (ccsd_rdm.py:10-20) back-rotated (solver.py:496-505) -> fragment energy (helper.py:220-339)
// with the fragment ERIs resident in HBM between sweeps (the reference re-reads them from HDF5 every call:
// helper.py:182-189, :303-304).
#include "fragment.h"
#include "ao2mo.h"
#include "mp2.h"
#include <string>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <cmath>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <unistd.h>

namespace qemb {

static inline int64_t npair(int64_t n) { return n * (n + 1) / 2; }

int Fragment::set_eri_s4_host(const double* s4) {
  const int64_t np = npair(n_);
  clear_df_factor(); s4_transient_.release();
  QTRY(eri_s4_.alloc(np * np));
  return dev_h2d(eri_s4_, s4, sizeof(double) * np * np);
}
int Fragment::set_eri_s4_dev(const double* s4_dev) {
  const int64_t np = npair(n_);
  clear_df_factor();
  QTRY(eri_s4_.alloc(np * np));
  return dev_d2d(eri_s4_, s4_dev, sizeof(double) * np * np);
}
int Fragment::adopt_eri_s4(DBuf&& s4) {
  const int64_t np = npair(n_);
  if (s4.n != np * np || !s4.p) { set_error("adopt_eri_s4: block of the wrong size"); return QEMB_ERR_ARG; }
  clear_df_factor();
  eri_s4_ = std::move(s4);
  return 0;
}
// ---- the fragment's 3-index factor B[naux][npair(n)] (eri = B^T B): set AFTER the ERIs it belongs to (new ERIs drop it)
void Fragment::clear_df_factor() { df_factor_.release(); df_naux_ = 0; forget_solve(); }      // (every setter of ERIs or of a factor comes through here or adopts)
// A factor that does not belong to the resident ERIs would give a fragment RHF (which reads the block) and amplitude equations (which would read the
// factor) of two different Hamiltonians, silently.  When the factor is set the WHOLE block is probed: for two fixed pseudo-random vectors x the products
// B^T (B x) and eri_s4 x must agree (two gemv-sized passes; round 4 compared the leading 16 x 16 corner only, which a factor that is stale, truncated or
// of a fragment sharing its first pairs passes).  Any failure on the way leaves the fragment WITHOUT a factor.
int Fragment::check_df_factor() {
  if (!eri_s4_.p) return 0;
  const int64_t np = npair(n_);
  constexpr int NV = 2;
  std::vector<double> x((size_t)(np * NV));
  uint64_t st = 0x9E3779B97F4A7C15ull ^ (uint64_t)np;
  for (double& e : x) { st = st * 6364136223846793005ull + 1442695040888963407ull; e = (double)((st >> 11) & ((1ull << 53) - 1)) / (double)(1ull << 52) - 1.0; }
  DBuf X, Z, Y1, Y2;
  QTRY(X.alloc(np * NV)); QTRY(Z.alloc((int64_t)df_naux_ * NV)); QTRY(Y1.alloc(np * NV)); QTRY(Y2.alloc(np * NV));
  QTRY(dev_h2d(X, x.data(), sizeof(double) * np * NV));
  QTRY(gemm((int64_t)df_naux_, NV, np, 1.0, df_factor_, np, true, X, NV, false, 0.0, Z, NV));        // Z = B X
  QTRY(gemm(np, NV, (int64_t)df_naux_, 1.0, df_factor_, np, false, Z, NV, false, 0.0, Y1, NV));       // Y1 = B^T Z
  QTRY(gemm(np, NV, np, 1.0, eri_s4_, np, true, X, NV, false, 0.0, Y2, NV));                          // Y2 = eri_s4 X
  std::vector<double> y1((size_t)(np * NV)), y2((size_t)(np * NV));
  QTRY(dev_d2h(y1.data(), Y1, sizeof(double) * np * NV));
  QTRY(dev_d2h(y2.data(), Y2, sizeof(double) * np * NV));
  double worst = 0.0, scale = 1.0;
  for (size_t k = 0; k < y1.size(); ++k) { worst = std::max(worst, std::fabs(y1[k] - y2[k])); scale = std::max(scale, std::fabs(y2[k])); }
  if (!(worst <= 1e-9 * scale)) {
    set_error("set_df_factor: B^T B x differs from the fragment's ERI block applied to x by " + std::to_string(worst) + " (random probe of the whole block): not the factor of these ERIs");
    return QEMB_ERR_ARG;
  }
  return 0;
}
int Fragment::set_df_factor_host(int naux, const double* B) {
  if (naux <= 0 || !B) { set_error("set_df_factor: need naux > 0 and the factor"); return QEMB_ERR_ARG; }
  clear_df_factor();
  int rc = df_factor_.alloc((int64_t)naux * npair(n_));
  if (rc == 0) { df_naux_ = naux; rc = dev_h2d(df_factor_, B, sizeof(double) * naux * npair(n_)); }
  if (rc == 0) rc = check_df_factor();
  if (rc != 0) clear_df_factor();      // a half-set or refused factor is not kept
  return rc;
}
int Fragment::set_df_factor_dev(int naux, const double* B_dev) {
  if (naux <= 0 || !B_dev) { set_error("set_df_factor: need naux > 0 and the factor"); return QEMB_ERR_ARG; }
  clear_df_factor();
  int rc = df_factor_.alloc((int64_t)naux * npair(n_));
  if (rc == 0) { df_naux_ = naux; rc = dev_d2d(df_factor_, B_dev, sizeof(double) * naux * npair(n_)); }
  if (rc == 0) rc = check_df_factor();
  if (rc != 0) clear_df_factor();
  return rc;
}
int Fragment::set_df_only_host(int naux, const double* B) {
  if (naux <= 0 || !B) { set_error("set_df_only: need naux > 0 and the factor"); return QEMB_ERR_ARG; }
  eri_s4_.release(); s4_transient_.release(); clear_df_factor();
  int rc = df_factor_.alloc((int64_t)naux * npair(n_));
  if (rc == 0) { df_naux_ = naux; rc = dev_h2d(df_factor_, B, sizeof(double) * naux * npair(n_)); }
  if (rc != 0) clear_df_factor();
  return rc;
}
int Fragment::set_df_only_dev(int naux, const double* B_dev) {
  if (naux <= 0 || !B_dev) { set_error("set_df_only: need naux > 0 and the factor"); return QEMB_ERR_ARG; }
  eri_s4_.release(); s4_transient_.release(); clear_df_factor();
  int rc = df_factor_.alloc((int64_t)naux * npair(n_));
  if (rc == 0) { df_naux_ = naux; rc = dev_d2d(df_factor_, B_dev, sizeof(double) * naux * npair(n_)); }
  if (rc != 0) clear_df_factor();
  return rc;
}
int Fragment::adopt_df_only(DBuf&& B, int naux) {
  if (naux <= 0 || !B.p || B.n != (int64_t)naux * npair(n_)) { set_error("adopt_df_only: factor of the wrong size"); return QEMB_ERR_ARG; }
  eri_s4_.release(); s4_transient_.release(); forget_solve();
  df_factor_ = std::move(B); df_naux_ = naux;
  return 0;
}
int Fragment::materialize_s4(DBuf& out) {
  if (!df_factor_.p) { set_error("Fragment: no factor to form the ERI block from"); return QEMB_ERR_ARG; }
  const int64_t np = npair(n_);
  QTRY(out.alloc(np * np));
  return df_pair_product(np, df_naux_, df_factor_, out);
}
int Fragment::export_df_factor(double* B_host) {
  if (!df_factor_.p) { set_error("fragment has no 3-index factor"); return QEMB_ERR_ARG; }
  return dev_d2h(B_host, df_factor_, sizeof(double) * df_naux_ * npair(n_));
}
int Fragment::export_eri_s4(double* s4_host) {
  const int64_t np = npair(n_);
  if (eri_s4_.p) return dev_d2h(s4_host, eri_s4_, sizeof(double) * np * np);
  if (!df_factor_.p) { set_error("fragment has no ERIs"); return QEMB_ERR_ARG; }
  DBuf tmp;
  QTRY(materialize_s4(tmp));
  return dev_d2h(s4_host, tmp, sizeof(double) * np * np);
}
int64_t Fragment::resident_bytes() const {
  int64_t words = eri_s4_.n + df_factor_.n + C_.n + eps_.n + dm_.n + J_.n + K_.n + t_prev_.n + z_prev_.n + sci_V_.keys.n + sci_V_.c.n;
  return 8 * words;
}
int Fragment::adopt_df_factor(DBuf&& B, int naux) {
  if (naux <= 0 || !B.p || B.n != (int64_t)naux * npair(n_)) { set_error("adopt_df_factor: factor of the wrong size"); return QEMB_ERR_ARG; }
  // beside a resident block the factor is only read while its route is the cheaper one (or forced): a large auxiliary set with the route left to the cost
  // rule would keep 8 naux npair bytes that nothing reads (~1 GB per n = 220 fragment at naux = 5000) -- not kept
  if (eri_s4_.p && mo_route_ == -1 && !mo_factor_route_pays(n_, naux)) { B.release(); clear_df_factor(); return 0; }
  df_factor_ = std::move(B); df_naux_ = naux;
  return 0;
}
int Fragment::set_mo_route(int route) {
  if (route < -1 || route > 1) { set_error("set_mo_route: -1 (by cost), 0 (four-index transformation) or 1 (3-index factor)"); return QEMB_ERR_ARG; }
  mo_route_ = route;
  return 0;
}
bool Fragment::use_factor_route() const {
  if (!df_factor_.p || mo_route_ == 0) return false;
  if (!eri_s4_.p) return true;      // a fragment that lives on its factor: forming the block first would cost what the factor's own product costs
  return mo_route_ == 1 || mo_factor_route_pays(n_, df_naux_);
}
// the half-unpacked tensor [P(p,q)][r][s] before the SCF, when something reads it: it is the first operand of the four-index
// transformation (and the exchange operand beyond n = 1024); the factor route needs neither
int Fragment::scf_operand(DBuf& X1, bool* unpacked) {
  *unpacked = false;
  if (mo_route_ == 1 && !df_factor_.p) { set_error("Fragment: the factor route was requested (set_mo_route 1) and no 3-index factor is set"); return QEMB_ERR_ARG; }
  if (use_factor_route() && (n_ <= 1024 || !eri_s4_.p)) return 0;
  if (!eri_s4_.p) QTRY(materialize_s4(s4_transient_));      // factor-only fragment with the four-index route forced (A/B runs): the block lives for this solve
  QTRY(X1.alloc(mo_transform_work(n_)));
  QTRY(dev_unpack_tril_rows_ld(npair(n_), n_, mo_slab_ld(n_), s4_ptr(), X1));      // rows mo_slab_ld(n) apart (ccsd.cpp)
  *unpacked = true;
  return 0;
}
int Fragment::mo_integrals(int o, int nf, DBuf& X1, bool x1_unpacked, MoIntegrals& ints, bool build_Vl, bool build_T34) {
  DBuf X0;
  QTRY(X0.alloc(mo_transform_work(n_)));
  if (!X1.p) { QTRY(X1.alloc(mo_transform_work(n_))); x1_unpacked = false; }
  last_route_factor_ = use_factor_route();
  if (last_route_factor_) return mo_transform_factor(n_, o, nf, df_naux_, df_factor_, X0, X1, C_, ints, build_Vl, build_T34);
  const int rc = mo_transform(n_, o, nf, s4_ptr(), X0, X1, C_, ints, build_Vl, build_T34, x1_unpacked);
  s4_transient_.release();
  return rc;
}
void Fragment::set_energy_data(const double* h1, const double* veff0, const double* veff, double weight, const int* centers, int ncen) {
  const size_t n2 = (size_t)n_ * n_;
  if (h1) h1_.assign(h1, h1 + n2);
  if (veff0) veff0_.assign(veff0, veff0 + n2);
  if (veff) veff_.assign(veff, veff + n2);
  weight_ = weight;
  centers_.assign(centers, centers + ncen);
}

int Fragment::run_scf(int o, const double* h, const double* dm0, const ScfOptions& opt, double* X0, ScfResult* sres, bool warm) {
  const int64_t n2 = (int64_t)n_ * n_;
  o_ = o;
  forget_solve();      // C_ / eps_ are about to change: rdm2() belongs to the solve that sets last_kind_ after this SCF
  // The orbitals of this fragment's previous solve (any sweep) serve as the basis in which the Jacobi eigensolver starts: the Fock
  // matrix of the new sweep is nearly diagonal there (heff moves by a matching step), so the first diagonalisation needs two sweeps
  // instead of eight.  Only the eigensolver's starting point changes -- the SCF still starts from dm0 -- so this does not depend on
  // `warm` (which is about reusing amplitudes, i.e. results).
  (void)warm;
  const bool c_guess = have_C_ && C_.p && dm0 && o == c_nocc_;
  if (!c_guess) { have_C_ = false; QTRY(C_.alloc(n2)); }
  QTRY(eps_.alloc(n_)); QTRY(dm_.alloc(n2)); QTRY(J_.alloc(n2)); QTRY(K_.alloc(n2));
  DBuf hd;
  QTRY(hd.alloc(n2));
  QTRY(dev_h2d_async(hd, h, sizeof(double) * n2));        // (consumed on this context's stream)
  if (dm0) {
    QTRY(dev_h2d_async(dm_, dm0, sizeof(double) * n2));
  } else {   // core guess
    DBuf tmp; QTRY(tmp.alloc(n2)); QTRY(dcopy(n2, hd, tmp));
    QTRY(dev_jacobi_eigh(n_, tmp, eps_, C_, nullptr));
    QTRY(gemm(n_, n_, o, 2.0, C_, n_, true, C_, n_, true, 0.0, dm_, n_));
  }
  JkSource src;
  DBuf Bfull;
  if (s4_ptr()) { src.eri_s1 = X0; src.eri_s4 = s4_ptr(); }
  else {        // the fragment lives on its factor: J / K from B (scf.cpp build_jk_factor)
    QTRY(Bfull.alloc((int64_t)df_naux_ * n2));
    QTRY(unpack_df_factor(n_, df_naux_, df_factor_, Bfull));
    src.Bp = df_factor_; src.Bfull = Bfull; src.naux = df_naux_;
  }
  const int rc = rhf_device_from(n_, o, hd, src, dm_, opt, C_, eps_, J_, K_, sres, c_guess);
  have_C_ = (rc == 0 && sres->converged);
  c_nocc_ = o;
  return rc;
}

int Fragment::hf_veff_from_dm(const double* P_host, double* J_host, double* K_host) {
  if (!has_eris()) { set_error("Fragment: ERIs not set"); return QEMB_ERR_ARG; }
  const int64_t n2 = (int64_t)n_ * n_;
  DBuf X0, P, J, K;
  QTRY(P.alloc(n2)); QTRY(J.alloc(n2)); QTRY(K.alloc(n2));
  QTRY(dev_h2d(P, P_host, sizeof(double) * n2));
  if (factor_only()) {
    QTRY(X0.alloc((int64_t)df_naux_ * n2));
    QTRY(unpack_df_factor(n_, df_naux_, df_factor_, X0));
    QTRY(build_jk_factor(n_, df_naux_, df_factor_, X0, P, nullptr, 0, J, K));
  } else {
    if (n_ > 1024) {      // (up to n = 1024 J and K come from the packed block in one pass: no half-unpacked tensor is needed)
      QTRY(X0.alloc(mo_transform_work(n_)));
      QTRY(dev_unpack_tril_rows(npair(n_), n_, eri_s4_, X0));
    }
    QTRY(build_jk(n_, X0, P, J, K, eri_s4_));
  }
  QTRY(dev_d2h(J_host, J, sizeof(double) * n2));
  QTRY(dev_d2h(K_host, K, sizeof(double) * n2));
  return 0;
}

int Fragment::scf_only(int o, const double* h, const double* dm0, const ScfOptions& opt, double* mo_coeff, double* mo_energy,
                       double* J_host, double* K_host, ScfResult* sres) {
  if (!has_eris()) { set_error("Fragment: ERIs not set"); return QEMB_ERR_ARG; }
  if (o <= 0 || o > n_) { set_error("Fragment: need 0 < nsocc <= n"); return QEMB_ERR_ARG; }
  const int64_t n2 = (int64_t)n_ * n_;
  DBuf X0;
  if (n_ > 1024 && eri_s4_.p) {      // (up to n = 1024 J and K come from the packed block in one pass: no half-unpacked tensor is needed)
    QTRY(X0.alloc(mo_transform_work(n_)));
    QTRY(dev_unpack_tril_rows(npair(n_), n_, eri_s4_, X0));     // half-unpacked [P(p,q)][r][s]
  }
  QTRY(run_scf(o, h, dm0, opt, X0, sres));
  if (mo_coeff) QTRY(dev_d2h(mo_coeff, C_, sizeof(double) * n2));
  if (mo_energy) QTRY(dev_d2h(mo_energy, eps_, sizeof(double) * n_));
  if (J_host) QTRY(dev_d2h(J_host, J_, sizeof(double) * n2));
  if (K_host) QTRY(dev_d2h(K_host, K_, sizeof(double) * n2));
  return 0;
}

// Coupled-perturbed HF (shared/external/cphf_utils.py:12-81, used by the HF Jacobian of the QN optimiser,
// shared/external/optqn.py:456-466):  A = 4 (ia|jb) - (ib|ja) - (ij|ab) - diag(e_i - e_a)  (:27-32),
// B0_p = Co^T v_p Cv (:37-41), u_p = A^-1 B0_p (:70), dP_p = -(Co u_p Cv^T + transpose) (:75-81).
// A is the (positive definite) RHF orbital Hessian, so the solve is Cholesky + triangular inverse + two GEMMs.
int Fragment::cphf_response(int o, const double* h, const double* dm0, const ScfOptions& opt, const double* vpots, int npot,
                            double* dPs) {
  if (!has_eris()) { set_error("Fragment: ERIs not set"); return QEMB_ERR_ARG; }
  if (o <= 0 || o >= n_ || npot <= 0) { set_error("cphf_response: bad arguments"); return QEMB_ERR_ARG; }
  const int n = n_, v = n - o;
  const int64_t n2 = (int64_t)n * n, nov = (int64_t)o * v;
  DBuf X1;
  bool x1_unpacked = false;
  QTRY(scf_operand(X1, &x1_unpacked));
  ScfResult sres;
  QTRY(run_scf(o, h, dm0, opt, X1, &sres));
  if (!sres.converged) { set_error("cphf_response: fragment SCF did not converge"); return QEMB_ERR_NOCONV; }
  std::vector<double> C((size_t)n2), eps((size_t)n);
  QTRY(dev_d2h(C.data(), C_, sizeof(double) * n2));
  QTRY(dev_d2h(eps.data(), eps_, sizeof(double) * n));
  MoIntegrals ints;
  QTRY(mo_integrals(o, 0, X1, x1_unpacked, ints, false, false));
  X1.release();
  DBuf A, L, Linv, d;
  QTRY(A.alloc(nov * nov)); QTRY(d.alloc(nov));
  QTRY(dcopy(nov * nov, ints.ovov, A));
  QTRY(axpby(nov * nov, 0.0, A, 4.0, A));                                              // 4 (ia|jb)
  QTRY(perm4(A, ints.ovov, o, v, o, v, 0, 3, 2, 1, -1.0, 1.0));                         // - (ib|ja)
  QTRY(perm4(A, ints.oovv, o, o, v, v, 0, 2, 1, 3, -1.0, 1.0));                         // - (ij|ab)
  std::vector<double> den((size_t)nov);
  for (int i = 0; i < o; ++i) for (int a = 0; a < v; ++a) den[(size_t)i * v + a] = eps[(size_t)o + a] - eps[(size_t)i];
  QTRY(dev_h2d(d, den.data(), sizeof(double) * nov));
  {
    Copy4Desc c{};
    c.dim[0] = 1; c.dim[1] = 1; c.dim[2] = 1; c.dim[3] = nov;
    c.in = d; c.si[3] = 1; c.out = A; c.so[3] = nov + 1; c.alpha = 1.0; c.beta = 1.0;
    QTRY(dev_copy4(c));                                                               // - diag(e_i - e_a)
  }
  ints = MoIntegrals();
  QTRY(dev_cholesky_lower(nov, A));
  QTRY(Linv.alloc(nov * nov));
  QTRY(dev_tri_inverse_lower(nov, A, Linv));
  A.release();
  // right-hand sides B0[(ia), p]
  std::vector<double> B0((size_t)nov * npot), tmp((size_t)o * n);
  for (int p = 0; p < npot; ++p) {
    const double* vp = vpots + (size_t)p * n2;
    for (int i = 0; i < o; ++i) for (int q = 0; q < n; ++q) { double s = 0; for (int r = 0; r < n; ++r) s += C[(size_t)r * n + i] * vp[(size_t)r * n + q]; tmp[(size_t)i * n + q] = s; }
    for (int i = 0; i < o; ++i) for (int a = 0; a < v; ++a) { double s = 0; for (int q = 0; q < n; ++q) s += tmp[(size_t)i * n + q] * C[(size_t)q * n + o + a]; B0[((size_t)i * v + a) * npot + p] = s; }
  }
  DBuf dB, dY, dU;
  QTRY(dB.alloc(nov * npot)); QTRY(dY.alloc(nov * npot)); QTRY(dU.alloc(nov * npot));
  QTRY(dev_h2d(dB, B0.data(), sizeof(double) * nov * npot));
  QTRY(gemm_nn(nov, npot, nov, 1.0, Linv, dB, 0.0, dY));                                // y = L^-1 B0
  QTRY(gemm_tn(nov, npot, nov, 1.0, Linv, dY, 0.0, dU));                                // u = L^-T y
  std::vector<double> U((size_t)nov * npot);
  QTRY(dev_d2h(U.data(), dU, sizeof(double) * nov * npot));
  std::vector<double> X((size_t)n * v);
  for (int p = 0; p < npot; ++p) {
    double* dP = dPs + (size_t)p * n2;
    for (int r = 0; r < n; ++r) for (int a = 0; a < v; ++a) { double s = 0; for (int i = 0; i < o; ++i) s += C[(size_t)r * n + i] * U[((size_t)i * v + a) * npot + p]; X[(size_t)r * v + a] = s; }
    for (int r = 0; r < n; ++r) for (int q = 0; q < n; ++q) { double s = 0; for (int a = 0; a < v; ++a) s += X[(size_t)r * v + a] * C[(size_t)q * n + o + a]; dP[(size_t)r * n + q] = -s; }
    for (int r = 0; r < n; ++r) for (int q = 0; q < r; ++q) { const double t = dP[(size_t)r * n + q] + dP[(size_t)q * n + r]; dP[(size_t)r * n + q] = dP[(size_t)q * n + r] = t; }
    for (int r = 0; r < n; ++r) dP[(size_t)r * n + r] *= 2.0;
  }
  return 0;
}

int Fragment::prepare_ccsd(int o, const double* h, const double* dm0, const FragmentOptions& opt) {
  if (!has_eris()) { set_error("Fragment: ERIs not set"); return QEMB_ERR_ARG; }
  if (o <= 0 || o >= n_) { set_error("Fragment: need 0 < nsocc < n"); return QEMB_ERR_ARG; }
  retire_solver();
  DBuf X1;
  bool x1_unpacked = false;
  QTRY(scf_operand(X1, &x1_unpacked));
  ScfResult sres;
  QTRY(run_scf(o, h, dm0, opt.scf, X1, &sres));
  if (!sres.converged) { set_error("fragment SCF did not converge (also not with level shift 0.2)"); return QEMB_ERR_NOCONV; }
  MoIntegrals ints;
  QTRY(mo_integrals(o, nf_, X1, x1_unpacked, ints, /*build_Vl=*/true, false));   // measurement hook: dense block available for export
  X1.release();
  cc_.reset(new CcsdSolver());
  QTRY(cc_->setup(std::move(ints), eps_));
  return cc_->init_amps();
}
int Fragment::ccsd_reset() { if (!cc_) { set_error("Fragment: prepare_ccsd first"); return QEMB_ERR_ARG; } return cc_->init_amps(); }
int Fragment::ccsd_iterate(int niter, double* e_corr, double* normt) {
  if (!cc_) { set_error("Fragment: prepare_ccsd first"); return QEMB_ERR_ARG; }
  for (int i = 0; i < niter; ++i) QTRY(cc_->iterate(e_corr, normt));
  return 0;
}

int Fragment::solve(int o, const double* h, const double* dm0, const FragmentOptions& opt, int eeval, FragmentResult* res,
                    double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* t1_out, double* t2_out) {
  QTRY(solve_begin(o, h, dm0, opt, eeval, res));
  if (!sp_.no_virtuals) {
    bool conv = false;
    QTRY(cc_->kernel(opt.cc, &res->e_corr_mo, &res->n_iter, &conv));
    res->ccsd_converged = conv;
  }
  return solve_end(mo_coeff, mo_energy, rdm1_emb, rdm1_mo, t1_out, t2_out);
}

// Several fragments in one call: the phases around the CCSD iterations (fragment RHF + MO transformation + set-up; amplitudes -> 1-RDM ->
// energies) run per fragment on one host thread and execution context each, as solver.map_fragments does; the CCSD iterations of all
// fragments run in LOCK STEP on the calling thread (ccsd_kernel_lockstep: one grouped launch per operation for all fragments).
// The per-fragment phases of a batched sweep run on PERSISTENT host threads (round 5): worker f serves fragment f of every phase of every sweep.  Starting six
// std::threads three times per sweep cost ~0.1 ms per phase on the sweep's critical path (the last thread starts ~100 us after the first) -- 0.3 ms of an octane BE2
// sweep of 14 ms.  The pool is never destroyed (its threads sleep on a condition variable; a fork()ed child makes its own); a second caller that finds it busy starts
// plain threads as before.
namespace {
class PhasePool {
 public:
  static PhasePool* acquire(int F) {
    static std::mutex guard;
    static PhasePool* pool = nullptr;
    std::lock_guard<std::mutex> lk(guard);
    if (!pool || pool->pid_ != getpid()) pool = new PhasePool();      // (first use, or the child of a fork: the parent's workers do not exist here)
    if (!pool->busy_.try_lock()) return nullptr;
    pool->grow(F);
    return pool;
  }
  void release() { busy_.unlock(); }
  // fn(f) for f in [0, F) on workers 0 .. F-1; returns when every call has returned
  void run(int F, const std::function<void(int)>& fn) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      fn_ = &fn; active_ = F; pending_ = F; ++gen_;
    }
    cv_work_.notify_all();
    std::unique_lock<std::mutex> lk(mu_);
    cv_done_.wait(lk, [&] { return pending_ == 0; });
    fn_ = nullptr;
  }
 private:
  PhasePool() : pid_(getpid()) {}
  void grow(int F) {
    while ((int)nworkers_ < F) {
      const int id = nworkers_++;
      std::thread([this, id] { loop(id); }).detach();
    }
  }
  void loop(int id) {
    unsigned long long seen = 0;
    for (;;) {
      const std::function<void(int)>* fn = nullptr;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_work_.wait(lk, [&] { return gen_ != seen; });
        seen = gen_;
        if (id < active_) fn = fn_;
      }
      if (!fn) continue;
      (*fn)(id);
      bool last;
      { std::lock_guard<std::mutex> lk(mu_); last = (--pending_ == 0); }
      if (last) cv_done_.notify_one();
    }
  }
  pid_t pid_;
  std::mutex busy_, mu_;
  std::condition_variable cv_work_, cv_done_;
  const std::function<void(int)>* fn_ = nullptr;
  int active_ = 0, pending_ = 0, nworkers_ = 0;
  unsigned long long gen_ = 0;
};
// A batched call: its execution contexts, whether the fragments run side by side, the worker pool and the per-fragment statuses.  per_fragment(fn) runs fn(f) for
// every fragment -- each on the worker thread of fragment f bound to execution context f + 1 (threaded), or one after the other -- and folds what they return:
// the first failure (in fragment order) is the call's status and error text, else the last warning
struct Fanout {
  int F; bool threaded = false; PhasePool* pool = nullptr; std::vector<int> rc; std::vector<std::string> msg;
  explicit Fanout(int F_) : F(F_), rc(F_, 0), msg(F_) {}
  ~Fanout() { if (pool) pool->release(); }
  int init() {
    const int have = dev_ctx_count(F + 1);
    if (have < 0) return have;
    // a backend with a single execution context (the scalar mock of tests/hostcheck) runs the per-fragment phases one after the other
    threaded = have >= F + 1 && F > 1;
    if (threaded) pool = PhasePool::acquire(F);      // (busy with another caller's batch: none, a std::thread per fragment and phase)
    return 0;
  }
  template <class Fn> int operator()(Fn fn) {
    if (threaded) {
      auto body = [&](int f) {
        rc[f] = dev_ctx_bind(f + 1);
        if (rc[f] == 0) rc[f] = fn(f);
        if (rc[f] != 0) msg[f] = last_error();
      };
      if (pool) pool->run(F, body);
      else {
        std::vector<std::thread> th;
        for (int f = 0; f < F; ++f) th.emplace_back([&, f] { body(f); });
        for (auto& t : th) t.join();
      }
    } else {
      for (int f = 0; f < F; ++f) { rc[f] = fn(f); if (rc[f] != 0) msg[f] = last_error(); }
    }
    int status = 0;
    for (int f = 0; f < F; ++f) if (rc[f] < 0) { set_error("fragment " + std::to_string(f) + ": " + msg[f]); return rc[f]; }
    for (int f = 0; f < F; ++f) if (rc[f] > 0) { status = rc[f]; set_error("fragment " + std::to_string(f) + ": " + msg[f]); }
    return status;
  }
};
}  // namespace

int Fragment::solve_batch(const std::vector<Fragment*>& frs, const std::vector<int>& o, const std::vector<const double*>& h,
                          const std::vector<const double*>& dm0, const FragmentOptions& opt, int eeval, std::vector<FragmentResult>& res,
                          const std::vector<BatchOutputs>& outs, LockstepStats* stats) {
  const int F = (int)frs.size();
  if (F == 0) return 0;
  static const bool trace = env_flag("QEMB_BATCH_TRACE", false);
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_start = now();
  res.assign(F, FragmentResult());
  Fanout per_fragment(F);
  QTRY(per_fragment.init());
  const bool threaded = per_fragment.threaded;
  // Before the iterations: the fragment RHF per fragment (host round trips inside), then MO integrals + CCSD set-up + starting amplitudes, each fragment on its own
  // stream.  (One pass of the host threads for both halves of the begin phase: a fragment goes on to its integrals as soon as ITS RHF is through instead of
  //  waiting for the slowest RHF of the sweep.)
  std::vector<double> ms_scf(F, 0.0);
  std::vector<double> ms_cc(F, 0.0), ms_capture(F, 0.0);      // (trace: the slowest fragment's share of the second half of the begin phase)
  QTRY(per_fragment([&](int f) {
    const double ts = now();
    int r = frs[f]->solve_begin_scf(o[f], h[f], dm0[f], opt, eeval, &res[f]);
    ms_scf[f] = now() - ts;
    if (r != 0) return r;
    const double t0 = now();
    r = frs[f]->solve_begin_cc();
    const double t1 = now();
    if (r == 0 && frs[f]->cc_ && F > 1) r = frs[f]->tape_for_lockstep(F);      // recorded side by side (or kept from the last sweep); a lone fragment keeps its executable graph
    const double t2 = now();
    if (r == 0) r = dev_sync();                                               // the lock-step loop reads this fragment's buffers from another stream
    ms_cc[f] = (t1 - t0) + (now() - t2); ms_capture[f] = t2 - t1;
    return r;
  }));
  const double t_begin_done = now();
  std::vector<CcsdSolver*> solvers; std::vector<int> idx, ctx; std::vector<CcsdOptions> copt;
  for (int f = 0; f < F; ++f) if (!frs[f]->sp_.no_virtuals) { solvers.push_back(frs[f]->cc_.get()); idx.push_back(f); ctx.push_back(threaded ? f + 1 : 0); copt.push_back(opt.cc); }
  if (!solvers.empty()) {
    std::vector<double> e; std::vector<int> nit; std::vector<char> conv;
    QTRY(ccsd_kernel_lockstep(solvers, copt, ctx, 0, e, nit, conv, stats));
    for (size_t k = 0; k < idx.size(); ++k) { res[idx[k]].e_corr_mo = e[k]; res[idx[k]].n_iter = nit[k]; res[idx[k]].ccsd_converged = conv[k] != 0; }
  }
  const double t_lock_done = now();
  const int rc = per_fragment([&](int f) { return frs[f]->solve_end(outs[f].mo_coeff, outs[f].mo_energy, outs[f].rdm1_emb, outs[f].rdm1_mo, outs[f].t1, outs[f].t2); });
  if (trace) std::fprintf(stderr, "[qemb batch] %d fragments: begin %.2f ms (RHF <= %.2f, integrals + set-up <= %.2f, recording <= %.2f), lock-step iterations %.2f ms (tapes %.2f, post %.2f), end %.2f ms\n", F,
                          t_begin_done - t_start, *std::max_element(ms_scf.begin(), ms_scf.end()), *std::max_element(ms_cc.begin(), ms_cc.end()), *std::max_element(ms_capture.begin(), ms_capture.end()),
                          t_lock_done - t_begin_done, stats ? stats->ms_tapes : 0.0, stats ? stats->ms_post : 0.0, now() - t_lock_done);
  return rc;
}

int Fragment::solve_begin(int o, const double* h, const double* dm0, const FragmentOptions& opt, int eeval, FragmentResult* res) {
  QTRY(solve_begin_scf(o, h, dm0, opt, eeval, res));
  return solve_begin_cc();
}
// every solver refuses an energy evaluation without the static data before its fragment RHF
int Fragment::check_energy_data(int eeval) const {
  if (eeval && (h1_.empty() || veff0_.empty())) { set_error("Fragment: set_energy_data(h1, veff0, ...) before an energy evaluation"); return QEMB_ERR_ARG; }
  return 0;
}
// what a solver reports when it has no correlated step to run (no virtual orbitals), and until its own step fills them in
static void mean_field_result(FragmentResult* res) { res->e_corr_mo = 0.0; res->n_iter = 0; res->ccsd_converged = true; res->lambda_iters = 0; }
int Fragment::solve_begin_scf(int o, const double* h, const double* dm0, const FragmentOptions& opt, int eeval, FragmentResult* res) {
  sp_ = SolvePending();
  sp_.o = o; sp_.opt = opt; sp_.eeval = eeval; sp_.res = res;
  last_route_factor_ = false;
  if (!has_eris()) { set_error("Fragment: ERIs not set"); return QEMB_ERR_ARG; }
  if (o <= 0 || o > n_) { set_error("Fragment: need 0 < nsocc <= n"); return QEMB_ERR_ARG; }
  QTRY(check_energy_data(eeval));
  const int n = n_, v = n - o;
  // nsocc == n: an embedding space without virtual orbitals.  PySCF's CCSD then has empty amplitude arrays and returns E_corr = 0; the
  // sweep body needs the mean-field results only (density = 2 I in any orthonormal basis, no correlation contribution to the energies).
  const int64_t n2 = (int64_t)n * n;
  static const bool trace = env_flag("QEMB_SCF_TRACE", false);      // host time of the steps of this phase on stderr (a measuring aid)
  auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = trace ? now() : 0.0;
  retire_solver();
  const double t1 = trace ? now() : 0.0;
  // ---- fragment RHF on the half-unpacked tensor [P(p,q)][r][s] (kept: it is the first operand of the MO transformation)
  QTRY(scf_operand(sp_.X1, &sp_.x1_unpacked));         // [P(p,q)][r][s] for the four-index route (kept: its first operand); nothing on the factor route
  const double t2 = trace ? now() : 0.0;
  ScfResult sres;
  QTRY(run_scf(o, h, dm0, opt.scf, sp_.X1, &sres, opt.warm_start != 0));
  if (trace) std::fprintf(stderr, "[qemb scf trace] n=%d retire %.0f us, operand %.0f us, run_scf %.0f us (%d cycles)\n", n, t1 - t0, t2 - t1, now() - t2, sres.cycles);
  res->scf_converged = sres.converged; res->scf_cycles = sres.cycles; res->e_scf = sres.e_tot;
  sp_.no_virtuals = (v == 0);
  if (!sres.converged) {
    set_error("fragment SCF did not converge (also not with level shift 0.2)");
    if (opt.strict) return QEMB_ERR_NOCONV;
    sp_.unconverged = true;
  }
  sp_.C.assign((size_t)n2, 0.0); sp_.eps.assign((size_t)n, 0.0);
  QTRY(dev_d2h(sp_.C.data(), C_, sizeof(double) * n2));
  QTRY(dev_d2h(sp_.eps.data(), eps_, sizeof(double) * n));
  return 0;
}
// ---- integrals + CCSD set-up + starting amplitudes: launches only (allocations come from the context's pool once a sweep has run)
int Fragment::solve_begin_cc() {
  const int o = sp_.o, v = n_ - o;
  const FragmentOptions& opt = sp_.opt;
  FragmentResult* res = sp_.res;
  if (sp_.no_virtuals) {
    sp_.X1.release();
    mean_field_result(res);
    return 0;
  }
  dev_alloc_trace_begin();
  MoIntegrals ints;
  QTRY(mo_integrals(o, sp_.eeval ? nf_ : 0, sp_.X1, sp_.x1_unpacked, ints, /*build_Vl=*/false, /*build_T34=*/opt.relax_density != 0));
  sp_.X1.release();
  retire_solver();
  cc_.reset(new CcsdSolver());
  QTRY(cc_->setup(std::move(ints), eps_));
  if (opt.warm_start && t_prev_.p && t_prev_o_ == o) {
    QTRY(cc_->set_amps(t_prev_.p, t_prev_.p + (int64_t)o * v));
  } else {
    QTRY(cc_->init_amps());
  }
  sp_.alloc_hash = dev_alloc_trace_end();
  return 0;
}

// The recorded update of a lock-step sweep.  Recording costs a stream capture and ~50 node queries per fragment and sweep (0.4-0.5 ms of the begin phase of an
// octane sweep, the six host threads queueing on the runtime's capture lock), and a new tape means a new merge plan in dev_tape_run.  The tape only names
// buffers and sizes: when this solve's allocations landed where the last solve's did (the pool hands blocks back in the order they came -- sp_.alloc_hash), the
// last tape IS this solve's tape.  QEMB_TAPE_CACHE_CHECK=1: record anyway and compare with the kept tape (tests).
static std::atomic<long long> g_tape_reused{0}, g_tape_recorded{0};
void tape_cache_counters(long long* reused, long long* recorded, int reset) {
  if (reused) *reused = g_tape_reused.load();
  if (recorded) *recorded = g_tape_recorded.load();
  if (reset) { g_tape_reused = 0; g_tape_recorded = 0; }
}
// (peers: the fragment count of the sweep; it only enters the key)
int Fragment::tape_for_lockstep(int peers) {
  const bool check = env_flag("QEMB_TAPE_CACHE_CHECK", false);
  unsigned long long key = sp_.alloc_hash ^ (0x9e3779b97f4a7c15ull * (unsigned long long)(peers + 1)) ^ ((unsigned long long)sp_.o << 40) ^ ((unsigned long long)n_ << 20);
  if (key == 0) key = 1;
  tape_key_ = key;
  if (env_flag("QEMB_TAPE_CACHE_TRACE", false)) std::fprintf(stderr, "[qemb tape cache] fragment %p n %d: key %016llx, kept %016llx\n", (void*)this, n_, key, tape_cache_.tape ? tape_cache_.key : 0ull);
  if (tape_cache_.tape && tape_cache_.key == key) {
    if (check) {
      QTRY(cc_->prepare_tape());
      if (cc_->tape() && !dev_tape_equal(cc_->tape(), tape_cache_.tape)) { set_error(std::string("the kept tape differs from a fresh recording at the same buffer layout: ") + last_error()); return QEMB_ERR_DEVICE; }
    }
    cc_->adopt_tape(tape_cache_.tape);
    tape_cache_.tape = nullptr;
    g_tape_reused += 1;
    return 0;
  }
  g_tape_recorded += 1;
  return cc_->prepare_tape();
}
void Fragment::retire_solver() {
  if (cc_) {
    dev_tape_t t = cc_->release_tape();
    if (t) {
      if (tape_key_ != 0) { if (tape_cache_.tape) (void)dev_tape_destroy(tape_cache_.tape); tape_cache_.tape = t; tape_cache_.key = tape_key_; }
      else (void)dev_tape_destroy(t);
    }
  }
  tape_key_ = 0;
  cc_.reset();
}

// ---- the tail every correlated solve of a fragment shares: the solver hands finish_solve its MO-basis 1-RDM and its per-site two-body energies
// hf_dm = Co Co^T
static std::vector<double> hf_density(int n, int o, const std::vector<double>& C) {
  std::vector<double> hfdm((size_t)n * n, 0.0);
  for (int p = 0; p < n; ++p) for (int q = 0; q < n; ++q) { double s = 0; for (int i = 0; i < o; ++i) s += C[(size_t)p * n + i] * C[(size_t)q * n + i]; hfdm[(size_t)p * n + q] = s; }
  return hfdm;
}
// The per-site two-body energies e2_P of get_frag_energy (helper.py:286-339), P < nf, from what each solver contracts on the device:
// Z1, Z2 (energy_intermediates of the CCSD or the MP2 solver): e2_P = 1/2 (sum_i C[P,i] Z1[i,P] + sum_a C[P,o+a] Z2[a,P])
static std::vector<double> e2_from_Z(int n, int o, int nf, const std::vector<double>& C, const std::vector<double>& Z1, const std::vector<double>& Z2) {
  std::vector<double> e2((size_t)nf, 0.0);
  for (int P = 0; P < nf; ++P) {
    double s2 = 0;
    for (int i = 0; i < o; ++i) s2 += C[(size_t)P * n + i] * Z1[(size_t)i * nf + P];
    for (int a = 0; a < n - o; ++a) s2 += C[(size_t)P * n + o + a] * Z2[(size_t)a * nf + P];
    e2[P] = 0.5 * s2;
  }
  return e2;
}
// Imat of the relaxed CCSD path: e2_P = 1/4 sum_p' C[P,p'] I[p',P]  (cc_lambda.h)
static std::vector<double> e2_from_Imat(int n, int nf, const std::vector<double>& C, const std::vector<double>& Imat) {
  std::vector<double> e2((size_t)nf, 0.0);
  for (int P = 0; P < nf; ++P) {
    double s2 = 0;
    for (int q = 0; q < n; ++q) s2 += C[(size_t)P * n + q] * Imat[(size_t)q * nf + P];
    e2[P] = 0.25 * s2;
  }
  return e2;
}

// get_frag_energy (helper.py:286-339) from the embedding-basis density and the per-site two-body energies, and update_ebe_hf
int Fragment::frag_energies(const std::vector<double>& rdm, const std::vector<double>& hfdm, const std::vector<double>& e2, FragmentResult* res) {
  const int n = n_;
  const int64_t n2 = (int64_t)n * n;
  std::vector<double> J((size_t)n2), K((size_t)n2);
  std::vector<double> e1((size_t)nf_, 0.0), ec((size_t)nf_, 0.0);
  for (int P = 0; P < nf_; ++P) {
    double s1 = 0, sc = 0;
    for (int Q = 0; Q < n; ++Q) {
      const double d = 2.0 * (rdm[(size_t)P * n + Q] - hfdm[(size_t)P * n + Q]);   // helper.py:286
      s1 += h1_[(size_t)P * n + Q] * d; sc += veff0_[(size_t)P * n + Q] * d;
    }
    e1[P] = s1; ec[P] = sc;
  }
  res->e_frag[0] = res->e_frag[1] = res->e_frag[2] = 0.0;
  for (int c : centers_) { res->e_frag[0] += weight_ * e1[c]; res->e_frag[1] += weight_ * e2[c]; res->e_frag[2] += weight_ * ec[c]; }
  // update_ebe_hf (pfrag.py:327-400) with D = Co Co^T: e2_i = sum_j D_ij (2 J_ij - K_ij), J/K of D = J,K(dm)/2
  if (!veff_.empty()) {
    QTRY(dev_d2h(J.data(), J_, sizeof(double) * n2));
    QTRY(dev_d2h(K.data(), K_, sizeof(double) * n2));
    double ehf = 0.0;
    for (int c : centers_) {
      double a = 0;
      for (int Q = 0; Q < n; ++Q) {
        const double D = hfdm[(size_t)c * n + Q];
        a += 2.0 * h1_[(size_t)c * n + Q] * D + veff_[(size_t)c * n + Q] * D + D * (J[(size_t)c * n + Q] - 0.5 * K[(size_t)c * n + Q]);
      }
      ehf += weight_ * a;
    }
    res->ebe_hf = ehf;
  }
  return 0;
}

// After a solver's correlated step: rdm_emb = C rdm1_mo C^T / 2 (solver.py:496-505), the outputs, the energies, and what rdm2() needs of this solve.
// dm is the solver's MO-basis 1-RDM (n x n, host); e2 its per-site two-body energies (read with eeval only).  The back-rotation has two forms:
//   t1 given (o x v, host; dm = [[2 I, t1], [t1^T, 0]]): Co Co^T + (Co t1 Cv^T + Cv t1^T Co^T)/2 on the host -- no device call in the end phase of a lock-step sweep;
//   otherwise: two products with the resident orbitals on the device, symmetrised on the host.
int Fragment::finish_solve(const std::vector<double>* t1, const std::vector<double>& dm, const std::vector<double>& e2, int kind, bool relaxed, bool unconverged,
                           double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo) {
  const int o = sp_.o, n = n_, v = n - o;
  const int64_t n2 = (int64_t)n * n;
  const std::vector<double>& C = sp_.C;
  const std::vector<double> hfdm = hf_density(n, o, C);
  std::vector<double> rdm((size_t)n2, 0.0);
  if (t1) {
    std::vector<double> X((size_t)n * v, 0.0);
    for (int p = 0; p < n; ++p) for (int a = 0; a < v; ++a) { double s = 0; for (int i = 0; i < o; ++i) s += C[(size_t)p * n + i] * (*t1)[(size_t)i * v + a]; X[(size_t)p * v + a] = s; }
    for (int p = 0; p < n; ++p) for (int q = 0; q < n; ++q) { double s = 0; for (int a = 0; a < v; ++a) s += X[(size_t)p * v + a] * C[(size_t)q * n + o + a]; rdm[(size_t)p * n + q] = s; }
    for (int p = 0; p < n; ++p) for (int q = 0; q <= p; ++q) {
      const double sym = 0.5 * (rdm[(size_t)p * n + q] + rdm[(size_t)q * n + p]);
      rdm[(size_t)p * n + q] = rdm[(size_t)q * n + p] = hfdm[(size_t)p * n + q] + sym;
    }
  } else if (v > 0) {
    DBuf D, T, R;
    QTRY(D.alloc(n2)); QTRY(T.alloc(n2)); QTRY(R.alloc(n2));
    QTRY(dev_h2d(D, dm.data(), sizeof(double) * n2));
    QTRY(gemm_nn(n, n, n, 1.0, C_, D, 0.0, T));
    QTRY(gemm_nt(n, n, n, 0.5, T, C_, 0.0, R));
    QTRY(dev_d2h(rdm.data(), R, sizeof(double) * n2));
    for (int p = 0; p < n; ++p) for (int q = 0; q < p; ++q) { const double sym = 0.5 * (rdm[(size_t)p * n + q] + rdm[(size_t)q * n + p]); rdm[(size_t)p * n + q] = rdm[(size_t)q * n + p] = sym; }
  } else rdm = hfdm;      // no virtual orbitals: dm = 2 I
  if (rdm1_mo) std::memcpy(rdm1_mo, dm.data(), sizeof(double) * n2);
  if (rdm1_emb) std::memcpy(rdm1_emb, rdm.data(), sizeof(double) * n2);
  if (mo_coeff) std::memcpy(mo_coeff, C.data(), sizeof(double) * n2);
  if (mo_energy) std::memcpy(mo_energy, sp_.eps.data(), sizeof(double) * n);
  if (sp_.eeval) QTRY(frag_energies(rdm, hfdm, e2, sp_.res));
  // the next sweep may drive this fragment from a host thread bound to ANOTHER execution context (stream): the kept amplitudes,
  // multipliers and orbitals must be complete before this call returns (no inter-stream ordering exists otherwise)
  QTRY(dev_sync());
  last_kind_ = kind; last_o_ = o; last_relaxed_ = relaxed;
  return unconverged ? QEMB_WARN_NOCONV : 0;
}

int Fragment::solve_end(double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* t1_out, double* t2_out) {
  const int o = sp_.o, n = n_, v = n - o, eeval = sp_.eeval;
  const FragmentOptions& opt = sp_.opt;
  FragmentResult* res = sp_.res;
  const bool no_virtuals = sp_.no_virtuals;
  bool unconverged = sp_.unconverged;
  const int64_t n2 = (int64_t)n * n;
  if (!no_virtuals && !res->ccsd_converged) {
    set_error("CCSD did not converge in max_cycle iterations");
    if (opt.strict) return QEMB_ERR_NOCONV;
    unconverged = true;
  }
  // ---- amplitudes to the host as requested
  std::vector<double> t1((size_t)o * v);
  if (!no_virtuals) QTRY(dev_d2h(t1.data(), cc_->t1(), sizeof(double) * o * v));
  if (t1_out && !t1.empty()) std::memcpy(t1_out, t1.data(), sizeof(double) * o * v);
  if (t2_out && !no_virtuals) QTRY(dev_d2h(t2_out, cc_->t2(), sizeof(double) * (int64_t)o * o * v * v));
  std::vector<double> dm((size_t)n2, 0.0), e2;
  if (opt.relax_density && no_virtuals) {
    for (int i = 0; i < n; ++i) dm[(size_t)i * n + i] = 2.0;
    if (eeval) e2.assign((size_t)nf_, 0.0);
  } else if (opt.relax_density) {
    // ---- Lambda equations, response 1-RDM and the contraction of the response 2-RDM with the fragment ERIs
    CcLambda lam(*cc_);
    QTRY(lam.setup());
    if (opt.warm_start && z_prev_.p && z_prev_o_ == o) QTRY(lam.set_guess(z_prev_));
    bool lconv = false;
    QTRY(lam.kernel(opt.lam, &res->lambda_iters, &lconv));
    if (!lconv) {
      set_error("CCSD Lambda equations did not converge in max_cycle iterations");
      if (opt.strict) return QEMB_ERR_NOCONV;
      unconverged = true;
    }
    std::vector<double> Imat;
    if (eeval) Imat.assign((size_t)n * nf_, 0.0);
    QTRY(lam.densities(dm.data(), eeval ? cc_->integrals().T34.p : nullptr, nf_, eeval ? Imat.data() : nullptr));
    if (eeval) e2 = e2_from_Imat(n, nf_, sp_.C, Imat);
    if (opt.keep_amplitudes || opt.warm_start) {
      QTRY(z_prev_.alloc(lam.n_amp()));
      QTRY(dcopy(lam.n_amp(), lam.z(), z_prev_));
      z_prev_o_ = o;
    }
  } else {
    // unrelaxed: rdm1_mo = [[2 I, t1], [t1^T, 0]]  (shared/external/ccsd_rdm.py:10-20)
    for (int i = 0; i < o; ++i) dm[(size_t)i * n + i] = 2.0;
    for (int i = 0; i < o; ++i) for (int a = 0; a < v; ++a) { dm[(size_t)i * n + o + a] = t1[(size_t)i * v + a]; dm[(size_t)(o + a) * n + i] = t1[(size_t)i * v + a]; }
    if (eeval) {
      std::vector<double> Z1((size_t)o * nf_, 0.0), Z2;
      if (!no_virtuals) QTRY(cc_->energy_intermediates(Z1, Z2));
      e2 = e2_from_Z(n, o, nf_, sp_.C, Z1, Z2);
    }
  }
  // ---- keep amplitudes for a warm start of the next sweep
  if ((opt.keep_amplitudes || opt.warm_start) && !no_virtuals) {
    const int64_t na = cc_->n_amp();
    QTRY(t_prev_.alloc(na));
    QTRY(dcopy(na, cc_->t1(), t_prev_));
    t_prev_o_ = o;
  }
  const int rc = finish_solve(opt.relax_density ? nullptr : &t1, dm, e2, QEMB_RDM2_CCSD, opt.relax_density != 0, unconverged, mo_coeff, mo_energy, rdm1_emb, rdm1_mo);
  retire_solver();
  return rc;
}

// ---- solver == "MP2": everything after the fragment RHF is a handful of products with the factor and one pass over o^2 v^2 (mp2.cpp)
int Fragment::solve_mp2(int o, const double* h, const double* dm0, const FragmentOptions& opt, int eeval, FragmentResult* res,
                        double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* t2_out) {
  QTRY(solve_begin_scf(o, h, dm0, opt, eeval, res));
  const int n = n_, v = n - o;
  mean_field_result(res);
  std::vector<double> doo((size_t)o * o, 0.0), dvv, Z1((size_t)o * nf_, 0.0), Z2;
  if (v > 0) {
    Mp2Solver mp;
    if (use_factor_route()) {
      sp_.X1.release();
      last_route_factor_ = true;
      QTRY(mp.run_factor(n, o, eeval ? nf_ : 0, df_naux_, df_factor_, C_, eps_));
    } else {      // the packed block: the four-index transformation, of which ovov, A1, A2 are read (DESIGN.md prices it)
      MoIntegrals ints;
      QTRY(mo_integrals(o, eeval ? nf_ : 0, sp_.X1, sp_.x1_unpacked, ints, false, false));
      sp_.X1.release();
      QTRY(mp.run_blocks(std::move(ints), eps_));
    }
    res->e_corr_mo = mp.e_corr();
    if (t2_out) QTRY(dev_d2h(t2_out, mp.t2(), sizeof(double) * (int64_t)o * o * v * v));
    QTRY(mp.rdm1_blocks(doo, dvv));
    if (eeval) QTRY(mp.energy_intermediates(Z1, Z2));
  } else sp_.X1.release();      // no virtual orbitals: the mean-field results, as the CCSD path
  // rdm1_mo = [[2 I + doo + doo^T, 0], [0, dvv + dvv^T]]   (PySCF mp2.make_rdm1); kept for rdm2(): an MP2 solve keeps no amplitudes to form it from
  // (written before finish_solve can fail: rdm2() reads it only once finish_solve has set last_kind_, which run_scf cleared through forget_solve())
  mp2_dm1_.assign((size_t)n * n, 0.0);
  for (int i = 0; i < o; ++i) for (int j = 0; j < o; ++j) mp2_dm1_[(size_t)i * n + j] = doo[(size_t)i * o + j] + doo[(size_t)j * o + i] + (i == j ? 2.0 : 0.0);
  for (int a = 0; a < v; ++a) for (int b = 0; b < v; ++b) mp2_dm1_[(size_t)(o + a) * n + o + b] = dvv[(size_t)a * v + b] + dvv[(size_t)b * v + a];
  const std::vector<double> e2 = eeval ? e2_from_Z(n, o, nf_, sp_.C, Z1, Z2) : std::vector<double>();
  return finish_solve(nullptr, mp2_dm1_, e2, QEMB_RDM2_MP2, false, sp_.unconverged, mo_coeff, mo_energy, rdm1_emb, rdm1_mo);
}

// ---- solver == "FCI-hip": the fragment RHF, then the exact ground state of the embedding Hamiltonian in the determinant basis (fci.cpp)
// (pq|rs) in the fragment-MO basis as an n^2 x n^2 matrix from whichever residency the fragment has: the packed block (or B^T B of a fragment that lives on its
// factor) unpacked to [n]^4 and multiplied from both sides with CC[(mu nu)][(pq)] = C[mu,p] C[nu,q] -- two products of n^2 x n^2 matrices (n <= 16)
int Fragment::fci_mo_integrals(const std::vector<double>& C, DBuf& Vao, DBuf& CC, DBuf& Vmo) {
  const int n = n_;
  const int64_t n2 = (int64_t)n * n;
  DBuf s4tmp, Tm;
  const double* s4 = s4_ptr();
  if (!s4) { QTRY(materialize_s4(s4tmp)); s4 = s4tmp; }
  QTRY(Vao.alloc(n2 * n2)); QTRY(CC.alloc(n2 * n2)); QTRY(Vmo.alloc(n2 * n2)); QTRY(Tm.alloc(n2 * n2));
  QTRY(dev_unpack_s4(n, s4, Vao));
  std::vector<double> cc((size_t)(n2 * n2));
  for (int mu = 0; mu < n; ++mu) for (int nu = 0; nu < n; ++nu) for (int p = 0; p < n; ++p) for (int q = 0; q < n; ++q)
    cc[(size_t)((mu * n + nu) * n2 + p * n + q)] = C[(size_t)mu * n + p] * C[(size_t)nu * n + q];
  QTRY(dev_h2d(CC, cc.data(), sizeof(double) * n2 * n2));
  QTRY(gemm_nn(n2, n2, n2, 1.0, Vao, CC, 0.0, Tm));
  QTRY(gemm_tn(n2, n2, n2, 1.0, CC, Tm, 0.0, Vmo));
  s4_transient_.release();
  return dev_sync();      // (Tm and a transient block go back to the pool on return)
}

// e2_P = 1/2 sum_qrs Gamma_emb[P,q,r,s] (Pq|rs), Gamma_emb = (C x C) Gamma (C x C)^T the cumulant in the embedding basis; rows P < n_f only
int Fragment::fci_e2_sites(const double* CC, const double* G2, const double* Vao, std::vector<double>& e2) {
  const int64_t n2 = (int64_t)n_ * n_, n3 = n2 * n_;
  DBuf Tm, Ge, ed;
  QTRY(Tm.alloc(n2 * n2)); QTRY(Ge.alloc(n2 * n2)); QTRY(ed.alloc(nf_));
  QTRY(gemm_nn(n2, n2, n2, 1.0, CC, G2, 0.0, Tm));
  QTRY(gemm_nt(n2, n2, n2, 1.0, Tm, CC, 0.0, Ge));
  for (int P = 0; P < nf_; ++P) QTRY(dev_dot(n3, Ge.p + P * n3, Vao + P * n3, ed.p + P));
  QTRY(dev_d2h(e2.data(), ed, sizeof(double) * nf_));
  for (double& e : e2) e *= 0.5;
  return 0;
}

// ---- shared by solve_fci and solve_sci
// h in the fragment-MO basis: C^T h C (h, C [n][n] on the host)
static std::vector<double> mo_one_body(int n, const std::vector<double>& C, const double* h) {
  const int64_t n2 = (int64_t)n * n;
  std::vector<double> hmo((size_t)n2, 0.0), tmp((size_t)n2, 0.0);
  for (int p = 0; p < n; ++p) for (int nu = 0; nu < n; ++nu) { double s = 0; for (int mu = 0; mu < n; ++mu) s += C[(size_t)mu * n + p] * h[(size_t)mu * n + nu]; tmp[(size_t)p * n + nu] = s; }
  for (int p = 0; p < n; ++p) for (int q = 0; q < n; ++q) { double s = 0; for (int nu = 0; nu < n; ++nu) s += tmp[(size_t)p * n + nu] * C[(size_t)nu * n + q]; hmo[(size_t)p * n + q] = s; }
  return hmo;
}
// the device bytes a guard compares with: what is free, or the fragment's limit where that is less (limit < 0: none)
static int device_room(int64_t limit, double* room) {
  size_t free_b = 0, total_b = 0;
  QTRY(dev_mem_info(&free_b, &total_b));
  *room = (double)free_b;
  if (limit >= 0 && (double)limit < *room) *room = (double)limit;
  return 0;
}
// a single determinant (nsocc == n): the mean-field density 2 I, as the other solvers
static void single_determinant_dm(int n, std::vector<double>& dm) { for (int i = 0; i < n; ++i) dm[(size_t)i * n + i] = 2.0; }

int Fragment::solve_fci(int o, const double* h, const double* dm0, const FragmentOptions& opt, const FciOptions& fopt, int eeval, FragmentResult* res,
                        double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* civec) {
  const int n = n_, v = n - o;
  const int64_t n2 = (int64_t)n * n;
  if (n > kFciMaxOrb) { set_error("Fragment::solve_fci: n = " + std::to_string(n) + " embedding orbitals; the determinant-space solver takes at most " + std::to_string(kFciMaxOrb)); return QEMB_ERR_UNSUPPORTED; }
  if (o <= 0 || o > n) { set_error("Fragment: need 0 < nsocc <= n"); return QEMB_ERR_ARG; }
  QTRY(check_energy_data(eeval));      // (solve_begin_scf has the check for every solver; here it also keeps its place before the guard)
  int64_t rows = 0;      // the slab height this solve runs with (0: unslabbed), settled by the guard
  {      // the guard: D, G, the Davidson vectors, the tables and the n^4 pieces against what is free (or the fragment's limit), before anything is allocated
    double room = 0.0;
    QTRY(device_room(fci_mem_limit_, &room));
    const int64_t ns = fci_string_count(n, o);
    const double need = (double)fci_bytes_slab(n, o, fopt.max_space, 0);
    if (v > 0 && fci_slab_ != 0 && !(fci_slab_ < 0 && need <= room)) {      // a slabbed solve: its own figure against the same room
      rows = fci_slab_ > 0 ? std::min(fci_slab_, ns) : fci_rows_that_fit(n, o, fopt.max_space, room);
      const int64_t r1 = rows > 0 ? rows : 1;
      const double need_s = (double)fci_bytes_slab(n, o, fopt.max_space, r1);
      if (need_s > room) {
        set_error("Fragment::solve_fci: n = " + std::to_string(n) + ", nsocc = " + std::to_string(o) + " gives N_det = " + std::to_string(ns * ns) + " determinants; with rows = " +
                  std::to_string(r1) + " alpha rows of D and G at a time (" + std::to_string(fci_slab_count(ns, r1)) + " slabs) the working set is " + std::to_string(need_s * 1e-9) +
                  " GB, more than the " + std::to_string(room * 1e-9) + " GB of device memory it may take");
        return QEMB_ERR_ALLOC;
      }
    } else if (v > 0 && need > room) {
      set_error("Fragment::solve_fci: n = " + std::to_string(n) + ", nsocc = " + std::to_string(o) + " gives N_det = " + std::to_string(ns * ns) + " determinants and a working set of " +
                std::to_string(need * 1e-9) + " GB, more than the " + std::to_string(room * 1e-9) + " GB of device memory it may take");
      return QEMB_ERR_ALLOC;
    }
  }
  QTRY(solve_begin_scf(o, h, dm0, opt, eeval, res));
  sp_.X1.release();
  const std::vector<double>& C = sp_.C;
  bool unconverged = sp_.unconverged;
  mean_field_result(res);
  fci_c_.release(); fci_residual_ = 0.0;
  fci_rows_used_ = rows; fci_nslab_used_ = fci_slab_count(fci_string_count(n, o), rows);
  std::vector<double> dm((size_t)n2, 0.0), e2((size_t)nf_, 0.0);
  if (v > 0) {
    const FciTables* T = nullptr;
    QTRY(fci_tables(n, o, &T));
    const int64_t N = T->ndet();
    DBuf Vao, CC, Vmo;
    QTRY(fci_mo_integrals(C, Vao, CC, Vmo));
    const std::vector<double> hmo = mo_one_body(n, C, h);
    QTRY(fci_c_.alloc(N));
    FciResult fr;
    QTRY(fci_davidson(*T, hmo.data(), Vmo, fopt, fci_c_, &fr, rows));
    res->n_iter = fr.n_iter; res->ccsd_converged = fr.converged; fci_residual_ = fr.residual;
    res->e_corr_mo = fr.e - res->e_scf;
    if (!fr.converged) {
      set_error("FCI: the Davidson iteration did not converge in max_cycle applications of H (residual " + std::to_string(fr.residual) + ")");
      if (opt.strict) { fci_c_.release(); return QEMB_ERR_NOCONV; }
      unconverged = true;
    }
    if (civec) QTRY(dev_d2h(civec, fci_c_, sizeof(double) * N));
    DBuf G2;
    if (eeval) QTRY(G2.alloc(n2 * n2));
    QTRY(fci_rdm12(*T, fci_c_, o, dm.data(), eeval ? G2.p : nullptr, rows));
    if (eeval && nf_ > 0) QTRY(fci_e2_sites(CC, G2, Vao, e2));
  } else {
    single_determinant_dm(n, dm);
    if (civec) civec[0] = 1.0;
  }
  return finish_solve(nullptr, dm, e2, QEMB_RDM2_FCI, false, unconverged, mo_coeff, mo_energy, rdm1_emb, rdm1_mo);
}

// ---- solver == "SCI-hip": the fragment RHF, then the heat-bath selection of sci.cpp on the integrals of solve_fci; front and tail share its helpers
int Fragment::solve_sci(int o, const double* h, const double* dm0, const FragmentOptions& opt, const SciOptions& sopt, int eeval, FragmentResult* res,
                        double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo) {
  const int n = n_, v = n - o;
  const int64_t n2 = (int64_t)n * n;
  char eps_txt[32];
  snprintf(eps_txt, sizeof eps_txt, "%.3g", sopt.eps_var);
  if (n > kSciMaxOrb) { set_error("Fragment::solve_sci: n = " + std::to_string(n) + " embedding orbitals; the selected CI takes at most " + std::to_string(kSciMaxOrb) + " (one 64-bit word per spin)"); return QEMB_ERR_UNSUPPORTED; }
  if (o <= 0 || o > n) { set_error("Fragment: need 0 < nsocc <= n"); return QEMB_ERR_ARG; }
  if (!(sopt.eps_var > 0.0)) { set_error("Fragment::solve_sci: eps_var must be positive"); return QEMB_ERR_ARG; }
  if (sopt.max_round < 1 || sopt.max_det < 1) { set_error("Fragment::solve_sci: need max_round >= 1 and max_det >= 1"); return QEMB_ERR_ARG; }
  QTRY(check_energy_data(eeval));
  int64_t room_left = -1;
  {      // the guard: what max_det fixes against what is free (or the fragment's limit), before anything is allocated; the CSR arrays get what is left
    double room = 0.0;
    QTRY(device_room(sci_mem_limit_, &room));
    const double need = (double)sci_bytes(n, o, sopt.max_det, sopt.max_space);
    if (v > 0 && need > room) {
      set_error("Fragment::solve_sci: n = " + std::to_string(n) + ", eps_var = " + eps_txt + ", max_det = " + std::to_string(sopt.max_det) + " give a working set of " +
                std::to_string((int64_t)need) + " bytes (" + std::to_string(need * 1e-9) + " GB) before the matrix, more than the " + std::to_string(room * 1e-9) + " GB of device memory it may take");
      return QEMB_ERR_ALLOC;
    }
    room_left = (int64_t)(room - need);
  }
  QTRY(solve_begin_scf(o, h, dm0, opt, eeval, res));
  sp_.X1.release();
  const std::vector<double>& C = sp_.C;
  bool unconverged = sp_.unconverged;
  mean_field_result(res);
  std::vector<double> dm((size_t)n2, 0.0), e2((size_t)nf_, 0.0);
  if (v > 0) {
    DBuf Vao, CC, Vmo;
    QTRY(fci_mo_integrals(C, Vao, CC, Vmo));
    const std::vector<double> hmo = mo_one_body(n, C, h);
    SciSpace V; SciMatrix H; SciResult sr;
    QTRY(sci_solve(n, o, hmo.data(), Vmo, sopt, room_left, V, H, &sr));
    res->n_iter = sr.n_apply; res->ccsd_converged = sr.converged && sr.diag_converged;
    res->e_corr_mo = sr.e - res->e_scf;
    if (!res->ccsd_converged) {
      char b[200];
      snprintf(b, sizeof b, "SCI (n = %d, eps_var = %s): %s (%lld determinants, energy %.10f, residual %.3g)", n, eps_txt,
               sr.converged ? "a diagonalisation did not converge in max_cycle applications of H" : "the selection was still adding determinants after max_round rounds",
               (long long)sr.ndet, sr.e, sr.residual);
      set_error(b);
      if (opt.strict) return QEMB_ERR_NOCONV;
      unconverged = true;
    }
    DBuf G2;
    if (eeval) QTRY(G2.alloc(n2 * n2));
    {
      const auto t0 = std::chrono::steady_clock::now();
      QTRY(sci_rdm12(n, V.k(), V.N, H.rp(), H.ci(), V.c, o, dm.data(), eeval ? G2.p : nullptr));
      sr.ms[SCI_T_RDM] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    if (eeval && nf_ > 0) QTRY(fci_e2_sites(CC, G2, Vao, e2));
    H = SciMatrix();      // the matrix goes: 12 bytes per stored element (GBs at 10^9) would stay with every fragment of a sweep; rdm2() forms the pattern again
    const int rc = finish_solve(nullptr, dm, e2, QEMB_RDM2_SCI, false, unconverged, mo_coeff, mo_energy, rdm1_emb, rdm1_mo);
    if (rc >= 0) { sci_V_ = std::move(V); sci_res_ = sr; sci_hmo_ = hmo; sci_C_ = C; }      // 24 bytes per determinant stay (run_scf dropped the last solve's through forget_solve)
    return rc;
  }
  single_determinant_dm(n, dm);
  const int rc = finish_solve(nullptr, dm, e2, QEMB_RDM2_SCI, false, unconverged, mo_coeff, mo_energy, rdm1_emb, rdm1_mo);
  if (rc >= 0) { sci_res_ = SciResult(); sci_res_.ndet = 1; sci_res_.nnz = 1; sci_res_.converged = true; sci_res_.e = res->e_scf; }
  return rc;
}
int Fragment::sci_dets(uint64_t* alpha, uint64_t* beta, double* c) const {
  if (last_kind_ != QEMB_RDM2_SCI) { set_error("Fragment::sci_dets: the last solve of this fragment was not an SCI solve"); return QEMB_ERR_ARG; }
  if (sci_V_.N == 0) {      // the single determinant of nsocc == n
    const uint64_t hf = last_o_ >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << last_o_) - 1);
    if (alpha) alpha[0] = hf;
    if (beta) beta[0] = hf;
    if (c) c[0] = 1.0;
    return 0;
  }
  const int64_t N = sci_V_.N;
  std::vector<uint64_t> k((size_t)(2 * N));
  QTRY(dev_d2h(k.data(), sci_V_.keys, sizeof(uint64_t) * 2 * N));
  for (int64_t i = 0; i < N; ++i) { if (alpha) alpha[i] = k[(size_t)(2 * i)]; if (beta) beta[i] = k[(size_t)(2 * i + 1)]; }
  if (c) QTRY(dev_d2h(c, sci_V_.c, sizeof(double) * N));
  return 0;
}

// ---- the second-order correction of the last SCI solve (sci.cpp: sci_pt2), on integrals formed again as rdm2() forms again what it needs
int64_t Fragment::sci_pt2_work_bytes(int n, int nsocc, int64_t ndet, int64_t max_ext) {
  const int64_t n2 = (int64_t)n * n;
  return sci_pt2_bytes(n, nsocc, ndet, max_ext) + 8 * (4 * n2 * n2 + n2);      // Vao, CC, Vmo and the intermediate of fci_mo_integrals; h
}
int Fragment::sci_pt2(double eps_pt, int64_t max_ext, double* e_pt2, int64_t* n_ext, int* batches, double* ms3) {
  double e = 0.0, ms[SCI_PT2_T_COUNT] = {0, 0, 0};
  int64_t next = 0;
  int nb = 0;
  auto hand_out = [&]() {
    if (e_pt2) *e_pt2 = e;
    if (n_ext) *n_ext = next;
    if (batches) *batches = nb;
    if (ms3) for (int k = 0; k < SCI_PT2_T_COUNT; ++k) ms3[k] = ms[k];
  };
  hand_out();
  if (!(eps_pt > 0.0)) { set_error("Fragment::sci_pt2: eps_pt must be positive"); return QEMB_ERR_ARG; }
  if (last_kind_ < 0) { set_error("Fragment::sci_pt2: no solve has run on this fragment since its ERIs or orbitals were last set"); return QEMB_ERR_ARG; }
  if (last_kind_ != QEMB_RDM2_SCI) {
    set_error(std::string("Fragment::sci_pt2: the last solve of this fragment was ") + (last_kind_ == QEMB_RDM2_MP2 ? "MP2" : last_kind_ == QEMB_RDM2_FCI ? "FCI" : "CCSD") + ", not SCI");
    return QEMB_ERR_ARG;
  }
  const int n = n_, o = last_o_;
  if (o == n) return 0;      // a single determinant: nothing outside it
  if (sci_V_.N == 0 || sci_hmo_.empty() || sci_C_.empty()) { set_error("Fragment::sci_pt2: the determinants of the last SCI solve were not kept"); return QEMB_ERR_ARG; }
  char eps_txt[32];
  snprintf(eps_txt, sizeof eps_txt, "%.3g", eps_pt);
  {      // the guard, before anything is allocated
    double room = 0.0;
    QTRY(device_room(sci_mem_limit_, &room));
    if (max_ext <= 0) {      // the largest count that fits beside the integrals (one at the least: the comparison below then refuses)
      const int64_t integrals = sci_pt2_work_bytes(n, o, sci_V_.N, 0) - sci_pt2_bytes(n, o, sci_V_.N, 0);
      max_ext = std::max<int64_t>(1, sci_pt2_max_ext(n, o, sci_V_.N, (int64_t)std::min(room, 9e18) - integrals));
    }
    const double need = (double)sci_pt2_work_bytes(n, o, sci_V_.N, max_ext);
    if (need > room) {
      set_error("Fragment::sci_pt2: n = " + std::to_string(n) + ", eps_pt = " + eps_txt + ", max_ext = " + std::to_string(max_ext) + " over " + std::to_string(sci_V_.N) +
                " determinants give a working set of " + std::to_string((int64_t)need) + " bytes (" + std::to_string(need * 1e-9) + " GB), more than the " + std::to_string(room * 1e-9) +
                " GB of device memory it may take");
      return QEMB_ERR_ALLOC;
    }
  }
  const int64_t n2 = (int64_t)n * n;
  DBuf Vao, CC, Vmo, hd;
  QTRY(fci_mo_integrals(sci_C_, Vao, CC, Vmo));
  Vao.release(); CC.release();
  QTRY(hd.alloc(n2));
  QTRY(dev_h2d(hd, sci_hmo_.data(), sizeof(double) * n2));
  double dbl_bound = 0.0;
  QTRY(sci_double_bound(n, Vmo, &dbl_bound));
  const int rc = qemb::sci_pt2(n, o, hd, Vmo, dbl_bound, sci_V_, sci_res_.e, eps_pt, max_ext, 0, 0, &e, &next, &nb, ms);
  if (rc == 0) hand_out();
  return rc;
}

// ---- Frags.rdm2__ (molbe/solver.py:528): the n^4 tensor of the last solve, written once by one kernel (rdm2_ops.hip)
// Device bytes of one call: the tensor, the 1-RDM, and for MP2 what forming t2 again takes -- ovov, t2, G and the larger of the two integral routes' work space
// (factor: the unpacked factor, its half-rotated virtual columns and Lov, mp2.cpp; block: the two buffers of mo_transform and the ovov block it leaves).
int64_t Fragment::rdm2_bytes(int kind, int o, int with_dm1, int64_t fci_rows) const {
  const int64_t n = n_, v = n - o, n2 = n * n, ov2 = (int64_t)o * v * o * v;
  int64_t words = n2 * n2 + (with_dm1 ? n2 : 0);
  // the tensor and the 1-RDM (sci_rdm12) and the pattern of the matrix, formed again from the resident keys: row pointers, counts, run offsets and 4 bytes per stored element
  if (kind == QEMB_RDM2_SCI) return 8 * (n2 * n2 + 2 * n2) + 20 * sci_V_.N + 4 * sci_res_.nnz;
  if (kind == QEMB_RDM2_FCI) {      // the tensor, A = D D^T, the 1-RDM and D itself, or fci_rows alpha rows of it (fci_rdm12)
    const int64_t ns = fci_string_count(n_, o);
    return 8 * (2 * n2 * n2 + n2 + (v > 0 ? n2 * (fci_rows > 0 && fci_rows < ns ? fci_rows : ns) * ns : 0));
  }
  if (kind == QEMB_RDM2_MP2 && v > 0) {
    const int64_t factor = (int64_t)df_naux_ * (n2 + n * v + (int64_t)o * v), block = 2 * mo_transform_work(n_) + ov2;
    words += 3 * ov2 + (use_factor_route() ? factor : block);
  }
  return 8 * words;
}
int Fragment::rdm2(int kind, int with_dm1, double* out, bool out_on_device) {
  if (kind != QEMB_RDM2_CCSD && kind != QEMB_RDM2_MP2 && kind != QEMB_RDM2_FCI && kind != QEMB_RDM2_SCI) { set_error("Fragment::rdm2: kind must be QEMB_RDM2_CCSD, QEMB_RDM2_MP2, QEMB_RDM2_FCI or QEMB_RDM2_SCI"); return QEMB_ERR_ARG; }
  if (last_kind_ < 0) { set_error("Fragment::rdm2: no solve has run on this fragment since its ERIs or orbitals were last set"); return QEMB_ERR_ARG; }
  if (kind != last_kind_) { set_error(std::string("Fragment::rdm2: the last solve of this fragment was ") + (last_kind_ == QEMB_RDM2_MP2 ? "MP2" : last_kind_ == QEMB_RDM2_FCI ? "FCI" : last_kind_ == QEMB_RDM2_SCI ? "SCI" : "CCSD") + ", not the kind asked for"); return QEMB_ERR_ARG; }
  if (last_relaxed_) { set_error("Fragment::rdm2: relaxed (Lambda) 2-RDMs are not implemented; solve without relax_density"); return QEMB_ERR_UNSUPPORTED; }
  const int n = n_, o = last_o_, v = n - o;
  const int64_t n2 = (int64_t)n * n;
  // ---- the guard: tensor + workspace against what is free (or the fragment's limit), before anything is allocated
  double room = 0.0;
  QTRY(device_room(rdm2_mem_limit_, &room));
  int64_t fci_rows = 0;      // the slab height of an FCI 2-RDM (set_fci_slab): given, or under -1 the largest that fits when the whole D does not
  if (kind == QEMB_RDM2_FCI && v > 0 && fci_slab_ != 0) {
    const int64_t ns = fci_string_count(n, o), per_row = 8 * n2 * ns;
    const int64_t whole = rdm2_bytes(kind, o, with_dm1) - (out_on_device ? 8 * n2 * n2 : 0);
    if (fci_slab_ > 0) fci_rows = std::min(fci_slab_, ns);
    else if ((double)whole > room) fci_rows = std::max<int64_t>(1, std::min<int64_t>(ns, (int64_t)std::floor((room - (double)(whole - per_row * ns)) / (double)per_row)));
  }
  const int64_t need = rdm2_bytes(kind, o, with_dm1, fci_rows) - (out_on_device ? 8 * n2 * n2 : 0);
  if ((double)need > room) {
    set_error("Fragment::rdm2: the 2-RDM of a fragment with n = " + std::to_string(n) + " takes " + std::to_string((double)n2 * (double)n2 * 8e-9) + " GB and " +
              std::to_string((double)(rdm2_bytes(kind, o, with_dm1, fci_rows) - 8 * n2 * n2) * 1e-9) + " GB of workspace, more than the " + std::to_string(room * 1e-9) + " GB of device memory it may take");
    return QEMB_ERR_ALLOC;
  }
  if (kind == QEMB_RDM2_FCI || kind == QEMB_RDM2_SCI) {      // make_rdm2 of the kept vector; with_dm1 = 0: minus the mean-field part (what rdm2__ holds with use_cumulant)
    DBuf R;
    double* target = out;
    if (!out_on_device) { QTRY(R.alloc(n2 * n2)); target = R; }
    if (v == 0) {      // a single determinant: the HF 2-RDM, whose cumulant is zero
      std::vector<double> d2((size_t)(n2 * n2), 0.0);
      if (with_dm1) for (int p = 0; p < n; ++p) for (int q = 0; q < n; ++q) { d2[(size_t)((p * n + p) * n2 + q * n + q)] += 4.0; d2[(size_t)((p * n + q) * n2 + q * n + p)] -= 2.0; }
      QTRY(dev_h2d(target, d2.data(), sizeof(double) * n2 * n2));
    } else if (kind == QEMB_RDM2_SCI) {
      if (sci_V_.N == 0) { set_error("Fragment::rdm2: the determinants of the last SCI solve were not kept"); return QEMB_ERR_ARG; }
      std::vector<double> d1((size_t)n2);
      SciMatrix P;
      QTRY(sci_build(n, nullptr, nullptr, sci_V_.k(), sci_V_.N, -1, "Fragment::rdm2", P));
      QTRY(sci_rdm12(n, sci_V_.k(), sci_V_.N, P.rp(), P.ci(), sci_V_.c, with_dm1 ? -1 : o, d1.data(), target));
    } else {
      if (!fci_c_.p) { set_error("Fragment::rdm2: the vector of the last FCI solve was not kept"); return QEMB_ERR_ARG; }
      const FciTables* T = nullptr;
      QTRY(fci_tables(n, o, &T));
      std::vector<double> d1((size_t)n2);
      fci_rows_used_ = fci_rows; fci_nslab_used_ = fci_slab_count(T->ns, fci_rows);
      QTRY(fci_rdm12(*T, fci_c_, with_dm1 ? -1 : o, d1.data(), target, fci_rows));
    }
    return out_on_device ? dev_sync() : dev_d2h(out, R, sizeof(double) * n2 * n2);
  }
  const double *t1d = nullptr, *t2d = nullptr;
  Mp2Solver mp;      // (lives until the kernel has run)
  if (v > 0 && kind == QEMB_RDM2_CCSD) {
    if (!t_prev_.p || t_prev_o_ != o) { set_error("Fragment::rdm2: the amplitudes of the last CCSD solve were not kept"); return QEMB_ERR_ARG; }
    t1d = t_prev_.p; t2d = t_prev_.p + (int64_t)o * v;
  } else if (v > 0) {
    const bool route = last_route_factor_;      // (mo_route_used keeps describing the solve)
    int rc;
    if (use_factor_route()) {
      rc = mp.run_factor(n, o, 0, df_naux_, df_factor_, C_, eps_);
    } else {
      DBuf X1; bool unpacked = false; MoIntegrals ints;
      rc = scf_operand(X1, &unpacked);
      if (rc == 0) rc = mo_integrals(o, 0, X1, unpacked, ints, false, false);
      X1.release();
      if (rc == 0) rc = mp.run_blocks(std::move(ints), eps_);
    }
    last_route_factor_ = route;
    if (rc) return rc;
    t2d = mp.t2();
  }
  DBuf D, R;
  if (with_dm1) {      // dm1 - 2 I_occ: [[0, t1], [t1^T, 0]] after CCSD (ccsd_rdm.py:10-20), the oo / vv blocks of mp2.make_rdm1 after MP2
    std::vector<double> d((size_t)n2, 0.0);
    if (kind == QEMB_RDM2_MP2) {
      d = mp2_dm1_;
      for (int i = 0; i < o; ++i) d[(size_t)i * n + i] -= 2.0;
    } else if (v > 0) {
      std::vector<double> t1((size_t)o * v);
      QTRY(dev_d2h(t1.data(), t1d, sizeof(double) * o * v));
      for (int i = 0; i < o; ++i) for (int a = 0; a < v; ++a) d[(size_t)i * n + o + a] = d[(size_t)(o + a) * n + i] = t1[(size_t)i * v + a];
    }
    QTRY(D.alloc(n2));
    QTRY(dev_h2d(D, d.data(), sizeof(double) * n2));
  }
  if (out_on_device) {
    QTRY(dev_rdm2_assemble(kind, o, v, t1d, t2d, with_dm1 ? D.p : nullptr, out));
    return dev_sync();      // (t2 of an MP2 call and D go back to the pool on return)
  }
  QTRY(R.alloc(n2 * n2));
  QTRY(dev_rdm2_assemble(kind, o, v, t1d, t2d, with_dm1 ? D.p : nullptr, R));
  return dev_d2h(out, R, sizeof(double) * n2 * n2);
}

// ---- the perturbative triples correction of the last CCSD solve (ccsd_t.cpp), on MO blocks formed again as rdm2() forms again what it needs
int64_t Fragment::ccsd_t_work_bytes(int o, int tile) const {
  const int64_t n = n_, v = n - o, O = o, n2 = n * n, np = npair(n), npv = v * (v + 1) / 2, nm = v * (v - 1) / 2;
  const int64_t kept = O * v * v * v + O * O * O * v + O * O * v * v;
  // mo_transform / mo_transform_factor without site rows: X0, X1, the six blocks, the packed ovvv of the factor route and the (+/-) packed ladder operands
  // (rows padded to an even length); on the factor route the unpacked and half-transformed factor and its packed MO image
  int64_t transform = 2 * mo_transform_work(n_) + O * O * O * O + kept + 2 * O * O * v * v + npv * (npv + 1) + std::max<int64_t>(nm, 1) * (nm + 2);
  if (use_factor_route()) transform += (int64_t)df_naux_ * (2 * n2 + np) + O * v * npv;
  return std::max(8 * transform, 8 * kept + ccsd_t_bytes(O, v, tile));
}
int Fragment::ccsd_t(double* e_t, CcsdTStats* stats, double* ms_integrals) {
  if (e_t) *e_t = 0.0;
  if (stats) *stats = CcsdTStats();
  if (ms_integrals) *ms_integrals = 0.0;
  if (last_kind_ < 0) { set_error("Fragment::ccsd_t: no solve has run on this fragment since its ERIs or orbitals were last set"); return QEMB_ERR_ARG; }
  if (last_kind_ != QEMB_RDM2_CCSD) {
    set_error(std::string("Fragment::ccsd_t: the last solve of this fragment was ") + (last_kind_ == QEMB_RDM2_MP2 ? "MP2" : last_kind_ == QEMB_RDM2_FCI ? "FCI" : "SCI") + ", not CCSD");
    return QEMB_ERR_ARG;
  }
  const int n = n_, o = last_o_, v = n - o;
  if (v == 0) return 0;      // a single determinant
  if (!t_prev_.p || t_prev_o_ != o) { set_error("Fragment::ccsd_t: the amplitudes of the last CCSD solve were not kept"); return QEMB_ERR_ARG; }
  if (o < 2 || v < 2) return 0;      // no triples: nothing is formed
  // ---- the guard, before anything is allocated: the largest tile whose working set fits
  double room = 0.0;
  QTRY(device_room(ccsd_t_mem_limit_, &room));
  const int64_t kept = 8 * ((int64_t)o * v * v * v + (int64_t)o * o * o * v + (int64_t)o * o * v * v);      // the three blocks beside the working set of ccsd_t_energy
  const int tile = (double)ccsd_t_work_bytes(o, 1) <= room ? ccsd_t_pick_tile(o, v, room - (double)kept) : 0;
  if (tile < 1) {
    const double need = (double)ccsd_t_work_bytes(o, 1);
    set_error("Fragment::ccsd_t: n = " + std::to_string(n) + ", n_occ = " + std::to_string(o) + ": the triples correction takes " + std::to_string((int64_t)need) + " bytes (" +
              std::to_string(need * 1e-9) + " GB) with the smallest tile, more than the " + std::to_string(room * 1e-9) + " GB of device memory it may take");
    return QEMB_ERR_ALLOC;
  }
  // ---- ovvv, ovoo, ovov by the route the fragment would take; everything else the transformation leaves goes back at once
  const auto t0 = std::chrono::steady_clock::now();
  DBuf ovvv, ovoo, ovov;
  {
    const bool route = last_route_factor_;      // (mo_route_used keeps describing the solve)
    DBuf X1; bool unpacked = false; MoIntegrals ints;
    int rc = scf_operand(X1, &unpacked);
    if (rc == 0) rc = mo_integrals(o, 0, X1, unpacked, ints, false, false);
    last_route_factor_ = route;
    s4_transient_.release();
    if (rc) return rc;
    ovvv = std::move(ints.ovvv); ovoo = std::move(ints.ovoo); ovov = std::move(ints.ovov);
  }
  QTRY(dev_sync());
  if (ms_integrals) *ms_integrals = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return ccsd_t_energy(o, v, t_prev_.p, t_prev_.p + (int64_t)o * v, ovvv, ovoo, ovov, eps_, eps_.p + o, tile, e_t, stats);
}

int Fragment::solve_mp2_batch(const std::vector<Fragment*>& frs, const std::vector<int>& o, const std::vector<const double*>& h, const std::vector<const double*>& dm0,
                              const FragmentOptions& opt, int eeval, std::vector<FragmentResult>& res, const std::vector<BatchOutputs>& outs) {
  const int F = (int)frs.size();
  if (F == 0) return 0;
  res.assign(F, FragmentResult());
  Fanout per_fragment(F);
  QTRY(per_fragment.init());
  return per_fragment([&](int f) {
    return frs[f]->solve_mp2(o[f], h[f], dm0[f], opt, eeval, &res[f], outs[f].mo_coeff, outs[f].mo_energy, outs[f].rdm1_emb, outs[f].rdm1_mo, outs[f].t2);
  });
}

}  // namespace qemb
