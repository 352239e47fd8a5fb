// fragment.h -- one embedded fragment resident on the device and the body of the fragment sweep
// (be_func's loop body, molbe/solver.py:301-547 == run_solver, molbe/be_parallel.py:40-307).
#pragma once
#include <string>
#include <cstdint>
#include <memory>
#include <vector>
#include "ccsd.h"
#include "cc_lambda.h"
#include "scf.h"
#include "fci.h"
#include "sci.h"
#include "ccsd_t.h"

namespace qemb {

struct FragmentOptions {
  CcsdOptions cc;
  ScfOptions scf;
  int warm_start = 0;      // reuse converged t1/t2 of the previous solve as the CCSD guess (reference restarts from MP2)
  int keep_amplitudes = 1; // keep t1/t2 resident after the solve
  int relax_density = 0;   // solve_ccsd(relax=True), solver.py:925-939: Lambda equations + response densities
  LambdaOptions lam;
  int strict = 1;          // 0: non-convergence is reported (QEMB_WARN_NOCONV) instead of being an error, like PySCF's warnings
};

struct FragmentResult {
  int n_iter = 0;
  int lambda_iters = 0;
  int scf_cycles = 0;
  int ccsd_converged = 0, scf_converged = 0;
  double e_corr_mo = 0.0;      // CCSD correlation energy of the embedding problem
  double e_scf = 0.0;          // fragment RHF energy (electronic, of h = fock + heff)
  double e_frag[3] = {0, 0, 0};   // [e1, e2, ec] weighted centre sums (get_frag_energy, helper.py:333-339)
  double ebe_hf = 0.0;         // update_ebe_hf (pfrag.py:327-400) evaluated with the SCF orbitals of this solve
};

class Fragment {
 public:
  Fragment(int n, int nf) : n_(n), nf_(nf) {}
  int last_lambda_iters = 0;
  int n() const { return n_; }
  int nf() const { return nf_; }
  int o() const { return o_; }
  // ERIs: 4-fold packed (npair x npair), the layout of dataset "f{I}" (mbe.py:1039)
  int set_eri_s4_host(const double* s4);
  int set_eri_s4_dev(const double* s4_dev);     // device-to-device copy
  int adopt_eri_s4(DBuf&& s4);                  // takes the block a transform just produced (no copy: 4.7 GB at n = 220)
  double* eri_s4() { return eri_s4_.p; }
  // The fragment's 3-index factor B[naux][npair(n)] with eri_s4 = B^T B (bb of molbe/eri_onthefly.py:141-143), optional.  With it the MO integrals
  // of a solve come from the factor (mo_transform_factor, ccsd.cpp) while that is the cheaper route; set it AFTER the ERIs (new ERIs drop it).
  int set_df_factor_host(int naux, const double* B);
  int set_df_factor_dev(int naux, const double* B_dev);
  int adopt_df_factor(DBuf&& B, int naux);
  void clear_df_factor();
  // A fragment that LIVES on its factor (round 5): no 4-fold packed block is resident -- 8 naux npair bytes instead of 8 npair^2 (128 MB instead of 4.7 GB at
  // n = 220, naux = 660).  J / K of the fragment RHF, the MO integrals, the energies and the CPHF response all come from the factor; the block is formed on
  // demand only (export_eri_s4, or a solve with the four-index route forced: a transient of that solve).  Any set_eri_s4 / adopt_eri_s4 ends the mode.
  int set_df_only_host(int naux, const double* B);
  int set_df_only_dev(int naux, const double* B_dev);
  int adopt_df_only(DBuf&& B, int naux);
  bool factor_only() const { return !eri_s4_.p && df_factor_.p; }
  bool has_eris() const { return eri_s4_.p || df_factor_.p; }
  int export_eri_s4(double* s4_host);               // the resident block, or B^T B formed for this call
  int export_df_factor(double* B_host);             // the resident factor (df_naux() x npair(n)); an error without one
  int64_t resident_bytes() const;                   // device bytes this fragment keeps between solves (ERIs / factor, orbitals, kept amplitudes)
  int df_naux() const { return df_naux_; }
  int set_mo_route(int route);                  // -1: by cost (default), 0: four-index transformation of eri_s4, 1: the factor (an error without one)
  bool use_factor_route() const;
  bool last_route_was_factor() const { return last_route_factor_; }
  // static data for the energies: h1, veff0 (n x n host), centre weight/indices
  void set_energy_data(const double* h1, const double* veff0, const double* veff, double weight, const int* centers, int ncen);
  // The sweep body.  h = fock + heff (n x n host), dm0 (n x n host, may be null -> core guess).
  // Outputs (host, nullable): mo_coeff n*n, mo_energy n, rdm1_emb n*n (= C rdm1 C^T / 2), rdm1_mo n*n, t1 o*v, t2 o*o*v*v.
  int solve(int o, const double* h, const double* dm0, const FragmentOptions& opt, int eeval, FragmentResult* res,
            double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* t1, double* t2);
  // The same in three steps -- everything before the CCSD iterations, (the iterations: cc_->kernel or the lock-step loop of solve_batch),
  // everything after -- so that several fragments can share the middle step.  solve_end keeps what belongs to CCSD (amplitudes, Lambda equations, the 1-RDM, the
  // per-site two-body energies) and ends in finish_solve, the tail it shares with solve_mp2 and solve_fci.
  int solve_begin(int o, const double* h, const double* dm0, const FragmentOptions& opt, int eeval, FragmentResult* res);
  // ... and solve_begin itself in two halves: the fragment RHF (host round trips inside), then MO integrals + CCSD set-up + starting amplitudes (launches only)
  int solve_begin_scf(int o, const double* h, const double* dm0, const FragmentOptions& opt, int eeval, FragmentResult* res);
  int solve_begin_cc();
  int solve_end(double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* t1, double* t2);
  struct BatchOutputs { double *mo_coeff = nullptr, *mo_energy = nullptr, *rdm1_emb = nullptr, *rdm1_mo = nullptr, *t1 = nullptr, *t2 = nullptr; };
  // every fragment of a sweep in one call: solve_begin / solve_end per fragment on its own execution context (host thread + stream),
  // the CCSD iterations of all of them in lock step (one grouped launch per operation).  Results as from solve(), bit for bit.
  static int solve_batch(const std::vector<Fragment*>& frs, const std::vector<int>& o, const std::vector<const double*>& h,
                         const std::vector<const double*>& dm0, const FragmentOptions& opt, int eeval, std::vector<FragmentResult>& res,
                         const std::vector<BatchOutputs>& outs, LockstepStats* stats);
  // solver == "MP2" of be_func (molbe/solver.py:313-317): fragment RHF -> density-fitted MP2 (mp2.h) -> unrelaxed MP2 1-RDM (oo and vv blocks) -> back-rotation ->
  // fragment energies.  Of opt only scf and strict are read; no amplitudes are kept.  Outputs as solve(); there is no t1.
  int solve_mp2(int o, const double* h, const double* dm0, const FragmentOptions& opt, int eeval, FragmentResult* res,
                double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* t2);
  // ... for every fragment of a sweep, spread over the execution contexts that exist (MP2 has no iterations to run in lock step).  Results as from solve_mp2(), bit for bit.
  static int solve_mp2_batch(const std::vector<Fragment*>& frs, const std::vector<int>& o, const std::vector<const double*>& h, const std::vector<const double*>& dm0,
                             const FragmentOptions& opt, int eeval, std::vector<FragmentResult>& res, const std::vector<BatchOutputs>& outs);
  // solver == "FCI" of be_func (molbe/solver.py:339-342, :507-547): fragment RHF -> determinant-space FCI of h = fock + heff with the fragment's ERIs in the fragment-MO
  // basis, nelec = (o, o) (fci.h) -> make_rdm1 -> back-rotation -> get_frag_energy with the cumulant of make_rdm2, contracted on the device against the resident
  // integrals.  Of opt only scf and strict are read.  civec: ns * ns (host, nullable).  n > 16: QEMB_ERR_UNSUPPORTED; the working set against the free device memory
  // (or set_fci_mem_limit): QEMB_ERR_ALLOC.  The vector stays on the device for a later rdm2(QEMB_RDM2_FCI).
  int solve_fci(int o, const double* h, const double* dm0, const FragmentOptions& opt, const FciOptions& fopt, int eeval, FragmentResult* res,
                double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* civec);
  void set_fci_mem_limit(int64_t bytes) { fci_mem_limit_ = bytes; }
  // The slab height of solve_fci and rdm2(QEMB_RDM2_FCI): 0 (default) the whole space in one piece -- the path and the guard above --, k > 0 the slab kernels with
  // k alpha rows of D and G at a time (fci.h; k >= ns: one slab), -1 unslabbed when that fits the room, else the largest height that does.  The guard of a slabbed
  // solve compares fci_bytes_slab with the same room.  fci_slab_used: what the last FCI solve or FCI 2-RDM call ran with (rows 0, one slab: unslabbed).
  int set_fci_slab(int64_t rows) { if (rows < -1) { set_error("Fragment::set_fci_slab: rows = " + std::to_string(rows) + "; need 0 (off), a positive slab height or -1 (automatic)"); return QEMB_ERR_ARG; } fci_slab_ = rows; return 0; }
  void fci_slab_used(int64_t* rows, int64_t* n_slab) const { if (rows) *rows = fci_rows_used_; if (n_slab) *n_slab = fci_nslab_used_; }
  // solver == "SCI-hip": the selected-CI branch of be_func (molbe/solver.py:412-462) as the heat-bath selection of sci.h on the integrals solve_fci forms, for
  // n <= 64; everything after the vector is the tail of solve_fci (make_rdm1, cumulant of the 2-RDM on the device, fci_e2_sites, finish_solve).  The guard compares
  // sci_bytes with the free device memory (or set_sci_mem_limit) before anything is allocated; the determinants and the vector stay on the device for a later
  // rdm2(QEMB_RDM2_SCI) and sci_dets(); the matrix does not.
  int solve_sci(int o, const double* h, const double* dm0, const FragmentOptions& opt, const SciOptions& sopt, int eeval, FragmentResult* res,
                double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo);
  void set_sci_mem_limit(int64_t bytes) { sci_mem_limit_ = bytes; }
  const SciResult& sci_result() const { return sci_res_; }
  int sci_dets(uint64_t* alpha, uint64_t* beta, double* c) const;
  // the screened Epstein-Nesbet correction (sci.h: sci_pt2) of what the last SCI solve left -- the determinants, the vector, e_sci and the kept orbitals, from which
  // h and V in the fragment-MO basis are formed again (fci_mo_integrals).  A diagnostic of the embedding problem: it is added to no energy.  max_ext <= 0: the
  // largest count the room (free device memory, or set_sci_mem_limit) allows.  The working set sci_pt2_work_bytes is compared with the room before anything is
  // allocated.  Outputs nullable; ms3: host wall time of screen, sorts / merges, rows.  nsocc == n: zeros.
  int sci_pt2(double eps_pt, int64_t max_ext, double* e_pt2, int64_t* n_ext, int* batches, double* ms3);
  static int64_t sci_pt2_work_bytes(int n, int nsocc, int64_t ndet, int64_t max_ext);      // sci_pt2_bytes and the n^4 pieces of fci_mo_integrals, h
  double fci_residual() const { return fci_residual_; }
  // The perturbative triples correction E_(T) (ccsd_t.h) of the last CCSD solve of this fragment, relaxed or not, from the kept t1 / t2, the orbital energies
  // and ovvv, ovoo, ovov formed again by the route the fragment would take (factor or block), as rdm2() forms t2 of an MP2 solve again.  A diagnostic of the
  // embedding problem: it is added to no energy.  No solve, a last solve that was not CCSD, amplitudes that were not kept, or ERIs / orbitals changed since:
  // QEMB_ERR_ARG.  The tile is the largest of kCcsdTTiles whose working set ccsd_t_work_bytes fits the room (free device memory, or set_ccsd_t_mem_limit); if
  // Tv = 1 does not fit: QEMB_ERR_ALLOC naming n, before anything is allocated.  mo_route_used, resident_bytes and the kept amplitudes stay as the solve left
  // them.  No virtual orbitals: 0.0.  ms_integrals: host wall time of forming the blocks again.  Outputs nullable.
  int ccsd_t(double* e_t, CcsdTStats* stats, double* ms_integrals);
  void set_ccsd_t_mem_limit(int64_t bytes) { ccsd_t_mem_limit_ = bytes; }
  // device bytes of ccsd_t() with that tile: the larger of the transformation (its two work buffers, every block it leaves, the factor's images on that route)
  // and of the three kept blocks with ccsd_t_bytes
  int64_t ccsd_t_work_bytes(int o, int tile) const;
  // the kept t1 / t2 and Lambda multipliers go back to the pool: the next solve starts from the MP2 guess; rdm2(QEMB_RDM2_CCSD) and ccsd_t() are refused until then
  void drop_amplitudes() { t_prev_.release(); z_prev_.release(); t_prev_o_ = z_prev_o_ = -1; }
  int last_nsocc() const { return last_kind_ >= 0 ? last_o_ : -1; }      // occupied orbitals of the last solve; -1: none since the ERIs or orbitals were set
  // Frags.rdm2__ (molbe/solver.py:528) of the last solve in the fragment-MO basis, out: n^4 (host).  kind QEMB_RDM2_CCSD: make_rdm2_urlx from the kept t1 / t2;
  // QEMB_RDM2_MP2: mp2.make_rdm2, t2 formed again from the resident orbitals (an MP2 solve keeps no amplitudes).  One kernel writes the tensor (rdm2_ops.hip).
  // A relaxed solve: QEMB_ERR_UNSUPPORTED; no solve of that kind, or ERIs / orbitals changed since: QEMB_ERR_ARG.
  // out_on_device: out is an n^4 device buffer of the caller (the full-basis accumulation); the guard then counts the workspace alone
  int rdm2(int kind, int with_dm1, double* out, bool out_on_device = false);
  // device bytes rdm2() may take (tensor + workspace); < 0: whatever is free
  void set_rdm2_mem_limit(int64_t bytes) { rdm2_mem_limit_ = bytes; }
  int64_t rdm2_bytes(int kind, int o, int with_dm1, int64_t fci_rows = 0) const;      // 8 n^4 + the workspace of the call (fci_rows > 0: D of an FCI 2-RDM in slabs of that height)
  // Bench hooks: set up the CCSD problem once (SCF + transform), then time single iterations.
  int prepare_ccsd(int o, const double* h, const double* dm0, const FragmentOptions& opt);
  int ccsd_iterate(int niter, double* e_corr, double* normt);
  int ccsd_export(const char* name, double* host, int64_t nelem) {
    if (!cc_) { set_error("Fragment: prepare_ccsd first"); return QEMB_ERR_ARG; }
    if (name && std::string(name) == "mo_coeff") {      // the orbitals the MO integrals were transformed with
      if (nelem != (int64_t)n_ * n_) { set_error("export_block: element count mismatch"); return QEMB_ERR_ARG; }
      return dev_d2h(host, C_, sizeof(double) * nelem);
    }
    return cc_->export_block(name, host, nelem);
  }
  int ccsd_reset();                              // back to the MP2 guess
  // fragment RHF only (Frags.scf(fs=True), mbe.py:1160): outputs host n*n / n / n*n / n*n, nullable
  int scf_only(int o, const double* h, const double* dm0, const ScfOptions& opt, double* mo_coeff, double* mo_energy,
               double* J_host, double* K_host, ScfResult* sres);
  // CPHF response of the fragment RHF density to npot one-body perturbations v_p (n x n each, host):
  // dP_p = d(P)/d(lambda_p), P the spin-summed... see fragment.cpp.  dPs: npot x n x n (host).
  int cphf_response(int o, const double* h, const double* dm0, const ScfOptions& opt, const double* vpots, int npot, double* dPs);
  // J/K based pieces that do not need a correlated solve (row a6 / a15)
  int hf_veff_from_dm(const double* P_host, double* J_host, double* K_host);   // J,K of an n x n density

 private:
  int run_scf(int o, const double* h, const double* dm0, const ScfOptions& opt, double* X0, ScfResult* sres, bool warm = false);
  int materialize_s4(DBuf& out);                    // B^T B over packed pairs
  const double* s4_ptr() const { return eri_s4_.p ? eri_s4_.p : s4_transient_.p; }
  DBuf s4_transient_;                               // factor-only fragment, four-index route forced: the block for the duration of one solve
  int scf_operand(DBuf& X1, bool* unpacked);
  int check_df_factor();
  int mo_integrals(int o, int nf, DBuf& X1, bool x1_unpacked, MoIntegrals& ints, bool build_Vl, bool build_T34);
  // The tail every solver shares (fragment.cpp): after its correlated step a solver hands finish_solve its MO-basis 1-RDM (the rdm1_mo output), its per-site two-body
  // energies and what rdm2() has to know of the solve; finish_solve forms hf_dm = Co Co^T and rdm1_emb = C rdm1_mo C^T / 2 -- from t1 on the host where the density is
  // [[2 I, t1], [t1^T, 0]] (unrelaxed CCSD), else by two products on the device --, copies the four outputs, evaluates the energies (frag_energies), waits for the
  // device and returns the solve's status (QEMB_WARN_NOCONV for an unconverged one)
  int finish_solve(const std::vector<double>* t1, const std::vector<double>& dm, const std::vector<double>& e2, int kind, bool relaxed, bool unconverged,
                   double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo);
  int frag_energies(const std::vector<double>& rdm, const std::vector<double>& hfdm, const std::vector<double>& e2, FragmentResult* res);
  int check_energy_data(int eeval) const;           // QEMB_ERR_ARG for an energy evaluation without set_energy_data; from solve_begin_scf, which every solver passes
  DBuf df_factor_; int df_naux_ = 0; int mo_route_ = -1; bool last_route_factor_ = false;
  bool have_C_ = false; int c_nocc_ = -1;    // C_ holds the orbitals of a converged earlier solve with c_nocc_ occupied orbitals (the Jacobi eigensolver starts in that basis)
  int n_, nf_, o_ = -1;
  DBuf eri_s4_;
  std::vector<double> h1_, veff0_, veff_;
  double weight_ = 1.0;
  std::vector<int> centers_;
  // what solve_begin_scf hands to the solver's own step and to finish_solve
  struct SolvePending {
    int o = 0, eeval = 0; FragmentOptions opt; FragmentResult* res = nullptr;
    bool unconverged = false, no_virtuals = false;
    std::vector<double> C, eps;
    DBuf X1; bool x1_unpacked = false;      // the half-unpacked tensor between the two halves of solve_begin (four-index route)
    unsigned long long alloc_hash = 0;      // dev_alloc_trace_end over integrals + set-up + starting amplitudes of this solve
  } sp_;
  // the recorded amplitude update of the last lock-step solve and the buffer layout it is valid for (tape_for_lockstep / retire_solver)
  struct TapeCache { dev_tape_t tape = nullptr; unsigned long long key = 0; ~TapeCache() { if (tape) (void)dev_tape_destroy(tape); } } tape_cache_;
  unsigned long long tape_key_ = 0;
  int tape_for_lockstep(int peers);
  void retire_solver();
  // state of the last solve
  DBuf C_, eps_, dm_, J_, K_;
  std::unique_ptr<CcsdSolver> cc_;
  DBuf t_prev_;   // warm-start amplitudes (t1 then t2)
  DBuf z_prev_;   // warm-start Lambda multipliers (relax_density)
  int z_prev_o_ = -1;
  int t_prev_o_ = -1;
  // what rdm2() needs of the last solve: its kind (-1: none, or the orbitals / ERIs changed since), whether it was relaxed, nsocc; after an MP2 solve the
  // 1-RDM (host, n x n): it keeps no amplitudes to form it from (CCSD: [[2 I, t1], [t1^T, 0]] from the kept t1 when asked)
  int last_kind_ = -1, last_o_ = 0; bool last_relaxed_ = false;
  std::vector<double> mp2_dm1_;
  int64_t rdm2_mem_limit_ = -1;
  int64_t ccsd_t_mem_limit_ = -1;
  // after an FCI solve: the CI vector (device, ns * ns)
  DBuf fci_c_;
  double fci_residual_ = 0.0;
  int64_t fci_mem_limit_ = -1;
  int64_t fci_slab_ = 0, fci_rows_used_ = 0, fci_nslab_used_ = 1;
  int fci_mo_integrals(const std::vector<double>& C, DBuf& Vao, DBuf& CC, DBuf& Vmo);
  int fci_e2_sites(const double* CC, const double* G2, const double* Vao, std::vector<double>& e2);      // the cumulant contracted with the integrals, per fragment site
  // after an SCI solve: the sorted determinants with the vector (device, 24 bytes per determinant); rdm2() forms the pattern of the matrix over them again;
  // h in the fragment-MO basis and the orbitals (host, n x n each) for sci_pt2()
  SciSpace sci_V_;
  SciResult sci_res_;
  std::vector<double> sci_hmo_, sci_C_;
  int64_t sci_mem_limit_ = -1;
  void forget_solve() { last_kind_ = -1; sci_V_ = SciSpace(); sci_res_ = SciResult(); sci_hmo_.clear(); sci_C_.clear(); }
};

// lock-step tapes kept from an earlier solve / recorded anew since the last reset (all fragments of the process)
void tape_cache_counters(long long* reused, long long* recorded, int reset);

}  // namespace qemb
