/* qemb_hip.h -- C ABI of libqemb_hip.so: the MI355X (gfx950) per-fragment embedding solver that sits behind
 * QuEmb's Frags / solver / int_transform seams (troyvvgroup/quemb).
 *
 * Conventions (reference precedent: shared/external/unrestricted_utils.py:142-160 -- caller-allocated
 * numpy buffers handed to a C function as plain pointers):
 *   - plain C types only; FP64; row-major; every HOST buffer (in and out) is allocated by the caller;
 *   - device-resident state lives behind opaque handles with explicit *_free;
 *   - every function returns 0 on success and <0 on failure; qemb_last_error() returns the message
 *     (the reference's natives throw C++ exceptions mapped to Python -- _cpp/eri_sparse_DF.cpp:40-62 --
 *     a C ABI returns a status instead and the Python shim raises);
 *   - pair index ij = i(i+1)/2 + j, i >= j (shared/helper.py:260-276, _cpp/indexers.hpp:75-79);
 *   - embedding orbitals are ordered fragment sites first, then bath (molbe/pfrag.py:489-491).
 *   - There is NO CPU fallback: without a visible HIP device qemb_init() fails.
 *   - This header is the PRODUCT ABI (what a QuEmb binding calls).  The device primitives the drivers are composed of,
 *     the device timers and the measurement / tuning hooks used by tests/, bench.py and tools/ are declared in qemb_hip_ops.h.
 */
#ifndef QEMB_HIP_H
#define QEMB_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define QEMB_OK 0
#define QEMB_ERR_ARG (-1)
#define QEMB_ERR_ALLOC (-2)
#define QEMB_ERR_DEVICE (-3)
#define QEMB_ERR_NOCONV (-4)
#define QEMB_ERR_NUMERIC (-5)
#define QEMB_ERR_UNSUPPORTED (-6) /* a well-formed request for something this library does not implement (e.g. a relaxed 2-RDM) */
#define QEMB_WARN_NOCONV 1       /* only with strict_convergence = 0: results returned, but a solve did not converge */

/* ---------------------------------------------------------------- library / device ------------- */
int qemb_init(int device);                 /* select the GPU, create the library stream            */
const char* qemb_last_error(void);
const char* qemb_backend(void);            /* "hip-gfx950"                                         */
int qemb_sync(void);                      /* the calling thread's stream (execution context)      */
int qemb_device_sync(void);               /* every stream of the device                           */
int qemb_mem_info(size_t* free_bytes, size_t* total_bytes);

/* raw device buffers (for callers that keep tensors resident, e.g. bench.py / multi-fragment sweeps) */
int qemb_malloc(void** dptr, size_t bytes);
int qemb_free(void* dptr);                 /* parks the block for reuse (caching allocator)       */
int qemb_trim(void);                       /* hand every parked block back to the driver          */
int qemb_trim_all(void);              /* the same for EVERY execution context (their streams are drained first): between phases with very different working sets */
int qemb_h2d(void* dptr, const void* host, size_t bytes);
int qemb_d2h(void* host, const void* dptr, size_t bytes);
/* upload that only ORDERS the copy on the calling context's stream (for data that context consumes; qemb_sync or any later download of the context completes it).  The host
 * buffer is free on return: copies of up to 256 KB leave from pinned slots of the context (round 5 -- the runtime's pageable path serialised the host threads of a
 * batched sweep), larger ones fall back to the waiting path of qemb_h2d. */
int qemb_h2d_async(void* dptr, const void* host, size_t bytes);
int qemb_d2d(void* dst, const void* src, size_t bytes);

/* Execution contexts (one HIP stream + workspaces + block cache each; no reference counterpart -- the reference overlaps
 * fragments with a process pool, be_parallel.py:484).  qemb_ctx_count(n) makes contexts 0..n-1 available (0 = default) and
 * returns how many exist (or < 0); qemb_ctx_bind(k) binds the CALLING host thread to context k, so that several host
 * threads can each drive a fragment on their own stream (device timers of a context: qemb_ctx_timer_read, qemb_hip_ops.h).
 * qemb_ctx_partition(parts): contexts 1, 2, ... are spread over `parts` disjoint, interleaved sets of compute units (0 / 1: every context on the
 * whole chip), so that the HBM-bound passes of one large fragment run beside the MFMA-bound products of another; existing contexts are drained and get
 * new streams -- call it between sweeps, not while other threads are solving. */
int qemb_ctx_count(int n);
int qemb_ctx_bind(int k);
int qemb_ctx_partition(int parts);

/* ---------------------------------------------------------------- fragment solver (hot path) ----- */
/* Replaces, per fragment, the body of be_func's loop -- molbe/solver.py:301-547 -- and its worker twin
 * run_solver(h1, dm0, ..., nao, nocc, n_frag, weight_and_relAO_per_center, TA, h1_e, solver, eri_file,
 * veff, veff0, ...) -> (e_f, mo_coeff, rdm1, rdm2s, rdm1_tmp), molbe/be_parallel.py:40-60, :301-307:
 * fragment RHF (helper.py:73-151) -> solve_ccsd (solver.py:829-946) -> rdm1 back-rotation (solver.py:496-505)
 * -> get_frag_energy (helper.py:220-339).  The 2-RDM is never materialised: its contraction with the
 * fragment ERIs is evaluated from t1/t2 directly (identical result).                      */
typedef struct {
  uint32_t struct_size;      /* sizeof(qemb_solver_opts) of the header the caller was built against; qemb_default_opts sets it and
                              * every entry point that takes options rejects another value (QEMB_ERR_ARG): a binding whose field
                              * list has drifted from this header fails loudly instead of reading flags out of padding           */
  double cc_conv_tol;        /* |dE_corr|          default 1e-10 (PySCF 1e-7)                      */
  double cc_conv_tol_normt;  /* |dt|               default 1e-8  (PySCF 1e-5)                      */
  int cc_max_cycle;          /*                    default 100   (PySCF 50)                        */
  int cc_diis_space;         /*                    default 6     (PySCF 6)                         */
  double scf_conv_tol;       /* |dE_scf|           default 1e-11 (PySCF 1e-9)                      */
  double scf_conv_tol_grad;  /* ||FD-DF||          default 1e-7                                    */
  int scf_max_cycle;         /*                    default 50    (molbe/helper.py:118)             */
  int scf_diis_space;        /*                    default 8                                       */
  int warm_start;            /* reuse t1/t2 of the previous sweep as the CCSD guess (default 0)      */
  int verbose;
  int relax_density;         /* solve_ccsd(relax=True), solver.py:925-939: CCSD Lambda equations, response 1-RDM in
                              * rdm1_mo / rdm1_emb and the relaxed with_dm1=False 2-RDM in e_frag (default 0)          */
  double lambda_conv_tol;    /* |dz|               default 1e-8  (PySCF solve_lambda 1e-5)          */
  int lambda_max_cycle;      /*                    default 100                                      */
  int strict_convergence;    /* 1 (default): a fragment RHF / CCSD / Lambda solve that does not converge is an error, status
                              * QEMB_ERR_NOCONV, no outputs.  0: the reference's behaviour -- PySCF warns and carries on with what it
                              * has (helper.py:128-149, solver.py:905-912): every output is filled from the unconverged state and the
                              * call returns QEMB_WARN_NOCONV (> 0); qemb_last_error() says which solve it was.            */
} qemb_solver_opts;
void qemb_default_opts(qemb_solver_opts* opts);   /* always start from this; then change single fields */

typedef void* qemb_frag_t;   /* opaque: one fragment with its ERIs resident in HBM                   */
int qemb_frag_create(int n, int n_f, qemb_frag_t* out);
int qemb_frag_free(qemb_frag_t f);
/* fragment ERIs, 4-fold packed (npair(n) x npair(n)): the dataset "f{I}" of eri_file.h5 (mbe.py:1039) */
int qemb_frag_set_eri_s4(qemb_frag_t f, const double* eri_s4_host);
int qemb_frag_set_eri_s4_dev(qemb_frag_t f, const double* eri_s4_dev);
int qemb_frag_get_eri_s4(qemb_frag_t f, double* eri_s4_host);
/* Optional: the fragment's fitted 3-index factor B[naux][npair(n)] (rows L, unique pairs i >= j), the `bb` of
 * integral_direct_DF whose product `bb.T @ bb` IS the block above (molbe/eri_onthefly.py:141-143).  With it a solve forms
 * its MO-basis integrals from the factor -- transformed with the fragment's orbitals and multiplied with itself,
 * 2 naux npair(n)^2 flops -- instead of the four quarter transformations of the packed block (PySCF's ao2mo inside
 * cc.CCSD(...).ao2mo(), molbe/solver.py:900), while that is the cheaper route (naux <= 8 n); the results agree to
 * rounding.  Set it AFTER the ERIs it belongs to: new ERIs drop it, and a factor whose product differs from the resident block (random probe of the
 * WHOLE block: B^T (B x) against eri_s4 x for two vectors x, 1e-9 relative) is refused with QEMB_ERR_ARG and no factor is kept.  qemb_df_transform(..., frag) hands it over itself.
 * qemb_frag_mo_route: -1 choose by cost (default), 0 always the four-index transformation, 1 always the factor.        */
int qemb_frag_set_df_factor(qemb_frag_t f, int naux, const double* B_host);
int qemb_frag_set_df_factor_dev(qemb_frag_t f, int naux, const double* B_dev);
int qemb_frag_mo_route(qemb_frag_t f, int route);
/* A fragment that LIVES on its 3-index factor (round 5): qemb_frag_set_df_only[_dev] sets B (naux x npair(n), eri = B^T B) and drops any resident
 * 4-fold packed block -- 8 naux npair bytes resident instead of 8 npair^2 (128 MB instead of 4.7 GB at n = 220, naux = 660).  J / K of the fragment RHF
 * (helper.py:28-69 get_veff: J = B^T (B Dp), K = sum_L (B_L Co)(B_L Co)^T), the MO integrals, energies, relaxed densities and the CPHF response come
 * from the factor; qemb_frag_jk and qemb_frag_get_eri_s4 keep working (the block is formed for that call: B^T B).  qemb_frag_mo_route(f, 0) still forces
 * the four-index transformation (the block is then a transient of each solve).  Any qemb_frag_set_eri_s4 ends the mode.
 * qemb_frag_resident_bytes: device bytes the fragment keeps between solves (ERIs and / or factor, orbitals, densities, kept amplitudes).            */
int qemb_frag_set_df_only(qemb_frag_t f, int naux, const double* B_host);
int qemb_frag_set_df_only_dev(qemb_frag_t f, int naux, const double* B_dev);
int qemb_frag_resident_bytes(qemb_frag_t f, int64_t* bytes);
int qemb_frag_mo_route_used(qemb_frag_t f, int* used_factor, int* naux);   /* what the last solve did; naux of the factor held (0: none) */
/* h1 = TA^T hcore TA, veff0 = TA^T V_hf TA, veff (may be NULL), centre weight and indices
 * (Frags.weight_and_relAO_per_center, pfrag.py:100)                                                  */
int qemb_frag_set_energy_data(qemb_frag_t f, const double* h1, const double* veff0, const double* veff,
                              double weight, const int* centers, int ncenter);
/* J[p,q] = (pq|rs) P[r,s], K[p,r] = (pq|rs) P[q,s] from the resident ERIs (helper.py:64 dot_eri_dm)   */
int qemb_frag_jk(qemb_frag_t f, const double* P, double* J, double* K);
/* one fragment of the sweep.  h = fock + heff (n x n); dm0 n x n or NULL; eeval: also fragment energies.
 * outputs (any may be NULL): mo_coeff n*n, mo_energy n, rdm1_emb n*n (= C rdm1 C^T / 2, Frags._rdm1),
 * rdm1_mo n*n (Frags.rdm1__), t1 o*v, t2 o*o*v*v, e_frag[3] = [e1,e2,ec], scalars.  0 < nsocc <= n; nsocc == n (no virtual
 * orbitals) returns the mean-field results with E_corr = 0 and empty amplitudes, as PySCF's CCSD does.   */
int qemb_frag_solve(qemb_frag_t f, int nsocc, const double* h, const double* dm0, const qemb_solver_opts* opts,
                    int eeval, double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* t1,
                    double* t2, double* e_frag, double* e_corr_mo, double* e_scf, double* ebe_hf, int* n_iter,
                    int* scf_cycles);
/* Every fragment of a sweep in ONE call -- the "batched variant over a list of fragments per device" of the solver seam (the
 * reference's pool of workers, molbe/be_parallel.py:484-517).  Small fragments (octane BE2: six fragments of ~40 orbitals) are bound by the
 * NUMBER of dependent kernel launches, ~110 per CCSD iteration at 4-5 us each whatever the size: here the fragment RHF, the MO transformation
 * and the density / energy evaluation run per fragment on one stream each, and the CCSD iterations of all fragments run in lock step -- every
 * operation of the amplitude update is ONE grouped launch over all fragments still iterating.  Each fragment performs exactly the operations of
 * qemb_frag_solve in the same order: results are bit-identical.  Arguments are arrays over the fragments (pointer arrays and their entries may
 * be NULL where qemb_frag_solve allows NULL); e_frag is 3 * nfrag.  stats (nullable, 5 values): merged launch sequences run, launches they
 * issued, of which grouped, recorded operations they covered, largest number of fragments in one sequence.                               */
int qemb_frag_solve_batch(int nfrag, const qemb_frag_t* frags, const int* nsocc, const double* const* h, const double* const* dm0,
                          const qemb_solver_opts* opts, int eeval, double* const* mo_coeff, double* const* mo_energy,
                          double* const* rdm1_emb, double* const* rdm1_mo, double* const* t1, double* const* t2, double* e_frag,
                          double* e_corr_mo, double* e_scf, double* ebe_hf, int* n_iter, int* scf_cycles, int64_t* stats);
/* solver == "MP2" of be_func (molbe/solver.py:313-317, worker twin molbe/be_parallel.py:123-127): fragment RHF -> solve_mp2 (solver.py:781-826) ->
 * make_rdm1 (unrelaxed: oo and vv blocks) -> back-rotation -> get_frag_energy, density-fitted on the device: a fragment that holds its 3-index
 * factor needs only products with it (no ovvv / vvvv block, no iterations); one that holds only the 4-fold packed block goes through the four-index
 * transformation.  Of opts only scf_*, verbose and strict_convergence are read.  Outputs as qemb_frag_solve (there is no t1); t2 is o*o*v*v,
 * [i,j,a,b]; any may be NULL.  e_frag[1] is the cumulant two-body term (the dovov part of the MP2 2-RDM); nsocc == n gives the mean-field results. */
int qemb_frag_solve_mp2(qemb_frag_t f, int nsocc, const double* h, const double* dm0, const qemb_solver_opts* opts, int eeval,
                        double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* t2, double* e_frag,
                        double* e_corr_mo, double* e_scf, double* ebe_hf, int* scf_cycles);
/* ... for every fragment of a sweep in one call, spread over the execution contexts that exist (MP2 has no iterations to run in lock step): what
 * one-by-one calls return, bit for bit.  Arrays over the fragments as in qemb_frag_solve_batch; e_frag is 3 * nfrag.                             */
int qemb_frag_solve_mp2_batch(int nfrag, const qemb_frag_t* frags, const int* nsocc, const double* const* h, const double* const* dm0,
                              const qemb_solver_opts* opts, int eeval, double* const* mo_coeff, double* const* mo_energy,
                              double* const* rdm1_emb, double* const* rdm1_mo, double* const* t2, double* e_frag, double* e_corr_mo,
                              double* e_scf, double* ebe_hf, int* scf_cycles);
/* solver == "FCI" of be_func (molbe/solver.py:339-342, :507-547; the literal of this package is "FCI-hip"): fragment RHF -> `fci.FCI(mf, mo_coeff).kernel()` with
 * h1 = C^T (fock + heff) C, the fragment's ERIs in the fragment-MO basis, nelec = (nsocc, nsocc) and a zero constant -> make_rdm1 -> back-rotation -> get_frag_energy
 * with the cumulant of make_rdm2 (its mean-field part, solver.py:513-527, subtracted), in the determinant basis on the device: N_det = C(n, nsocc)^2 determinants
 * |Ia Ib> over the occupation strings of each spin in ascending order of their bit patterns, the vector c[Ia][Ib] row-major.  One application of H is two gather
 * passes around one FP64 product (pq|rs) D[rs, I] of shape n^2 x n^2 x N_det; the lowest state of the M_s = 0 space comes from a Davidson-Liu iteration started at
 * the determinant of lowest diagonal, converged on the residual ||H c - E c||_2 <= conv_tol.  No atomics anywhere: two calls return the same bits.
 * qemb_fci_opts: always start from qemb_default_fci_opts (conv_tol 1e-9, max_cycle 100 applications of H, max_space 12 basis vectors before the collapse to the
 *   Ritz vector, lindep 1e-14); NULL means these defaults; another struct_size is QEMB_ERR_ARG.  Of opts only scf_*, verbose and strict_convergence are read;
 *   non-convergence follows strict_convergence as for CCSD (QEMB_ERR_NOCONV, or results and QEMB_WARN_NOCONV).
 * Outputs as qemb_frag_solve; rdm1_mo is make_rdm1 (symmetrised), civec (nullable) ns * ns doubles: normalised, its largest-magnitude component positive;
 * e_fci the eigenvalue (e_fci - e_scf is the correlation energy of the embedding problem), n_iter the applications of H.  nsocc == n is a single determinant: the
 * mean-field results.
 * Limits: n > 16 is QEMB_ERR_UNSUPPORTED naming n.  Before anything is allocated the working set -- D and G (2 x 8 n^2 N_det bytes), (2 max_space + 4) vectors of
 * N_det, the tables and the n^4 pieces; qemb_frag_fci_bytes reports it -- is compared with min(free device memory, the limit of qemb_frag_fci_mem_limit):
 * QEMB_ERR_ALLOC naming n, nsocc and N_det.  Without slabs that is n <= 14 (7 alpha, 7 beta: 11.8 M determinants, 18.5 GB each for D and G); in slabs (15, 7) and
 * (16, 8) -- 165.6 M determinants -- run under a limit of 140 GB.
 * qemb_frag_fci_slab: D and G -- all but (2 max_space + 4) vectors of the working set -- in slabs of `rows` alpha strings (all beta strings: rows * ns determinant
 *   columns), one application of H and the RDM build walking the ceil(ns / rows) slabs in ascending order.  rows = 0 (the default): off, the path and the guard
 *   above, bit for bit.  rows = k > 0: the slab kernels with k rows (k >= ns: one slab); for one k two calls return the same bits, between different k and against
 *   rows = 0 the results agree to rounding.  rows = -1: unslabbed when that fits min(free, limit), else the largest rows that does.  Any other negative value:
 *   QEMB_ERR_ARG.  The guard of a slabbed solve compares qemb_frag_fci_bytes_slab (qemb_frag_fci_bytes with D and G at 2 x 8 n^2 min(rows, ns) ns bytes; rows = 0:
 *   the whole space) with the same room: QEMB_ERR_ALLOC naming n, nsocc, N_det, rows and the slab count.  qemb_frag_rdm2(QEMB_RDM2_FCI) follows the setting with
 *   its own limit.  qemb_frag_fci_slab_used: rows and slab count of the last FCI solve or FCI 2-RDM call of the fragment (unslabbed: rows 0, n_slab 1).
 * qemb_frag_fci_residual: ||H c - E c||_2 of the last FCI solve of the fragment. */
typedef struct {
  uint32_t struct_size;      /* sizeof(qemb_fci_opts); set by qemb_default_fci_opts, checked by every entry point that takes the struct */
  double conv_tol;           /* ||H c - E c||_2     default 1e-9  (PySCF: 1e-10 on the energy change) */
  int max_cycle;             /* applications of H   default 100 */
  int max_space;             /* basis vectors       default 12 */
  double lindep;             /*                     default 1e-14 */
} qemb_fci_opts;
void qemb_default_fci_opts(qemb_fci_opts* opts);
int qemb_frag_solve_fci(qemb_frag_t f, int nsocc, const double* h, const double* dm0, const qemb_solver_opts* opts, const qemb_fci_opts* fci_opts, int eeval,
                        double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* civec, double* e_frag, double* e_fci, double* e_scf,
                        double* ebe_hf, int* n_iter, int* scf_cycles);
int qemb_frag_fci_bytes(int n, int nsocc, int max_space, int64_t* bytes);
int qemb_frag_fci_mem_limit(qemb_frag_t f, int64_t bytes);
int qemb_frag_fci_slab(qemb_frag_t f, int64_t rows);
int qemb_frag_fci_bytes_slab(int n, int nsocc, int max_space, int64_t rows, int64_t* bytes);
int qemb_frag_fci_slab_used(qemb_frag_t f, int64_t* rows, int64_t* n_slab);
int qemb_frag_fci_residual(qemb_frag_t f, double* residual);
/* solver == "SCI-hip": the selected-CI branch of be_func (molbe/solver.py:412-462, SHCI_ArgsUser(hci_cutoff)) as a heat-bath selection on the device, for fragments
 * beyond the determinant-space limit of qemb_frag_solve_fci (n <= 64).  Fragment RHF, h1 and the ERIs in the fragment-MO basis as for FCI; then, from the HF
 * determinant: every determinant outside the space V that a single or double excitation connects to some i in V with |H_ai c_i| >= eps_var joins, with its
 * spin-swapped partner; the lowest eigenpair of H in the new V (CSR matrix over the sorted 2 x 64-bit keys, Davidson from the old vector padded with zeros, residual
 * <= conv_tol); stop when a round adds nothing.  Energy, vector and RDMs are those of the last diagonalisation; the perturbative correction is a call of its own (qemb_frag_sci_pt2).  The determinant set,
 * the matrix and the vector are the same bits on every call; the RDMs are accumulated with FP64 atomic adds and reproducible to rounding only.
 * qemb_sci_opts: always start from qemb_default_sci_opts (eps_var 1e-3, conv_tol 1e-9, max_cycle 100, max_space 12, max_round 30, max_det 2^20); NULL means these
 *   defaults; another struct_size or eps_var <= 0 is QEMB_ERR_ARG.  Reaching max_round before a round adds nothing, or a diagonalisation that misses conv_tol, is
 *   non-convergence and follows strict_convergence (QEMB_ERR_NOCONV, or results and QEMB_WARN_NOCONV).
 * Outputs as qemb_frag_solve_fci without the vector; e_sci the eigenvalue, n_iter the applications of H over all rounds.  nsocc == n is a single determinant.
 * Limits: n > 64 is QEMB_ERR_UNSUPPORTED naming the limit.  Before anything is allocated the part of the working set that max_det fixes (qemb_frag_sci_bytes: three
 * key lists and vectors, the candidate buffer of one slab, the Davidson vectors, row pointers, the n^4 pieces) is compared with min(free device memory, the limit of
 * qemb_frag_sci_mem_limit): QEMB_ERR_ALLOC naming n, eps_var and the bytes.  Each round the count is checked against max_det and the CSR arrays (12 bytes per stored
 * element, known once counted) against what is left: QEMB_ERR_ALLOC naming n, eps_var, the round, the count reached and the energy so far.
 * qemb_frag_sci_stats: determinants, rounds, stored matrix elements and ||H c - E c||_2 of the last SCI solve (each nullable).
 * qemb_frag_sci_dets: the final space, alpha[ndet], beta[ndet] (bit p = fragment MO p occupied, sorted by (alpha, beta)) and c[ndet] (each nullable).
 * qemb_frag_sci_pt2: the screened Epstein-Nesbet second-order correction of the last SCI solve of this fragment, from the determinants, the vector and e_sci it left
 *   on the device (h and V in the fragment-MO basis are formed again from the resident ERIs or factor and the kept orbitals):
 *     S_a = sum over i in V with |H_ai c_i| >= eps_pt of H_ai c_i,   e_pt2 = sum_a S_a^2 / (e_sci - H_aa),
 *   a over the n_ext determinants outside V with at least one passing product and their spin-swapped partners.  Denominators are not guarded.  After a converged
 *   solve eps_pt >= eps_var gives exactly 0 and n_ext = 0; eps_pt -> 0 gives the full second-order correction.  A diagnostic of the embedding problem: it enters no
 *   fragment or BE energy.  The externals are handled in ranges of the alpha word of at most max_ext determinants (batches: how many ranges), summed in ascending
 *   order: the same bits on every call with the same max_ext.  max_ext <= 0: the largest count that fits.  ms3: host wall time (ms) of the screen passes, the sorts /
 *   merges and the row passes.  Every output is nullable.  nsocc == n: zeros.
 *   Errors: eps_pt <= 0, no solve since the ERIs or orbitals were set, or a last solve that was not SCI: QEMB_ERR_ARG.  Before anything is allocated the working set
 *   (qemb_frag_sci_pt2_bytes: 40 bytes per external, the candidate buffer of the screen, the run starts, the n^4 pieces) is compared with min(free device memory, the
 *   limit of qemb_frag_sci_mem_limit): QEMB_ERR_ALLOC naming n, eps_pt and the bytes.  One alpha word with more than max_ext externals: QEMB_ERR_ALLOC naming n,
 *   eps_pt, max_ext and the count reached. */
typedef struct {
  uint32_t struct_size;      /* sizeof(qemb_sci_opts); set by qemb_default_sci_opts, checked by every entry point that takes the struct */
  double eps_var;            /* threshold on |H_ai c_i|   default 1e-3 (the reference's hci_cutoff) */
  double conv_tol;           /* ||H c - E c||_2           default 1e-9 */
  int max_cycle;             /* applications of H per diagonalisation   default 100 */
  int max_space;             /* basis vectors             default 12 */
  int max_round;             /* selection rounds          default 30 */
  int64_t max_det;           /* determinants              default 2^20 */
} qemb_sci_opts;
void qemb_default_sci_opts(qemb_sci_opts* opts);
int qemb_frag_solve_sci(qemb_frag_t f, int nsocc, const double* h, const double* dm0, const qemb_solver_opts* opts, const qemb_sci_opts* sci_opts, int eeval,
                        double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* e_frag, double* e_sci, double* e_scf,
                        double* ebe_hf, int* n_iter, int* scf_cycles);
int qemb_frag_sci_stats(qemb_frag_t f, int64_t* ndet, int* rounds, int64_t* nnz, double* residual);
int qemb_frag_sci_dets(qemb_frag_t f, uint64_t* alpha, uint64_t* beta, double* c);
int qemb_frag_sci_bytes(int n, int nsocc, int64_t max_det, int max_space, int64_t* bytes);
int qemb_frag_sci_mem_limit(qemb_frag_t f, int64_t bytes);
int qemb_frag_sci_pt2(qemb_frag_t f, double eps_pt, int64_t max_ext, double* e_pt2, int64_t* n_ext, int* batches, double* ms3);
int qemb_frag_sci_pt2_bytes(int n, int nsocc, int64_t ndet, int64_t max_ext, int64_t* bytes);
/* The fragment 2-RDM in the fragment-MO basis, Frags.rdm2__ (molbe/solver.py:528): out[n^4] (host, [p][q][r][s]) from what the LAST solve of this fragment
 * left on the device.  kind names that solve and must agree with it:
 *   QEMB_RDM2_CCSD  make_rdm2_urlx(t1, t2, with_dm1) of shared/external/ccsd_rdm.py:23-55 (unrelaxed), from the kept t1 / t2 of qemb_frag_solve[_batch];
 *   QEMB_RDM2_MP2   PySCF's mp2.make_rdm2 (unrelaxed; its ovov block is 2 (2 t2 - t2^T)), or its dovov part alone with with_dm1 = 0.  An MP2 solve keeps no
 *                   amplitudes: t2 is formed again from the resident orbitals and integrals (one product and one pass, small beside the n^4 tensor).
 * with_dm1 = 0: the ovov / vovo blocks only (the cumulant-like part get_frag_energy contracts); 1: plus the products of the correlation 1-RDM with the
 * HF determinant and the HF 2-RDM.  The tensor is assembled by one kernel that writes each of the n^4 elements once; 8 n^4 bytes of device memory are
 * needed beside the amplitudes (QEMB_ERR_ALLOC, with n in the message, when they are not free).  Relaxed (Lambda) 2-RDMs are not implemented: after a
 * solve with relax_density the call returns QEMB_ERR_UNSUPPORTED.  Without a preceding solve of that kind, or after new ERIs / another SCF: QEMB_ERR_ARG.
 *   QEMB_RDM2_FCI   make_rdm2 of the vector qemb_frag_solve_fci left on the device, in PySCF's convention dm2[p,q,r,s] = <p+ r+ s q> (E = sum h dm1 + 1/2 sum (pq|rs) dm2);
 *                   with_dm1 = 0: minus the mean-field part of solver.py:513-527, what rdm2__ holds with use_cumulant.  D is formed once more and multiplied with itself
 *                   (8 n^2 N_det bytes of work space beside two n^4 tensors).
 *   QEMB_RDM2_SCI   the same tensor of the selected vector qemb_frag_solve_sci left on the device with its determinants (24 bytes each; the matrix is not kept: its
 *                   pattern, 4 bytes per stored element, is formed again for the call), accumulated over the stored pairs with FP64 atomic adds. */
#define QEMB_RDM2_CCSD 0
#define QEMB_RDM2_MP2 1
#define QEMB_RDM2_FCI 2
#define QEMB_RDM2_SCI 3
int qemb_frag_rdm2(qemb_frag_t f, int kind, int with_dm1, double* out);
/* The device memory qemb_frag_rdm2 of THIS fragment may take: before anything is allocated the call compares 8 n^4 bytes plus its workspace (the 1-RDM; for MP2 the
 * three o^2 v^2 tensors and the integral work space of forming t2 again) with min(free device memory, bytes) and fails with QEMB_ERR_ALLOC and n in the message when
 * it does not fit.  bytes < 0 (default): the free device memory alone. */
int qemb_frag_rdm2_mem_limit(qemb_frag_t f, int64_t bytes);
/* The perturbative triples correction E_(T) of the last CCSD solve of this fragment, relaxed or not (only t1 and t2 are read), from the amplitudes it left on
 * the device, the orbital energies, and (ia|bc), (ia|jk), (ia|jb) formed again by the route the fragment takes (3-index factor or packed block).  Closed shell,
 * Fock = diag(mo_energy), chemists' notation, i j k m occupied, a b c f virtual:
 *     g[i,j,k,a,b,c] = sum_f (ia|fb) t2[k,j,c,f] - sum_m (ia|mj) t2[m,k,b,c]
 *     W = the sum of g over the six simultaneous permutations of the pairs (i,a), (j,b), (k,c);   V = W + t1[i,a] (jb|kc) + t1[j,b] (ia|kc) + t1[k,c] (ia|jb)
 *     E_(T) = 1/3 sum W r3(V) / D,   r3(X)_ijk = 4 X_ijk + X_jki + X_kij - 2 X_kji - 2 X_ikj - 2 X_jik,   D = e_i + e_j + e_k - e_a - e_b - e_c   (not guarded)
 *   It is the triples energy of the EMBEDDING problem of this fragment, a diagnostic of what CCSD leaves out: it is added to no fragment or BE energy, and a
 *   centre-projected BE-level (T) energy is not formed.  The virtual orbitals are cut into tiles of *tile (the largest of 16, 8, 4, 2, 1 whose six product
 *   buffers of 8 tile^3 o^3 bytes stay within 192 MiB and whose working set fits) and *n_tile_triples tile triples A >= B >= C are visited; per triple six batched
 *   FP64 MFMA products over K = v + o form g (particle and hole term) and one kernel the rest.  No atomics: the same bits on every call.  ms4: device time (ms) of the images, the
 *   products and the assembly, then host wall time of forming the integrals again.  Every output is nullable.  Fewer than two occupied or two virtual orbitals (no triples): 0.0, tile 0.
 *   Errors: no solve since the ERIs or orbitals were set, a last solve that was not CCSD, or amplitudes that were released since (qemb_frag_drop_amplitudes): QEMB_ERR_ARG.
 *   Before anything is allocated the working set with tile 1 (qemb_frag_ccsd_t_bytes) is compared with min(free device memory, the limit of
 *   qemb_frag_ccsd_t_mem_limit): QEMB_ERR_ALLOC naming n.
 * qemb_frag_ccsd_t_bytes: the device bytes of the call with that tile for nsocc occupied orbitals (0: as many as the last solve had): the larger of the integral transformation (its work
 *   buffers and every block it leaves) and of the three kept blocks with the two images (v^2 o + v o^2)(v + o), the six buffers, the partial sums and, beyond 20
 *   occupied orbitals, the scratch of the kernel.
 * qemb_frag_ccsd_t_mem_limit: the device bytes qemb_frag_ccsd_t of THIS fragment may take; bytes < 0 (default): the free device memory alone.
 * qemb_frag_drop_amplitudes: releases the t1 / t2 (and Lambda multipliers) this fragment keeps from its last CCSD solve -- 8 (o v + o^2 v^2) bytes each; the next
 *   solve starts from the MP2 guess, and qemb_frag_rdm2(QEMB_RDM2_CCSD) and qemb_frag_ccsd_t are refused until it has run. */
int qemb_frag_ccsd_t(qemb_frag_t f, double* e_t, int* tile, int64_t* n_tile_triples, double* ms4);
int qemb_frag_ccsd_t_bytes(qemb_frag_t f, int nsocc, int tile, int64_t* bytes);
int qemb_frag_ccsd_t_mem_limit(qemb_frag_t f, int64_t bytes);
int qemb_frag_drop_amplitudes(qemb_frag_t f);
/* The same tensor left ON THE DEVICE in out_dev (n^4 doubles from qemb_malloc): what the full-basis accumulation of BE.rdm12_fullbasis rotates (the guard
 * then counts the workspace of the call alone). */
int qemb_frag_rdm2_dev(qemb_frag_t f, int kind, int with_dm1, double* out_dev);
/* The guard of the full-basis 2-RDM (BE.rdm12_fullbasis, BE.compute_energy_full): need_bytes = the N^4 accumulator plus every workspace the call will
 * allocate, compared with min(free device memory, limit_bytes) (limit_bytes < 0: the free memory alone) BEFORE anything is allocated.  QEMB_ERR_ALLOC with
 * N (= nao) in the message when it does not fit. */
int qemb_rdm2_full_guard(int64_t nao, int64_t need_bytes, int64_t limit_bytes);
/* number of Lambda iterations of the last qemb_frag_solve with relax_density (0 otherwise) */
int qemb_frag_lambda_iters(qemb_frag_t f, int* n_iter);
/* fragment RHF only: get_scfObj(fock + heff, eri, nocc, dm0) of molbe/helper.py:73-151 as used by
 * Frags.scf(fs=True) at initialisation (mbe.py:1160).  J, K: of the converged density (nullable).        */
int qemb_frag_scf(qemb_frag_t f, int nsocc, const double* h, const double* dm0, const qemb_solver_opts* opts,
                  double* mo_coeff, double* mo_energy, double* J, double* K, double* e_scf, int* converged, int* cycles);
/* CPHF density response to npot one-body perturbations (npot x n x n) -> dPs (npot x n x n): the work inside
 * hfres_func / cphf_kernel_batch (shared/external/optqn.py:456-466, cphf_utils.py:55-81) that builds the
 * initial Jacobian of the quasi-Newton density matching.                                                 */
int qemb_frag_cphf(qemb_frag_t f, int nsocc, const double* h, const double* dm0, const qemb_solver_opts* opts,
                   const double* vpots, int npot, double* dPs);
/* stateless one-call form (host buffers in, host buffers out) */
int qemb_ccsd_solve(int n, int nsocc, int n_f, const double* h, const double* eri_s4, const double* dm0,
                    const qemb_solver_opts* opts, const double* h1, const double* veff0, double weight,
                    const int* centers, int ncenter, double* mo_coeff, double* mo_energy, double* t1, double* t2,
                    double* rdm1_emb, double* e_frag, double* e_corr_mo, int* n_iter);
/* ---------------------------------------------------------------- multi-GPU exchange -------------- */
/* One process per GPU; fragments are sharded over the ranks and the ONLY exchange of a sweep is one all-reduce of the residual buffer
 * [edge values, centre values, sum centre diag, e1, e2, ec, n_iter, failure flag] -- what be_func_parallel gets back from its pathos pool
 * as pickled result tuples (molbe/be_parallel.py:484-517) before solve_error reads Fobjs[j]._rdm1 (molbe/solver.py:683-778); SURVEY.md 8(e).
 * The communicator is RCCL (xGMI inside a node), created once per process on the device and stream of qemb_init, and needs no Python
 * package: qemb_comm_unique_id on ONE rank -> the 128 bytes travel to every rank out of band (file, socket, MPI_Bcast, a torch store...)
 * -> qemb_comm_init(rank, world, id) on every rank (collective).  Buffers are HOST buffers, reduced in place; every rank receives the
 * bit-identical result.  Without qemb_comm_init the process is a world of one: info reports (0, 1), all-reduce fails.                  */
#define QEMB_COMM_ID_BYTES 128
#define QEMB_COMM_SUM 0
#define QEMB_COMM_MAX 1
int qemb_comm_unique_id(void* id_out /* QEMB_COMM_ID_BYTES */);
int qemb_comm_init(int rank, int world, const void* id);
int qemb_comm_info(int* rank, int* world);
int qemb_comm_allreduce(double* host_buf, int64_t n, int op);
int qemb_comm_destroy(void);

/* ---------------------------------------------------------------- AO -> fragment ERI transforms -- */
/* Dense: replaces `ao2mo.incore.full(eri_, TA, compact=True)` of BE._eri_transform "in-core"
 * (molbe/mbe.py:1035-1039).  The AO tensor is uploaded once per system and stays resident.            */
typedef void* qemb_aoeri_t;
int qemb_aoeri_upload(int N, const double* eri, int sym /* 8, 4 or 1 */, qemb_aoeri_t* out);
int qemb_aoeri_free(qemb_aoeri_t ao);
/* TA: N x n (host).  Result 4-fold packed (npair(n) x npair(n)) to out_s4_host (nullable) and/or
 * straight into a fragment handle (nullable) -- the HDF5 dataset "f{I}" hand-off without the disk.     */
int qemb_ao2mo_dense(qemb_aoeri_t ao, const double* TA, int n, double* out_s4_host, qemb_frag_t frag);

/* Density fitted: replaces integral_direct_DF (molbe/eri_onthefly.py:45-145, "int-direct-DF") and the
 * transform_integral / transform_integral_cuda pair injected into _run_sparse_df_driver
 * (molbe/eri_sparse_DF.py:535-556, :677-678, :701-702; C++ _cpp/eri_sparse_DF.cpp:724-751).
 * qemb_df_create factors (P|Q) on the device (eri_onthefly.py:108); qemb_lpq_upload takes an existing
 * lower Cholesky factor instead (the `build_lowtri_PQ` seam / GPU_MatrixHandle, eri_sparse_DF.cpp:64-107). */
typedef void* qemb_df_t;
int qemb_df_create(int naux, const double* j2c, qemb_df_t* out);
int qemb_lpq_upload(const double* L_PQ, int naux, qemb_df_t* out);
int qemb_df_free(qemb_df_t df);
/* 3-index integrals: layout 0 = (N,N,naux) "pqL" as getints3c returns them (eri_onthefly.py:85),
 * 1 = (naux,N,N), 2 = (naux, npair(N)) unique pairs mu >= nu (SemiSparseSym3DTensor without screening) */
int qemb_df_set_ints(qemb_df_t df, int N, const double* ints, int layout);
/* The reference's SemiSparseSym3DTensor itself (_cpp/eri_sparse_DF.cpp:110-298), never expanded to the dense (P|mu nu):
 * unique_dense_data = the (naux x n_unique) column-major matrix of the reference (one aux vector per stored unique AO pair;
 * n_unique x naux when read row-major); exch_reachable_with_offsets (:260-279) in CSR form: the partners of AO mu are
 * reach_nu[reach_ptr[mu] .. reach_ptr[mu+1]) and reach_off[...] is the column of the pair's aux vector.  Device memory is
 * O(n_unique naux); both transforms below then run the screened algorithm on this storage.                            */
int qemb_df_set_ints_semisparse(qemb_df_t df, int N, int64_t n_unique, const double* unique_dense_data, const int64_t* reach_ptr,
                                const int32_t* reach_nu, const int64_t* reach_off);
int qemb_df_transform(qemb_df_t df, const double* TA, int n, double* out_s4_host, qemb_frag_t frag);
/* the same with the MO-coefficient screening of transform_integral(int_P_mu_nu, TA, S_abs, L_PQ, MO_coeff_epsilon)
 * (_cpp/eri_sparse_DF.cpp:739-751): (P|mu i) is kept only for mu with |S_abs TA|(mu,i) >= epsilon (get_AO_per_MO :443);
 * unstored (screened) AO pairs of the SemiSparseSym3DTensor are passed as zeros of the packed layout 2.              */
int qemb_df_transform_screened(qemb_df_t df, const double* TA, int n, const double* S_abs, double MO_coeff_epsilon,
                               double* out_s4_host, qemb_frag_t frag);
/* The same two transforms handing the FITTED FACTOR ALONE to the fragment (bb of eri_onthefly.py:141; the bb^T bb product of :143 is not formed): the
 * fragment then lives on it (qemb_frag_set_df_only semantics) -- the a4 transform without its 2 naux npair^2 flops and without the 8 npair^2 bytes.   */
int qemb_df_transform_factor(qemb_df_t df, const double* TA, int n, qemb_frag_t frag);
int qemb_df_transform_screened_factor(qemb_df_t df, const double* TA, int n, const double* S_abs, double MO_coeff_epsilon, qemb_frag_t frag);

/* Gamma-point periodic (CC-GDF) variant of the direct DF transform, kbe/eri_onthefly.py:48-241.
 * qemb_df_create_pbc: _j2c_cholesky_or_eig (:19-45) -- the periodic metric may be indefinite: Cholesky when it succeeds (*ischol = 1),
 *   otherwise the fit matrix V d^{-1/2} V^T over the eigenvalues d > 1e-14 (*ischol = 0); bb = L^{-1} b or bb = fit b (:222-227).
 * qemb_df_alloc_ints: zeroed fitted tensor (L|mu nu), real and imaginary part (`pqL_frag`, :152-155, held once at the AO level:
 *   TA^T [sum_G F (G|mu nu)] TA = sum_G F (TA^T (G|mu nu) TA), so the per-fragment transform of every plane-wave block is not needed).
 * qemb_df_add_pw_block: += sum_G F[L,G] (G|mu nu) for nG plane waves (:176-199); F = ft_ao(chgcell, Gv)^H as naux x nG (re, im),
 *   (G|mu nu) = ft_aopair * coulG^* as nG x N x N (re, im).
 * qemb_df_add_rs_block: rows [p0, p1) += the real-space block (aux_e2(auxcell) - aux_e2(chgcell), :85-103, :201-217) as (p1-p0) x N x N.
 * qemb_df_pw_imag_absmax: max |Im (L|mu nu)| -- zero for a +-G symmetric mesh; the host mirror reproduces the reference's
 *   `Imaginary part of ERI is larger than 1e-6` check (:231-236) from it.   qemb_df_pw_select: the tensor qemb_df_transform reads
 *   (0 = real part, 1 = imaginary part, 2 = their sum: Re / Im of bb^T bb follow from three real transforms).                      */
int qemb_df_create_pbc(int naux, const double* j2c, qemb_df_t* out, int* ischol);
int qemb_df_alloc_ints(qemb_df_t df, int N);
int qemb_df_add_pw_block(qemb_df_t df, int nG, const double* F_re, const double* F_im, const double* pw_re, const double* pw_im);
int qemb_df_add_rs_block(qemb_df_t df, int p0, int p1, const double* block);
int qemb_df_pw_imag_absmax(qemb_df_t df, double* out);
int qemb_df_pw_select(qemb_df_t df, int part);

/* k-point density fitting of the periodic driver: what kbe/pbe.py:529-565 (int_transform = "out-core-DF") hands to libdmet -- the k-point GDF tensor, one
 * complex block L^{ki,kj}[P,mu,nu] = (P | mu_ki* nu_kj) per k-point pair (un-normalised Bloch sums) -- stays on the device; a fragment with embedding orbitals
 * C^k = TA_k receives a REAL 3-index factor with nk * naux rows:
 *     M^q[P,pq] = sum_ki (C^ki)^H L^{ki,ki+q}[P] C^{ki+q},      (pq|rs) = nk^-3 sum_q sum_P Re( M^q[P,pq] conj(M^q[P,rs]) )
 *     rows nk^-3/2 Re M^q for a class q = -q;  (2 nk^-3)^1/2 Re M^q and (2 nk^-3)^1/2 Im M^q for the lower-numbered class of every pair (q, -q).
 * qemb_kdf_create: qclass[ki * nk + kj] = the class of kj - ki (the index of that k-point; the mesh has to close under differences: every row and column of the
 *   table a permutation of 0..nk-1), qconj[q] = the class of -q.  The memory of the resident blocks is compared with the free device memory first
 *   (QEMB_ERR_ALLOC with nk, naux, nao in the message).
 * qemb_kdf_set_pair: the block of the pair (ki, kj), naux x nao x nao interleaved complex128 on the host.  A pair whose class is the -q partner of a kept class
 *   may be omitted (it is accepted and not stored).
 * qemb_kdf_transform: TA_k = nk x nao x n interleaved complex128 (host).  factor_only != 0: the fragment lives on the factor (qemb_frag_set_df_only semantics);
 *   0: it receives the 4-fold packed block (the pair product of the factor) and the factor beside it, like qemb_df_transform.  out_s4_host (nullable): the block.
 *   A needed pair that was never set: QEMB_ERR_ARG naming the pair.  An embedding basis that is not time-reversal symmetric (M^q not symmetric in its two
 *   orbital indices beyond 1e-8 of its largest element, or Im M^q != 0 for q = -q): QEMB_ERR_NUMERIC with the deviation in the message.
 * qemb_kdf_guard: the memory check of create + transform on its own (n_kept classes kept, with_block: the packed block is formed too) against
 *   min(free device memory, limit_bytes) (limit_bytes < 0: the free memory alone); allocates nothing.                                                        */
typedef void* qemb_kdf_t;
int qemb_kdf_create(int nk, int naux, int nao, const int* qclass /* nk*nk */, const int* qconj /* nk */, qemb_kdf_t* out);
int qemb_kdf_set_pair(qemb_kdf_t kdf, int ki, int kj, const double* L_interleaved_host);
int qemb_kdf_transform(qemb_kdf_t kdf, const double* TA_k_interleaved /* nk*nao*n */, int n, double* out_s4_host /* or NULL */, qemb_frag_t frag, int factor_only);
int qemb_kdf_free(qemb_kdf_t kdf);
int qemb_kdf_guard(int nk, int naux, int nao, int n, int n_kept, int with_block, int64_t limit_bytes);
/* ---- DF integrals from the basis: (mu nu|P) and (P|Q) evaluated on the device (csrc/int3c.cpp, kernels csrc/int3c_ops.hip) ----
 * What the reference obtains from libcint (df.incore.aux_e2, auxmol.intor('int2c2e'): molbe/eri_onthefly.py:64-108, eri_sparse_DF.py:410-494).  Contracted,
 * real-spherical, orbital shells s p d, auxiliary shells s..g; normalisation and component order are those of the records.
 * qemb_int_basis_create: n_bf records of record_bytes each, one per CARTESIAN contracted function, shell after shell, the components of a shell in libcint
 *   order (x^l first) sharing centre, exponents and coefficients:
 *     struct { double ctr[3]; int lmn[3]; int nprim; double ex[8], co[8]; }      (co includes the normalisation; quemb_amd/integrals.py `_BF`)
 *   c2s: 245 doubles, the Cartesian -> spherical matrices of l = 0..4 one after the other, each ncart(l) x (2l+1) row-major.  The matrices of l = 0 and
 *   l = 1 must be the identity (p functions in x, y, z order, unit scale): the kernels do not apply them; anything else is QEMB_ERR_UNSUPPORTED.  A record that does not
 *   continue its shell, or l > 4: QEMB_ERR_UNSUPPORTED naming the function.  A basis is uploaded once and used for any number of calls.
 * qemb_int3c2e: layout 0 (N, N, naux), 1 (naux, N, N), 2 (naux, npair(N)) with mu >= nu, 3 (n_pairs, naux) for the n_pairs AO pairs (mu, nu) of `pairs`
 *   (host, 2 n_pairs indices; NULL with the other layouts).  out: host array, or a device pointer when out_on_device != 0 (no host copy is made).
 *   An orbital shell with l > 2: QEMB_ERR_UNSUPPORTED naming the shell.  Every element is stored once by one thread: the same bits run to run, and
 *   (mu nu|P) = (nu mu|P) exactly.
 * qemb_int2c2e: (P|Q), naux x naux; the lower triangle of shell pairs is computed and mirrored.
 * qemb_df_create_empty + qemb_df_set_ints_from_basis: a DF context filled in place -- (P|Q) is formed, factored and inverted on the device and
 *   (P|mu nu) is written by the kernels into the resident [naux][N][N] tensor; nothing of size naux N^2 exists on the host.  A context that had a
 *   metric or integrals gets new ones.  qemb_df_set_ints_semisparse_from_basis: the same for the semi-sparse storage of qemb_df_set_ints_semisparse;
 *   pairs (host, 2 n_unique indices) names the AO pair of every stored row, in offset order. */
typedef void* qemb_int_basis_t;
int qemb_int_basis_create(int n_bf, const void* bf_records, size_t record_bytes, const double* c2s, qemb_int_basis_t* out);
int qemb_int_basis_free(qemb_int_basis_t basis);
int qemb_int3c2e(qemb_int_basis_t basis, qemb_int_basis_t auxbasis, const int64_t* pairs, int64_t n_pairs, int layout, double* out, int out_on_device);
int qemb_int2c2e(qemb_int_basis_t auxbasis, double* out, int out_on_device);
int qemb_df_create_empty(qemb_df_t* out);
int qemb_df_set_ints_from_basis(qemb_df_t df, qemb_int_basis_t basis, qemb_int_basis_t auxbasis);
int qemb_df_set_ints_semisparse_from_basis(qemb_df_t df, qemb_int_basis_t basis, qemb_int_basis_t auxbasis, int64_t n_unique, const int64_t* pairs,
                                           const int64_t* reach_ptr, const int32_t* reach_nu, const int64_t* reach_off);
/* ---- the four-centre AO integrals (mu nu|la si) evaluated on the device from the basis (csrc/int4c.cpp, kernels csrc/int4c_ops.hip) ----
 * What the reference takes from mf._eri (libcint) on its "in-core" branch (molbe/mbe.py:1036).  Contracted, real-spherical, orbital shells s p d, the handles of
 * qemb_int_basis_create.  Only canonical shell quartets are evaluated; every element of the output is stored once, all images of an integral from one value:
 * the same bits run to run, and the 8 images of the full tensor are bit-identical.
 * qemb_int4c2e: sym = 8: 1-D npair (npair + 1) / 2 doubles, element ij (ij + 1) / 2 + kl for pair indices ij >= kl (PySCF's 8-fold form); sym = 4: [npair][npair];
 *   sym = 1: [N]^4.  Another sym: QEMB_ERR_ARG.  out: host array, or a device pointer when out_on_device != 0.  thresh > 0: Schwarz screening -- Q_ab = sqrt(max (ab|ab))
 *   per shell pair is evaluated on the device once per basis, a shell quartet with Q_ab Q_cd < thresh is stored as zeros; thresh = 0: nothing is skipped.
 *   An orbital shell with l > 2: QEMB_ERR_UNSUPPORTED naming the shell.  Before anything is allocated the work space (and the output, when the call allocates it)
 *   is compared with min(free device memory, the limit of qemb_int4c_mem_limit): QEMB_ERR_ALLOC with N in the message when it does not fit.
 * qemb_int4c_mem_limit: the device bytes the four-centre calls of THIS basis may take (bytes < 0, the default: the free device memory alone).
 * qemb_int4c_stats: the canonical shell quartets of the last fill of this basis and how many of them were screened (either pointer may be NULL).
 * qemb_aoeri_from_basis: the 4-fold packed integrals written by the kernels into a resident qemb_aoeri_t -- the operand of qemb_ao2mo_dense without an N^4 (or any)
 *   integral array on the host; the counterpart of qemb_df_set_ints_from_basis.  Same guard (output included) and refusals as qemb_int4c2e. */
int qemb_int4c2e(qemb_int_basis_t basis, int sym, double thresh, double* out, int out_on_device);
int qemb_int4c_mem_limit(qemb_int_basis_t basis, int64_t bytes);
int qemb_int4c_stats(qemb_int_basis_t basis, int64_t* n_quartets, int64_t* n_screened);
int qemb_aoeri_from_basis(qemb_int_basis_t basis, double thresh, qemb_aoeri_t* out);
/* ---- integral-direct J and K: the mean field of a basis whose N^4 integrals are never formed (csrc/int4c.cpp: int4c_jk_direct) ----
 * What PySCF's direct SCF does with mf._eri = None.  J[mu,nu] = sum (mu nu|la si) D[la,si], K[mu,la] = sum (mu nu|la si) D[nu,si] for a SYMMETRIC dm (N x N, row-major):
 * every canonical shell quartet is evaluated as in qemb_int4c2e and contracted with the density in the thread that evaluated it; nothing is stored.
 * J or K may be NULL (that matrix is not formed), not both.  dm, J, K: host arrays, or device pointers when io_on_device != 0.
 * The first call on a basis writes the pair stage and the Schwarz factors and keeps them on the device until qemb_int_basis_free; later calls (the SCF cycles)
 * issue the class launches and O(N^2) passes only.  Device memory: pair stage, lists and O(N^2) -- qemb_int_jk_direct_bytes reports it before anything is
 * allocated; the guard is that of qemb_int4c2e without an output term (qemb_int4c_mem_limit applies; QEMB_ERR_ALLOC with N in the message).
 * thresh > 0: a quartet is skipped when Q_ab Q_cd < thresh or Q_ab Q_cd dmax < thresh, dmax the largest |D| over the six shell blocks of dm the quartet reads;
 * thresh = 0 skips nothing; qemb_int4c_stats reports quartets and skipped quartets of the call.  thresh < 0, NULL dm, both outputs NULL: QEMB_ERR_ARG; an
 * orbital shell with l > 2: QEMB_ERR_UNSUPPORTED.
 * J and K are accumulated on one triangle with FP64 atomic adds and mirrored: symmetric to the bit, but -- unlike the stored forms of qemb_int4c2e -- the last
 * bits depend on the arrival order of the adds and may differ from run to run. */
int qemb_int_jk_direct(qemb_int_basis_t basis, const double* dm, double thresh, double* J, double* K, int io_on_device);
int qemb_int_jk_direct_bytes(qemb_int_basis_t basis, int64_t* bytes);
/* ---- integral-direct AO -> fragment transform: the "in-core" fragment integrals without the N^4 array (csrc/int4c.cpp: int4c_ao2mo_direct) ----
 * The 4-fold packed fragment integrals of qemb_ao2mo_dense, G_f[pq,rs] = sum TA_f[mu,p] TA_f[nu,q] TA_f[la,r] TA_f[si,s] (mu nu|la si), for nfrag fragments in ONE
 * pass over the integrals.  The canonical shell pairs are cut into slabs of at most tile_pairs AO pairs (whole shell pairs; a larger shell pair is a slab of its
 * own); for every pair of slabs the kernels of qemb_int4c2e write one tile of the 4-fold packed tensor and every fragment consumes it (two FP64 GEMMs) before the
 * next tile overwrites it.  Every unique integral is evaluated once; no buffer grows as N^4 or npair(N)^2: device memory is O(tile^2 + tile n^2 + sum_f npair(n_f)^2)
 * beside the pair stage of qemb_int_jk_direct, which is shared with that call (a basis that served one does not write it again).
 * TA[f]: N x n[f], host, row-major.  out_s4_host (NULL, or an array of nfrag host pointers, each nullable): npair(n[f])^2 doubles; frags (NULL, or nfrag handles,
 * each nullable): the block goes straight into the fragment, as with qemb_ao2mo_dense.  tile_pairs <= 0: chosen from the free device memory.
 * thresh > 0: a shell quartet with Q_ab Q_cd < thresh counts as zeros, as in qemb_int4c2e, and a whole tile is skipped when max Q over its rows times max Q over its
 * columns is below thresh; thresh = 0 skips nothing.  qemb_int4c_stats: canonical quartets and screened ones of the call (those of a skipped tile included);
 * qemb_int4c_tile_stats: tiles visited and tiles skipped (either pointer may be NULL).
 * Fixed loop order, no atomics: the result is bit-reproducible run to run and exactly symmetric (G[pq,rs] = G[rs,pq] to the bit).
 * qemb_ao2mo_direct_bytes: the device bytes of a call.  The same figure is compared with min(free device memory, the limit of qemb_int4c_mem_limit) before
 * anything is allocated: QEMB_ERR_ALLOC with N, the tile size and the bytes in the message.  thresh < 0, NULL TA, n[f] outside 1..N, a fragment handle of
 * another n: QEMB_ERR_ARG; an orbital shell with l > 2: QEMB_ERR_UNSUPPORTED naming the shell. */
int qemb_ao2mo_direct(qemb_int_basis_t basis, int nfrag, const double* const* TA, const int* n, double* const* out_s4_host, const qemb_frag_t* frags,
                      int64_t tile_pairs, double thresh);
int qemb_ao2mo_direct_bytes(qemb_int_basis_t basis, int nfrag, const int* n, int64_t tile_pairs, int64_t* bytes);
int qemb_int4c_tile_stats(qemb_int_basis_t basis, int64_t* n_visited, int64_t* n_skipped);

/* ---- Cholesky-decomposed AO integrals: a 3-index factor from the geometry with no auxiliary basis (csrc/int4c.cpp: int4c_cholesky; kernels csrc/cd_ops.hip) ----
 * Pivoted, incomplete Cholesky decomposition of the 4-fold packed tensor V[ij,kl] = (ij|kl) ~ sum_K L[K,ij] L[K,kl], blocked at shell-pair granularity and
 * entirely on the device.  |V - L^T L| <= tol element by element (on a positive semidefinite residual |R[ij,kl]| <= sqrt(R[ij,ij] R[kl,kl]) <= tol); only the
 * rank x npair integrals of the pivot columns are evaluated and nothing of size npair^2 exists.
 * tol > 0; span in (0, 1]: a panel takes the shell pairs whose largest residual diagonal exceeds max(span max d, tol), at most panel_pairs AO pairs (<= 0: 128; a
 * larger shell pair is a panel of its own); max_rank <= 0: what the memory the call may take allows, at most npair(N).
 * qemb_int_cholesky: out_packed_host (nullable): [rank][npair(N)] in canonical packed order (pair mu (mu + 1) / 2 + nu, mu >= nu), with room for max_rank rows
 *   (npair(N) rows when max_rank <= 0); *rank: the number of vectors.  Two calls give the same bits, on any execution context.
 * qemb_int_cholesky_bytes: the device bytes of a call (pair stage and lists, the diagonal, one panel npair x panel, the factor up to max_rank).  The same figure is
 *   compared with min(free device memory, the limit of qemb_int4c_mem_limit) before anything is allocated: QEMB_ERR_ALLOC with N in the message.
 * qemb_int_cholesky_stats: out4 = rank, panels, integral columns evaluated, the final largest residual diagonal of the last decomposition of this basis.
 * qemb_df_set_ints_from_cholesky: fills a context of qemb_df_create_empty with L as its [rank][N][N] tensor and an IDENTITY metric: no fit step, no rank x rank
 *   matrix; qemb_df_transform* skip the product with the inverse metric factor.
 * tol <= 0, span outside (0, 1]: QEMB_ERR_ARG; an orbital shell with l > 2: QEMB_ERR_UNSUPPORTED naming the shell; max_rank vectors with the largest residual diagonal
 * still above tol: QEMB_ERR_NOCONV, the message names N, the rank and that diagonal -- never a silently worse factor. */
int qemb_int_cholesky(qemb_int_basis_t basis, double tol, double span, int64_t panel_pairs, int64_t max_rank, double* out_packed_host, int64_t* rank);
int qemb_int_cholesky_bytes(qemb_int_basis_t basis, int64_t panel_pairs, int64_t max_rank, int64_t* bytes);
int qemb_int_cholesky_stats(qemb_int_basis_t basis, double* out4);
int qemb_df_set_ints_from_cholesky(qemb_df_t df, qemb_int_basis_t basis, double tol, double span, int64_t panel_pairs, int64_t max_rank);

/* ---- one-electron integrals of an uploaded basis on the device (csrc/int3c.cpp: int1e_fill; kernel csrc/int1e_ops.hip) ----
 * S (overlap), T (kinetic energy) and V = sum_C -Z_C <a|1/r_C|b> (nuclear attraction) of the contracted real-spherical functions of `basis`: normalisation, component
 * order and Cartesian -> spherical matrices are those of the uploaded records, i.e. of Mole.one_electron().  natm nuclei at xyz (3 natm doubles, Bohr) with charges Z.
 * S_out, T_out, V_out: host arrays, N x N row-major; a NULL one is not computed.  Only shell pairs A >= B are evaluated and every element is stored once with its
 * mirror image: the matrices are symmetric to the bit and two calls give the same bits (no atomics).  natm < 0, or V_out with natm > 0 and NULL xyz / Z: QEMB_ERR_ARG;
 * an orbital shell with l > 2: QEMB_ERR_UNSUPPORTED naming the shell and its l. */
int qemb_int1e(qemb_int_basis_t basis, int natm, const double* xyz, const double* Z, double* S_out, double* T_out, double* V_out);
/* ---- Edmiston-Ruedenberg localisation on factorised integrals (csrc/api.cpp, kernels csrc/loc_ops.hip) ----
 * Rotates the m columns of C (host, N x m row-major, orthonormal under the overlap) so that sum_i (ii|ii) = sum_P sum_i (B^P_ii)^2 is maximal, with B the 3-index factor of
 * the columns from the dense tensor of `df` (fitted: the metric applied; Cholesky: the vectors themselves) -- the quarter transforms of qemb_df_transform_factor, unpacked
 * on the device to the stack [naux][m][m], which the joint-diagonalisation sweeps of qemb_hip_ops.h take with K = naux.  The integrals are the factorised ones: exact to the factor's own
 * error.  U_host (m x m): the rotation, C_loc = C U.  *f_before / *f_after: the functional; *sweeps, *converged as for those sweeps.  The footprint -- stack, U,
 * workspace and the transform's buffers -- is checked against the limit set there and the free memory before anything is allocated (QEMB_ERR_ALLOC naming
 * K = naux and m).  A semi-sparse or periodic context, or m > 512 (the limit of the sweeps, named in the message): QEMB_ERR_UNSUPPORTED. */
int qemb_df_localize_er(qemb_df_t df, const double* C, int m, double stop_angle, int max_sweeps, double* U_host, int* sweeps, double* f_before, double* f_after, int* converged);

/* The dipole integrals <a|r - origin|b> of the same functions: out[3][N][N] (host; x, y, z), origin: 3 doubles (Bohr).  From the 1-D overlaps the overlap already
 * forms, one order up in the ket: <i|x - o|j> = s_{i,j+1} + (B_x - o) s_ij.  The same shell-pair ownership as qemb_int1e: every element is stored once with its
 * mirror image (symmetric to the bit, the same bits on every call).  An orbital shell with l > 2: QEMB_ERR_UNSUPPORTED, as there. */
int qemb_int1e_dipole(qemb_int_basis_t basis, const double* origin, double* out);

/* ---- J and K of the AO-level mean field from the resident dense 3-index tensor of a DF context (csrc/ao2mo.cpp: DfContext::jk) ----
 * With T = (P|mu nu) resident as [naux][N][N] and the inverse metric factor Linv (B = Linv T):  J[mu,nu] = sum_P B[P,mu nu] sum_{la si} B[P,la si] D[la,si],
 * K[mu,la] = sum_P sum_{nu si} B[P,mu nu] B[P,la si] D[nu,si].  The density enters K through a factor Cw (N x (npos + nneg), host, row-major): D = sum_k s_k c_k c_k^T,
 * the columns scaled by sqrt|w_k|, the npos columns with s_k = +1 first, then the nneg columns with s_k = -1 (an indefinite density is legal).  dm (N x N, host,
 * symmetric) feeds J; NULL: D is formed from Cw on the device.  J_out / K_out: host, N x N; either may be NULL, not both.  N must be the N of the context.
 *   J: rho = T D, c = Linv^T (Linv rho), J = sum_P c_P T_P: two passes over the tensor, 4 naux N^2 flop.
 *   K: per slab of occ_block columns of one sign Y[mu,P,k] = sum_nu T[P,mu,nu] Cw[nu,k], Z[mu] = Linv Y[mu], K +/-= Z Z^T over (P, k); 2 naux N k (2 N + naux) flop.
 *      The lower triangle is mirrored at the end: K is symmetric to the bit.
 * A context with an identity metric (qemb_df_set_ints_from_cholesky) skips both products with Linv.  occ_block <= 0: all columns if they fit, else the largest slab
 * (halving) that fits.  No atomics and a fixed slab order: the same bits from call to call at a given occ_block.
 * qemb_df_jk_bytes(ctx, ncol, occ_block, &bytes): 8 (f naux N kb + N ncol + (3 + s) N^2 + 3 naux), kb = occ_block > 0 ? min(occ_block, ncol) : ncol, f = 2 with a metric,
 *   1 with the identity; s N^2 doubles are the split-K slices the last product (K = naux kb) may leave in the GEMM's work space: s = 0 when naux kb < 1024 or
 *   t = ceil(N / 256)^2 >= 256, else min(ceil(768 / t), naux kb / 256) (0 when that is 1).  The other products of the call are never split.  qemb_df_jk compares its figure with min(free device memory, the limit of qemb_df_jk_mem_limit; < 0: none) before anything is allocated:
 *   QEMB_ERR_ALLOC with N, naux, the slab and the bytes in the message.
 * A semi-sparse context and a periodic one (planar re / im tensor: qemb_df_create_pbc + qemb_df_alloc_ints): QEMB_ERR_UNSUPPORTED naming the layout. */
int qemb_df_jk(qemb_df_t ctx, int N, const double* dm, const double* Cw, int npos, int nneg, int occ_block, double* J_out, double* K_out);
int qemb_df_jk_bytes(qemb_df_t ctx, int ncol, int occ_block, int64_t* bytes);
int qemb_df_jk_mem_limit(qemb_df_t ctx, int64_t bytes);

/* the resident 3-index factor of a fragment (qemb_frag_mo_route_used gives its naux), naux x npair(n) to the host; QEMB_ERR_ARG without one */
int qemb_frag_get_df_factor(qemb_frag_t f, double* B_host);

/* ---------------------------------------------------------------- Schmidt decomposition ---------- */
/* schmidt_decomposition(mo_coeff, nocc, AO_in_frag, thr_bath) -> (TA_lo_eo, n_f, n_b), molbe/pfrag.py:403-411.
 * lmo: N x nmo row-major; TA_lo_eo: caller buffer N x ld (ld >= n_f + n_b; 2*n_f always suffices).      */
int qemb_schmidt(const double* lmo, int N, int nmo, int nocc, const int64_t* frag_idx, int n_f, double thr,
                 double* TA_lo_eo, int ld, int* n_b, int* sweeps);
/* Same contract and (for the idempotent HF 1-RDM of pfrag.py:448-450) the same bath as qemb_schmidt, through the
 * rank-n_f invariant subspace spanned by D[env,frag]: O(N_env n_f nocc) instead of the O(N_env^3) eigenproblem.   */
int qemb_schmidt_subspace(const double* lmo, int N, int nmo, int nocc, const int64_t* frag_idx, int n_f, double thr,
                          double* TA_lo_eo, int ld, int* n_b, int* sweeps);
/* schmidt_decomp_svd(rdm, Frag_sites, thr_bath) -> TA, kbe/solver.py:9 (real part)                     */
int qemb_schmidt_svd(const double* rdm, int N, const int64_t* frag_idx, int n_f, double thr, double* TA, int ld,
                     int* n_b, int* sweeps);
/* Frags.get_nsocc (molbe/pfrag.py:208-239): Cproj = TA^T S C_occ (n x nocc) -> P (n x n, nullable),
 * nsocc, initial fragment MOs (n x n)                                                                  */
int qemb_nsocc_guess(const double* Cproj, int n, int nocc, double* P, int* nsocc, double* mo_coeffs);
/* ---------------------------------------------------------------- AO screening (semi-sparse DF) --- */
/* int |chi_a| |chi_b| of unnormalised uncontracted Cartesian Gaussians by Gauss-Hermite quadrature: the primitive stage of
 * approx_S_abs (molbe/eri_sparse_DF.py:733-865, :928-959; numba on the host in the reference).  nsh primitive shells (l <= 4, exponent,
 * centre xyz[3s..], first Cartesian function cart0[s], components in libcint order); roots / weights of the nroots-point rule;
 * out: ncart x ncart (host).  The contraction to |c|^T s |c| and the reachability lists are host logic (eri_sparse_DF.py).           */
int qemb_abs_overlap_prim(int nsh, const int* l, const double* ex, const double* xyz, const int64_t* cart0, int64_t ncart, int nroots,
                          const double* roots, const double* weights, double* out);
/* plain host-in/host-out matrix product on the device: C(MxN) = op(A) op(B) (convenience for TA = W @ TA_lo_eo) */
int qemb_matmul(int64_t M, int64_t N, int64_t K, const double* A, int transA, const double* B, int transB, double* C);

#ifdef __cplusplus
}
#endif
#endif /* QEMB_HIP_H */
