// sci.h -- heat-bath selected CI of one embedding problem on the device: the selected-CI branch of be_func (molbe/solver.py:412-462) without its external
// binary.  The rule (DESIGN.md §4 "Selected CI"): V0 = {HF determinant}; every determinant outside V that a single or double excitation connects to some i in V
// with |H_ai c_i| >= eps joins, together with its spin-swapped partner; the lowest eigenpair of H in the new V (Davidson from the old vector padded with
// zeros); stop when a round adds nothing.  Determinants are keys of two 64-bit occupation words kept sorted by (alpha, beta); H is a CSR matrix rebuilt each
// round.  Plain C++ over the dev_sci_* operations of dev_ops.h.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "fci.h"
#include "tensor_utils.h"

namespace qemb {

struct SciOptions {
  double eps_var = 1e-3;       // the threshold on |H_ai c_i| (the reference's hci_cutoff)
  double conv_tol = 1e-9;      // ||H c - E c||_2 of every diagonalisation
  int max_cycle = 100;         // applications of H per diagonalisation
  int max_space = 12;          // Davidson basis vectors before the collapse
  int max_round = 30;          // selection rounds
  int64_t max_det = (int64_t)1 << 20;
  double lindep = 1e-14;
};

// a sorted space with its vector, and the matrix over it (all on the device; keys: 2 N uint64, col: int32)
struct SciSpace { DBuf keys, c; int64_t N = 0; const uint64_t* k() const { return (const uint64_t*)keys.p; } };
struct SciMatrix {
  DBuf rowptr, col, val, hdiag; int64_t N = 0, nnz = 0;
  const int64_t* rp() const { return (const int64_t*)rowptr.p; }
  const int32_t* ci() const { return (const int32_t*)col.p; }
};
enum { SCI_T_SCREEN = 0, SCI_T_MERGE = 1, SCI_T_BUILD = 2, SCI_T_DAVIDSON = 3, SCI_T_RDM = 4, SCI_T_COUNT = 5 };
struct SciResult {
  double e = 0.0, residual = 0.0;
  int64_t ndet = 0, nnz = 0;
  int rounds = 0, n_apply = 0;
  bool converged = false;          // a round added nothing before max_round
  bool diag_converged = true;      // every diagonalisation met conv_tol
  double ms[SCI_T_COUNT] = {0, 0, 0, 0, 0};      // host wall time per stage, the device drained at each boundary
};

// single and double excitations of one determinant with nsocc electrons per spin in n orbitals; keys of the candidate buffer of one slab (a power of two that
// holds every excitation of one determinant and its partner); device bytes of a solve WITHOUT the CSR arrays, whose size is known only once a round has counted
// them: three key lists and vectors of max_det, the candidate buffer with its flags and offsets, the slab's lane counts, the Davidson basis with its images and
// four work vectors (residual, correction, diagonal, the kept vector), the row pointers and the n^4 pieces (V, the 2-RDM).  The CSR arrays (12 bytes per stored element) are checked against what is left each round.
int64_t sci_excitations(int n, int nsocc);
int64_t sci_candidate_capacity(int n, int nsocc);
int64_t sci_bytes(int n, int nsocc, int64_t max_det, int max_space);
constexpr int64_t kSciSlab = 4096;      // determinants screened per pass
// the bound on every double-excitation element: |(ai|bj) - (aj|bi)| <= 2 max |V| (V_dev [n^2][n^2], downloaded once)
int sci_double_bound(int n, const double* V_dev, double* bound);

// the determinants outside `V` that pass the rule for (V, c), partners included: sorted, unique, in `joined` (2 * njoined uint64).  slab / cap: determinants per
// pass and keys of the candidate buffer (0: kSciSlab and sci_candidate_capacity); stops early, with njoined > max_new, once more than max_new have joined.
// The slab follows the yield: after every pass the next one takes as many determinants as would fill 3/4 of the buffer at the rate just seen.  ms (nullable,
// SCI_T_COUNT slots): the evaluation passes are added to ms[SCI_T_SCREEN], the sorts, the unique / difference passes and the merges to ms[SCI_T_MERGE].
// alpha_lo / alpha_hi: only keys whose alpha word lies in [alpha_lo, alpha_hi] are emitted, a key and its partner each tested on its own -- the union over
// disjoint ranges is the unrestricted output, which the defaults give.
int sci_screen(int n, int nsocc, const double* h_dev, const double* V_dev, double dbl_bound, const SciSpace& V, double eps, int64_t slab, int64_t cap, int64_t max_new,
               DBuf& joined, int64_t* njoined, double* ms = nullptr, uint64_t alpha_lo = 0, uint64_t alpha_hi = ~(uint64_t)0);
// out = V merged with the sorted keys `joined` (none of them in V), the vector padded with zeros
int sci_merge(const SciSpace& V, const uint64_t* joined, int64_t njoined, SciSpace& out);
// the CSR matrix over the sorted keys (h_dev = V_dev = null: its row pointers and columns alone, 4 bytes per stored element); max_bytes >= 0: QEMB_ERR_ALLOC (message starting with `who`) when the arrays would take more
int sci_build(int n, const double* h_dev, const double* V_dev, const uint64_t* keys, int64_t N, int64_t max_bytes, const std::string& who, SciMatrix& H);
// lowest eigenpair of H from the start vector c (device, N, any norm > 0; a zero vector: QEMB_ERR_ARG) by fci_detail::davidson (fci.h) over the CSR product with
// H.hdiag as the preconditioner's diagonal; c receives the normalised vector (plain sum of c_I^2), largest-magnitude component positive
int sci_davidson(const SciMatrix& H, const SciOptions& opt, double* c, FciResult* res);
// dm1 (host, symmetrised) and dm2[p,q,r,s] = <p+ r+ s q> (n^4 doubles, device; may be null) of the vector over the stored pairs; o_cum >= 0: minus the mean-field part
int sci_rdm12(int n, const uint64_t* keys, int64_t N, const int64_t* rowptr, const int32_t* col, const double* c, int o_cum, double* dm1_host, double* dm2_dev);
// the round loop.  h_host [n][n], V_dev [n^2][n^2]; room: device bytes the CSR arrays may take (< 0: no check).  On QEMB_ERR_ALLOC / QEMB_ERR_NOCONV the message
// names n, eps, the round, the count reached and the energy so far.  Returns 0 with res->converged = false when max_round was reached.
int sci_solve(int n, int nsocc, const double* h_host, const double* V_dev, const SciOptions& opt, int64_t room, SciSpace& V, SciMatrix& H, SciResult* res);

// ---- the screened Epstein-Nesbet second-order correction of (V, c, e_var) (DESIGN.md §4 "Selected CI"):
//   S_a = sum over i in V with |H_ai c_i| >= eps_pt of H_ai c_i (a outside V; each product tested on its own),   E_PT2 = sum_{a in P} S_a^2 / (e_var - H_aa),
// P what sci_screen returns for (V, c, eps_pt), n_ext = |P|.  The denominators are not guarded.  One alpha-word range at a time, starting with every word: the
// screen at eps_pt with max_new = max_ext, the row pass (dev_sci_pt2_rows), a fixed-order sum.  A range in which more than max_ext determinants join is cut at
// the alpha word in the middle of the partial sorted list and both halves are done again; ranges run in ascending order and their sums are added in that order
// (*batches: the ranges that were summed).  A single alpha word with more than max_ext externals: QEMB_ERR_ALLOC naming n, eps_pt, max_ext and the count reached.
// ms (nullable, SCI_PT2_T_COUNT slots): host wall time of the screen passes, the sorts / merges and the row passes with their sums.
enum { SCI_PT2_T_SCREEN = 0, SCI_PT2_T_MERGE = 1, SCI_PT2_T_ROWS = 2, SCI_PT2_T_COUNT = 3 };
int sci_pt2(int n, int nsocc, const double* h_dev, const double* V_dev, double dbl_bound, const SciSpace& V, double e_var, double eps_pt, int64_t max_ext, int64_t slab, int64_t cap,
            double* e_pt2, int64_t* n_ext, int* batches, double* ms = nullptr);
// device bytes of one sci_pt2 call over ndet determinants beside the space itself: the joined list while it grows (two copies of max_ext + one slab's yield, and
// the slab's own new keys), the contributions, the candidate buffer with its flags and offsets, the slab's lane counts and the run starts
int64_t sci_pt2_bytes(int n, int nsocc, int64_t ndet, int64_t max_ext);
// the largest max_ext whose sci_pt2_bytes is at most `room` (< 1: not even one)
int64_t sci_pt2_max_ext(int n, int nsocc, int64_t ndet, int64_t room);
// the run starts of equal alpha of sorted keys (device): nseg + 1 offsets in segd, the last one N
int sci_alpha_runs(const uint64_t* keys, int64_t N, DBuf& segd, int64_t* nseg);

}  // namespace qemb
