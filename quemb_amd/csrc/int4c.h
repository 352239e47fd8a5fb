// int4c.h -- the four-centre AO integrals (mu nu|lambda sigma) on the device from an uploaded basis (IntBasis, int3c.h): what Mole.eri_s1 obtains from the host
// library and the reference from libcint (mf._eri, the operand of the "in-core" branch, molbe/mbe.py:1036).  The driver sorts the shell pairs into the six pair
// classes, has the pair stage written once (dev_int4c_pairs) and issues one launch per canonical class of quartets (dev_int4c_class); the result goes straight
// to the form the consumer reads: 8-fold packed (rdm2_eri_dot, RHF), 4-fold packed (AoEri, the operand of ao2mo_dense) or the full [N]^4 tensor.
#pragma once
#include <cstdint>
#include <vector>
#include "int3c.h"
#include "int4c_core.h"

namespace qemb {

// device bytes the call allocates beside its output: pair stage, index lists, Schwarz factors
int64_t int4c_work_bytes(const IntBasis& orb);
// doubles of the output in form sym (8, 4 or 1); -1 for another sym
int64_t int4c_out_words(int64_t N, int sym);
// The guard of the stored forms, before anything is allocated: the work space, plus the output when the call allocates it, against min(free device memory,
// orb.int4c_mem_limit) -- the one guard of int4c.cpp (mem_guard), which the direct calls apply to their own figures.  QEMB_ERR_ALLOC with N in the message.  An orbital shell with l > 2: QEMB_ERR_UNSUPPORTED naming the shell.  who: the entry point, for the messages.
int int4c_guard(const IntBasis& orb, int sym, bool with_output, const char* who);
// (mu nu|la si) into out_dev in form sym.  thresh > 0: quartets with Q_ab Q_cd < thresh are stored as zeros (Q from the device, cached in the basis);
// orb.int4c_stats receives the canonical shell quartets and how many of them were screened.
int int4c_fill(IntBasis& orb, int sym, double thresh, double* out_dev);
// Integral-direct J[mu,nu] = sum (mu nu|la si) D[la,si] and K[mu,la] = sum (mu nu|la si) D[nu,si] for a symmetric D: every canonical quartet is evaluated and
// contracted in the thread that evaluated it (dev_int4c_jk_class); nothing of size N^4 exists.  The first call on a basis writes the pair stage and the Schwarz
// factors and keeps them with the lists on the device (orb.pair_cache); later calls issue the class launches and the O(N^2) passes only.  J or K may be null.
// thresh > 0 skips a quartet with Q_ab Q_cd < thresh or Q_ab Q_cd max|D| < thresh (max over the six shell blocks of D the quartet reads); orb.int4c_stats as
// for int4c_fill.  The sums are accumulated with FP64 atomic adds: J and K are symmetric to the bit but not bit-reproducible from run to run.
int64_t int4c_jk_bytes(const IntBasis& orb);      // device bytes of a call: pair stage, lists, Schwarz factors, the N x N matrices and the shell-block table
int int4c_jk_direct(IntBasis& orb, const double* dm, double thresh, double* J, double* K, int io_on_device);
// Integral-direct AO -> fragment transform: G_f[pq,rs] = sum P_f[ij,pq] (ij|kl) P_f[kl,rs] for every fragment f of the call in ONE pass over the integrals, with no
// array of size N^4 or npair^2.  The canonical shell pairs are cut into slabs of at most tile_pairs AO pairs (whole shell pairs; a larger shell pair is a slab of its
// own); for every pair of slabs R >= S the quartet stage writes the tile E_RS of the 4-fold packed tensor (the kTile form: every unique integral still evaluated once
// in total) and each fragment consumes it, T = E_RS P_S, A += P_R^T T (ao2mo_tile_accumulate; R = S weighted 1/2); at the end G = A + A^T.  Fixed loop order, no
// atomics: bit-reproducible.  tile_pairs <= 0: chosen from the free memory.  thresh > 0: quartets screened as in int4c_fill, and a tile with max Q_R max Q_S < thresh
// is skipped altogether.  orb.int4c_stats as for int4c_fill (the quartets of a skipped tile count as screened), orb.int4c_tiles: tiles visited, tiles skipped.
// Pair stage, lists and Schwarz factors are those of orb.pair_cache.  out[f]: npair(n_f)^2 doubles on the device, allocated here.
// bytes: the device footprint of a call -- compared with min(free memory, orb.int4c_mem_limit) before anything is allocated (QEMB_ERR_ALLOC).
int int4c_ao2mo_direct_bytes(const IntBasis& orb, int nfrag, const int* n, int64_t tile_pairs, int64_t* bytes);
int int4c_ao2mo_direct(IntBasis& orb, int nfrag, const double* const* TA_host, const int* n, int64_t tile_pairs, double thresh, std::vector<DBuf>& out);
// one explicit tile (qemb_op_int4c_tile): rows = the AO pairs of the shell pairs pairs_r[k] = (I, J), I >= J, in list order and inside a shell pair in increasing
// AO pair index; columns likewise from pairs_s.  The two lists are the same list or have no shell pair in common.  out_host[row * ncol + col].
int int4c_tile(IntBasis& orb, const int32_t* pairs_r, int64_t n_r, const int32_t* pairs_s, int64_t n_s, double thresh, double* out_host);
// Pivoted, incomplete Cholesky decomposition of the 4-fold packed AO integrals, V[ij,kl] = (ij|kl) ~ sum_K L[K,ij] L[K,kl], blocked at shell-pair granularity and
// entirely on the device: the residual diagonal d (kDiag form), then until max d <= tol a panel S of whole shell pairs whose largest d exceeds
// max(span max d, tol) (descending, ties by the lower index, at most panel_pairs AO pairs; a larger shell pair alone), its integral columns (all ij | kl in S)
// by the kTile form, the update with the vectors so far (ONE FP64 GEMM, K = rank), the pivoted factorisation of the panel's own block (dev_cd_panel_factor), the
// new vectors at every AO pair (dev_cd_new_rows) and the diagonal update (dev_cd_diag_update).  On a positive semidefinite residual |R[ij,kl]| <=
// sqrt(R[ij,ij] R[kl,kl]) <= tol at the end.  rank x npair integrals are evaluated instead of npair^2 / 2, nothing of size npair^2 exists.  Fixed orders and no
// atomics: the same bits on every run and execution context.
// The panel's columns are written by two fill_tile calls into ONE buffer with a common leading dimension: (all pairs but S) x S -- two sets without a pair in
// common -- and S x S, the same list on both sides; the restriction fill_tile documents is kept.
// panel_pairs <= 0: 128.  max_rank <= 0: what the memory the call may take allows, at most npair.  bytes: pair stage and lists, the diagonal, one panel
// (npair x panel), the panel's work space and the factor up to max_rank -- compared with min(free memory, orb.int4c_mem_limit) before anything is allocated
// (QEMB_ERR_ALLOC, N in the message).  tol <= 0 or span outside (0, 1]: QEMB_ERR_ARG.  max_rank vectors with max d still above tol: QEMB_ERR_NOCONV, the message
// names N, the rank and the remaining max d.  orb.cd_stats / cd_dmax: rank, panels, columns evaluated, the final max d.
// The factor leaves in canonical packed order (out_host, nullable: [rank][npair(N)], room for max_rank -- or npair -- rows) or as the [rank][N][N] tensor of a DF
// context with an identity metric (DfContext::begin_ints_identity: no fit step).
int int4c_cholesky_bytes(const IntBasis& orb, int64_t panel_pairs, int64_t max_rank, int64_t* bytes);
int int4c_cholesky(IntBasis& orb, double tol, double span, int64_t panel_pairs, int64_t max_rank, double* out_host, int64_t* rank);
int int4c_cholesky_to_df(IntBasis& orb, double tol, double span, int64_t panel_pairs, int64_t max_rank, DfContext& df);
// one explicit block in the caller's shell order (qemb_op_int4c_class): out_host[((a * (2 lb + 1) + b) * (2 lc + 1) + c) * (2 ld + 1) + d]
int int4c_block(const int l[4], const BfRecord* const rec[4], const double* c2s_host, double* out_host);

}  // namespace qemb
