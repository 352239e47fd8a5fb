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
// one explicit block in the caller's shell order (qemb_op_int4c_class): out_host[((a * (2 lb + 1) + b) * (2 lc + 1) + c) * (2 ld + 1) + d]
int int4c_block(const int l[4], const BfRecord* const rec[4], const double* c2s_host, double* out_host);

}  // namespace qemb
