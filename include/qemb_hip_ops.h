/* qemb_hip_ops.h -- device-pointer primitives, device timers and measurement / tuning hooks of libqemb_hip.so.
 *
 * NOT part of the product ABI (include/qemb_hip.h): these entry points exist so that the parity tests can compare every kernel the
 * drivers are composed of with NumPy (tests/test_gpu_ops.py), and so that bench.py / tools/ can time single kernels.  All pointers
 * are DEVICE pointers (qemb_malloc) unless stated.  The tuning setters (qemb_set_gemm_*) act on the CALLING HOST THREAD only -- a host
 * thread drives one execution context (HIP stream), so a setter can never change the GEMMs in flight on another stream.
 */
#ifndef QEMB_HIP_OPS_H
#define QEMB_HIP_OPS_H
#include "qemb_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* device-time laps measured with HIP events on the library stream (slot ids: see QEMB_TIMER_*) */
#define QEMB_TIMER_LADDER 0
#define QEMB_TIMER_RINGS 1
#define QEMB_TIMER_ITER 2
#define QEMB_TIMER_AO2MO 3
#define QEMB_TIMER_SCF 4
#define QEMB_TIMER_GEMM_ANY 5
#define QEMB_TIMER_SCHMIDT 6
#define QEMB_TIMER_DF 7
int qemb_timer_begin(int slot);
int qemb_timer_end(int slot);
int qemb_timer_read(int slot, double* total_ms, int64_t* count);
int qemb_timer_reset(int slot);
int qemb_alloc_stats(long long* n_driver_allocs, long long* n_driver_frees, double* ms_in_driver_calls, double* gb_allocated, int reset);   /* pool misses (real hipMalloc calls) and real hipFree calls since the last reset */
int qemb_gemm_flop_count(double* flops, int reset);   /* 2 M N K batch summed over every FP64 MFMA product issued since the last reset (executed flops of a region; measurement hook) */
int qemb_tape_cache_counters(int64_t* reused, int64_t* recorded, int reset);   /* lock-step sweeps: recorded amplitude updates kept from the last solve of a fragment / recorded anew, since the last reset (measurement hook) */
int qemb_ctx_timer_read(int ctx, int slot, double* total_ms, int64_t* count, int reset);   /* timers of an idle execution context */
int qemb_timer_live_events(int slot);      /* event pairs held by the calling context's slot (bounded by recycling)   */

/* ---------------------------------------------------------------- device-pointer primitives ---- */
/* (the kernels the drivers below are composed of; exported so the parity tests can hit each one)    */

/* C[b] = alpha*op(A[b])*op(B[b]) + beta*C[b] on v_mfma_f64_16x16x4_f64.
 * a_kcontig: A(m,k)=A[m*lda+k] else A[k*lda+m];  b_kcontig: B(k,n)=B[n*ldb+k] else B[k*ldb+n].      */
int qemb_op_gemm(int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t lda, int a_kcontig,
                 int64_t strideA, const double* B, int64_t ldb, int b_kcontig, int64_t strideB, double beta,
                 double* C, int64_t ldc, int64_t strideC, int64_t batch);
/* C = A B with the rows of A (stored K x M, i.e. !a_kcontig) read through the slab-aware loader: A(m,k) = A[k*lda + m + (m / a_slab) * a_slab_skip].  With
 * lda = a_slab = n and a_slab_skip = n^2 - n the rows (pair, q) of a stack of n x n slabs X[pair][k][q] form ONE tall operand: the last quarter transform
 * of the embedding -> MO transformation (C^T . slab for every pair, csrc/ccsd.cpp mo_transform) as a flat product on the tall tile.  cfg as qemb_set_gemm_config. */
int qemb_op_gemm_slab_rows(int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, int64_t a_slab, int64_t a_slab_skip, const double* B, int64_t ldb,
                           int b_kcontig, double* C, int64_t ldc, int cfg);
/* -1 = automatic tile choice; 0..99 force a tile configuration (calling host thread only); 2xx = the round-1 main loop of the same tiles
 * (A/B measurements); 3xx = diagnostic instantiations that stamp s_memtime (qemb_op_gemm_stamps); 4xx / 5xx / 6xx = ABLATION instantiations
 * that leave memory traffic out and return WRONG products by construction (tools/gemm_ablation.py) -- measurement aids, reachable through
 * this hook only, never selected by the dispatcher or by any driver.                                                                      */
int qemb_set_gemm_config(int cfg);
/* calibration: sustained v_mfma_f64_16x16x4_f64 rate of the chip, registers only (TFLOP/s)           */
int qemb_mfma_f64_peak(int iters, int blocks_per_cu, double* tflops);
int qemb_set_gemm_splitk(int enabled);    /* automatic split-K for few-tile / long-K products (default on) */
/* One product (device pointers) timed on its own, with the sustained shader clock of the launch: every workgroup records its
 * s_memtime ticks, clock_ghz = sum(ticks) / (256 CUs x time) -- the clock itself when one workgroup is resident per CU (tile configs
 * 13/15/23/25), a multiple of it otherwise.  Synchronises; a measuring aid for bench.py / tools, not part of the solver path.        */
int qemb_op_gemm_probe(int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, int a_kcontig, const double* B, int64_t ldb, int b_kcontig,
                       double* C, int64_t ldc, int cfg, int ksplit, double* ms, double* clock_ghz, int64_t* workgroups);
/* diagnostic tile configurations 313 / 315 / 304 (8-wave tiles, both operands K-contiguous): per-wave s_memtime sums of one launch, averaged over its
 * waves: out7 = [cycles in k-steps 0..2 of the tiles, from there to past the per-tile barrier, in the last k-step, kernel ms, wave entry -> end of the
 * main loop, wave entry -> exit, workgroups] (sums over the k-tiles of a wave) */
int qemb_op_gemm_stamps(int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, int cfg,
                        int ksplit, double* out7);
/* the tile configuration and split-K factor the CCSD driver picks for a product of `rows` packed pair rows by `cols` columns (pp-ladder,
 * tau-side dressing): introspection for tests and tools, no device call */
int qemb_pair_gemm_choice(int64_t rows, int64_t cols, int* cfg, int* ksplit);
/* the plans of the nine CCSD products whose split-K slabs the consumer adds up, for a fragment of o occupied and v virtual orbitals -- the plans the
 * solver sizes its slab buffers and launches from: out[9][6] = (M, N, K, cfg, ksplit, slabs) for Fvv', the two long-K T1 terms, ladder +/-, Xw +/-,
 * tau-side X +/-.  Introspection for tests and tools, no device call */
int qemb_ccsd_gemm_plans(int o, int v, int64_t* out);
/* the ring products of the CCSD update of a fragment of o occupied and v virtual orbitals: out[0] = 1 when the shape is in the replay regime (o^2 v^2 <= 2^22),
 * out[1] the tile id (-1: the dispatcher's choice), out[2] the K split (0: the dispatcher's), out[3] the bytes of split-K workspace that the parallel region of
 * the last two products takes inside a tape.  No device call */
int qemb_ccsd_ring_plan(int o, int v, int64_t* out);
int qemb_set_gemm_ksplit(int ksplit);      /* explicit split-K factor for qemb_op_gemm (0 = automatic) */
/* entry `index` (0, 1, ...) of the table of production tiles (csrc/gemm_tiles.h), in the table's order: its id, tile rows x cols, k-step, whether it runs
 * the MODE 1 main loop on 16-byte loads, whether id + 200 addresses its classic loop, and the id of its pp-ladder twin (-1: none).  QEMB_ERR_ARG past
 * the end.  Introspection for tests and tools, no device call */
int qemb_gemm_tile_table(int index, int* id, int* rows, int* cols, int* bk, int* mode1, int* has_classic, int* ladder_twin);
/* what the calling host thread's last FP64 MFMA product launched: the tile id, 16-byte (1) or 8-byte (0) operand loads, main loop (1 = MODE 1), K slices,
 * the super-block walk (0 0: m-tiles fastest) and wide_c = 1 when the epilogue stores every C matrix of the launch in 16-byte pairs (ldc and N even, C
 * 16-byte aligned; under split-K: of the workspace slabs).  The host-check library reports vec2 and wide_c of the descriptor and zeros for the rest */
int qemb_gemm_last_launch(int* cfg, int* vec2, int* mode, int* ksplit, int* sb_m, int* sb_n, int* wide_c);
/* out[sum ik*so[k]] = alpha*in[sum ik*si[k]] + beta*out[...], 0<=ik<dim[k], 4 dims                  */
int qemb_op_copy4(const int64_t dim[4], const double* in, const int64_t si[4], double* out,
                  const int64_t so[4], double alpha, double beta);
int qemb_op_outer4(const int64_t dim[4], const double* u, int64_t su0, int64_t su2, const double* v,
                   int64_t sv1, int64_t sv3, double* out, const int64_t so[4], double alpha, double beta);
int qemb_op_div_denom(double* x, int64_t d0, int64_t d1, int64_t d2, int64_t d3, const double* ea,
                      const double* eb, const double* ec, const double* ed);
/* (+/-) pair-packed pp-ladder helpers, P(x,y) = x(x+1)/2+y (x>=y), Q(x,y) = x(x-1)/2+y (x>y):
 * Vp[P(ab),P(cd)] = (ac|bd)+(ad|bc), Vm[Q(ab),Q(cd)] = (ac|bd)-(ad|bc) from the n^4 MO tensor (virtuals offset o);
 * Tp[P(ij),P(cd)] = w(tau_ijcd+tau_ijdc), w = 1/2 | 1/4 (c==d), Tm[Q(ij),Q(cd)] = (tau_ijcd-tau_ijdc)/2;
 * scatter: t2[ijab] += Rp+Rm, t2[ijba] += Rp-Rm, t2[jiab] += Rp-Rm, t2[jiba] += Rp+Rm                         */
int qemb_op_ladder_pack_vvvv(int64_t n, int64_t o, const double* M, double* Vp, int64_t ldp, double* Vm, int64_t ldm);
int qemb_op_ladder_pack_tau(int64_t o, int64_t v, const double* tau, double* Tp, int64_t ldp, double* Tm, int64_t ldm);
int qemb_op_ladder_scatter_pm(int64_t o, int64_t v, const double* Rp, int64_t ldp, const double* Rm, int64_t ldm, double* t2);
int qemb_op_dot(int64_t n, const double* x, const double* y, double* out_dev);
int qemb_op_absmax(int64_t n, const double* x, double* out_dev);
int qemb_op_gemv_rows(int64_t rows, int64_t cols, const double* T, int64_t ldt, const double* x, double* y,
                      double alpha, double beta);
int qemb_op_gemv_rows_batched(int64_t rows, int64_t cols, int64_t nbatch, const double* T, int64_t ldt, int64_t strideT,
                              const double* x, int64_t stridex, double* y, double alpha, double beta);
int qemb_op_contract_mid(int64_t outer, int64_t mid, int64_t inner, const double* T, const double* x,
                         double* Y, int64_t ldy, double alpha, double beta);
int qemb_op_unpack_s4(int64_t n, const double* s4, double* s1);
int qemb_op_pack_s4(int64_t n, const double* s1, double* s4);
int qemb_op_unpack_s8_to_s4(int64_t n, const double* s8, double* s4);
/* A[r][c] = A[c][r], r < c (completes a SYRK-style result computed on and below the diagonal) */
int qemb_op_mirror_lower(int64_t n, double* A, int64_t lda);
/* exchange matrix K[p,r] = sum (pq|rs) D[q,s] from the half-unpacked tensor H[P(p,q)][r][s] (scf.hf.dot_eri_dm's K at helper.py:64) */
int qemb_op_k_from_pairs(int64_t n, const double* H, const double* D, double* K);
/* the same K and the packed Coulomb vector Jp[P(p,q)] = sum_{r>=s} (pq|rs) Dp[P(r,s)] in ONE pass over the 4-fold packed block S4
 * (J and K of scf.hf.dot_eri_dm, helper.py:64); Dp = D + D^T off the diagonal, D on it, packed; Dp / Jp may be null; n <= 1024 */
int qemb_op_jk_from_packed(int64_t n, const double* S4, const double* D, const double* Dp, double* Jp, double* K);
/* (+/-) pair packing of the last two indices of in[rows][v][v] (Op: c >= d sums, Om: c > d differences; rows padded to ldp / ldm)
 * and the inverse scatter of packed pair ROWS: out[i,j,:] = Xp + Xm, out[j,i,:] = Xp - Xm */
int qemb_op_pack_pm_cols(int64_t rows, int64_t v, const double* in, double* Op, int64_t ldp, double* Om, int64_t ldm);
int qemb_op_scatter_pm_rows(int64_t o, int64_t ncols, const double* Xp, const double* Xm, double* out);
/* hole-hole ladder through packed pairs: the (+/-) packed images of W[k,l,i,j] (Ap[P(ij)][P(kl)] = W[klij] + W[klji], W[kkij] on k = l;
 * Am[Q(ij)][Q(kl)] = W[klij] - W[klji]) and the scatter of TWO pairs of packed result rows, p = Rp + f Hp (f = 2 on a = b), m = Rm + Hm,
 * assigned to (assign != 0) or accumulated into t2 */
int qemb_op_pack_w_pm(int64_t o, const double* W, double* Ap, int64_t lda_p, double* Am, int64_t lda_m);
int qemb_op_ladder_scatter_pm2(int64_t o, int64_t v, const double* Rp, int64_t ldp, const double* Rm, int64_t ldm, const double* Hp, const double* Hm,
                               int assign, double* t2);
int qemb_op_lincomb2(int64_t n, double a, const double* x, double b, const double* y, double beta, double* out);   /* out = a x + b y + beta out */
/* Single-pass kernels of the CCSD amplitude update (csrc/ccsd.cpp), device pointers:
 *   small_k_update: C[z][m][n] += alpha sum_k A[z][k][m] B[z][k][n]  (K = n_occ; batch strides sA / sB / sC, 0 shares an operand)
 *   ccsd_ph_layouts: from t2[o][o][v][v] and t1 in one pass T[k,c,j,b] = t2[k,j,c,b], Tp = t2[k,j,b,c], S = 2T - Tp,
 *                    Ut = S - 2 t1[j,c] t1[k,b], Tpt = Tp + 2 t1[j,c] t1[k,b] (all [o][v][o][v]) and Th[k,j,c,b] = 2 t2[k,j,b,c] - t2[k,j,c,b]
 *   ccsd_y_traces:  Y[a,c] = 2 sum_k ZC[k,k,a,c] - sum_k ZB[k,c,a,k]   (ZC [o][o][v][v], ZB [o][v][v][o])
 * and of the semi-sparse DF transform: gather_rows dst[r,:] = idx[r] >= 0 ? src[idx[r],:] : 0 (idx: int64 on the device), scale_rows x[r,:] *= s[r] */
int qemb_op_small_k_update(int64_t batch, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t sA, const double* B, int64_t sB, double* C, int64_t sC);
int qemb_op_ccsd_ph_layouts(int64_t o, int64_t v, const double* t2, const double* t1, double* T, double* Tp, double* S, double* Ut, double* Tpt, double* Th);
int qemb_op_ccsd_y_traces(int64_t o, int64_t v, const double* ZC, const double* ZB, double* Y);
/* One pass over ovvv for two products of the CCSD update (csrc/ccsd_ovvv_ops.hip), device pointers:
 *   ccsd_ph_layouts_ring: ccsd_ph_layouts writing Tp, S, Ut, Tpt alone (S[k,c,i,d] is Theta in the slab order of ovvv for amplitudes with t2[ikcd] = t2[kidc])
 *   ccsd_ovvv_slabs:   G > 0, the number of partial slabs ccsd_ovvv_pass writes for this shape; 0: a shape it refuses (n_occ > 32, or n_virt beyond its
 *                      register / LDS limits)
 *   ccsd_ovvv_pass:    ZB[k,c,a,i] = sum_d ovvv[k,c,a,d] t1[i,d] ([o][v][v][o]) and PA[g][i][a], G slabs [o][v] whose sum over g (in order) is
 *                      sum_{k,c,d} Thk[k,c,i,d] ovvv[k,c,a,d]; slab g holds the (k,c) pairs [g o v / G, (g + 1) o v / G).  The same bits on every call. */
int qemb_op_ccsd_ph_layouts_ring(int64_t o, int64_t v, const double* t2, const double* t1, double* Tp, double* S, double* Ut, double* Tpt);
int qemb_op_ccsd_ovvv_slabs(int64_t o, int64_t v);
int qemb_op_ccsd_ovvv_pass(int64_t o, int64_t v, const double* ovvv, const double* t1, const double* Thk, double* ZB, double* PA);
/* The t1-dependent parts of both ring intermediates of the CCSD update in one pass (csrc/ccsd_ring_prep_ops.hip), device pointers:
 *   ccsd_ring_prep:      W2[i,a,k,c] = W2base[i,a,k,c] + ZC[k,i,a,c] - sum_l t1[l,a] OC[k,i,l,c],
 *                        R[i,a,k,c] = P1[i,a,k,c] + W1base[i,a,k,c] + ZB[k,c,a,i] - sum_l t1[l,a] OB[k,i,l,c] - W2[i,a,k,c] / 2
 *                        (ZB [o][v][v][o] and ZC [o][o][v][v] are only read; OB[k,i,l,c] = ovoo[k,c,l,i], OC[k,i,l,c] = ovoo[l,c,k,i], [o][o][o][v]; the rest
 *                        [o][v][o][v]).  The same bits on every call; a shape outside n_occ <= 32, n_virt <= 4096 is an error.
 *   ccsd_u_update:       U[i,j,a,b] = (U[i,j,a,b] + Z[i,a,b,j]) - sum_k A[i,j,k,a] t1[k,b]: the rank-n_occ update of U ([o][o][v][v], in place) with its
 *                        transposed addend Z ([o][v][v][o]) in the same sweep; A: [o][o][o][v].  Same shape limits.
 *   ccsd_ring_prep_rule: 1 when a CCSD solver of this shape takes the pass (replay != 0: a fragment small enough to replay its recorded update), else 0;
 *                        QEMB_RING_PREP=0 / 1 forces it off / on wherever the shape allows */
int qemb_op_ccsd_ring_prep(int64_t o, int64_t v, const double* t1, const double* P1, const double* W1base, const double* W2base, const double* ZB, const double* ZC,
                           const double* OB, const double* OC, double* R, double* W2);
int qemb_op_ccsd_ring_prep_rule(int64_t o, int64_t v, int replay);
int qemb_op_ccsd_u_update(int64_t o, int64_t v, const double* A, const double* t1, const double* Z, double* U);
/* Fused passes of the CCSD amplitude update (csrc/ccsd.cpp update_amps), device pointers:
 *   copy4_two: qemb_op_copy4 with base (NULL: out) and a second output of the same pass, addressed like out: out2 = c2a in2 + c2b (value written to out)
 *   scatter_pm_rows_add / ccsd_y_traces_add: the plain ops with an addend laid out like the result
 *   pack_w_pm_sum: pack_w_pm of W[k,l,i,j] = Wt[i,j,k,l] + X[i,j,k,l] + At[j,i,k,l] + At[i,j,l,k], W never stored
 *   ccsd_finish_t2_rings: F[ijab] = U[ijab] + RS[iajb] - M[iajb] / 2 - M[ibja];  t2n[ijab] = t2n[jiba] = (t2n[ijab] + OV[ijab] + F[ijab] + F[jiba]) / D (i >= j);
 *                         t1n[ia] /= eo[i] - ev[a] (t1n may be NULL) */
int qemb_op_copy4_two(const int64_t dim[4], const double* in, const int64_t si[4], double* out, const int64_t so[4], double alpha, double beta, const double* base,
                      double* out2, const double* in2, double c2a, double c2b);
int qemb_op_scatter_pm_rows_add(int64_t o, int64_t ncols, const double* Xp, const double* Xm, double* out, const double* add);
int qemb_op_ccsd_y_traces_add(int64_t o, int64_t v, const double* ZC, const double* ZB, double* Y, const double* add);
int qemb_op_pack_w_pm_sum(int64_t o, const double* Wt, const double* X, const double* At, double* Ap, int64_t lda_p, double* Am, int64_t lda_m);
/*   ccsd_t1_assemble: t1n[i,a] = sum_c t1[i,c] Lvv[a,c] - sum_k Loo[k,i] t1[k,a] + sum_k (sum_c t1[i,c] Fov[k,c]) t1[k,a] + S[(ia),:] . Fov + Lph1[(ia),:] . t1 + sum_s PA[s] - sum_s PB[s]  (PA / PB: SA / SB slabs of o v doubles, strideA / strideB apart)
 *   gemv_rows_two: two independent matrix-vector passes in one launch;  ccsd_y_traces_slabs: Y = traces + scale * sum of S slabs of `add` */
int qemb_op_ccsd_t1_assemble(int64_t o, int64_t v, const double* t1, const double* Lvv, const double* Loo, const double* Fov, const double* S, const double* Lph1,
                             const double* PA, int SA, int64_t strideA, const double* PB, int SB, int64_t strideB, double* t1n);
int qemb_op_gemv_rows_two(int64_t rows1, int64_t cols1, const double* T1, int64_t ld1, const double* x1, double* y1, double a1, double b1,
                          int64_t rows2, int64_t cols2, const double* T2, int64_t ld2, const double* x2, double* y2, double a2, double b2);
int qemb_op_ccsd_y_traces_slabs(int64_t o, int64_t v, const double* ZC, const double* ZB, double* Y, const double* add, int S, int64_t stride, double scale);
int qemb_op_ccsd_finish_t2_rings(int64_t o, int64_t v, double* t2n, const double* U, const double* OV, const double* RS, const double* M, const double* eo, const double* ev, double* t1n);
/* The two single-launch ends of a CCSD iteration (csrc/ccsd.cpp post_issue / post_extrapolate), device pointers except where noted:
 *   diis_push: e = trial - prev, xcopy = trial (xcopy may be NULL), row[j] = <e, ys[j]> for j < m <= 8 with ys[self] == e; `ys` is a HOST array of
 *              m device pointers; the row goes to row_dev (device, m doubles) and row_host (HOST, m doubles: the wrapper waits for it)
 *   ccsd_extrapolate_energy: amp = sum_k coef[k] xs[k] over [t1 | t2] (coef: HOST, xs: HOST array of device pointers, nterms <= 8), tau = t2 + t1 (x) t1,
 *              *e_host = <L, tau> (HOST double; the wrapper waits) */
int qemb_op_diis_push(int64_t n, const double* trial, const double* prev, double* e, double* xcopy, int m, const double* const* ys, int self, double* row_dev, double* row_host);
int qemb_op_ccsd_extrapolate_energy(int64_t o, int64_t v, int nterms, const double* coef, const double* const* xs, double* amp, const double* L, double* tau, double* e_host);
int qemb_op_gather_rows(int64_t nrows, int64_t len, const int64_t* idx_dev, const double* src, int64_t ld, double* dst);
int qemb_op_scale_rows(int64_t nrows, int64_t len, double* x, const double* s);
/* pair-packed MO transformation helpers (half the flops of the four-index ao2mo.kernel call of PySCF's cc.ao2mo(), which
 * solve_ccsd reaches at molbe/solver.py:900): row gather x >= y; the same fused with the unpack of the pair column; block gathers
 * from the pair-first MO tensor Mp[P(p,q)][r][s] and from the 3/4-transformed tensor T[P(r,s)][c][x]; (+/-) ladder operands. */
int qemb_op_pack_pair_rows(int64_t n, int64_t ncols, const double* in, double* out);
int qemb_op_unpack_tril_pair_rows(int64_t nr, int64_t n, const double* in, double* full);
int qemb_op_extract_pf(int64_t n, const double* Mp, int64_t p0, int64_t q0, int64_t r0, int64_t s0, int64_t sp, int64_t sq,
                       int64_t sr, int64_t ss, double* out);
int qemb_op_extract_pf_t(int64_t n, const double* T, int64_t x0, int64_t r0, int64_t s0, int64_t c0, int64_t sx, int64_t sr,
                         int64_t ss, int64_t sc, double* out);
int qemb_op_ladder_pack_vvvv_pf(int64_t n, int64_t o, const double* Mp, double* Vp, int64_t ldp, double* Vm, int64_t ldm);
/* ... and the same gathers from the pair product S[P(p,q)][P(r,s)] (npair x npair, both triangles) without its pair-first image; T restricted to the
 * requested pairs (slab (r,s) at row r * ss + s); the pair columns of a packed factor as a dense operand; the pair product itself (out = bb^T bb). */
int qemb_op_extract_pf_t_compact(int64_t n, const double* T, int64_t x0, int64_t c0, int64_t sx, int64_t sr, int64_t ss, int64_t sc,
                                 double* out, int64_t slab);
int qemb_op_gather_pair_cols(int64_t rows, int64_t n, const double* in, int64_t r0, int64_t s0, int64_t sr, int64_t ss, double* out);
int qemb_op_extract_ps(int64_t n, const double* S, int64_t p0, int64_t q0, int64_t r0, int64_t s0, int64_t sp, int64_t sq,
                       int64_t sr, int64_t ss, double* out);
int qemb_op_extract_ps_packed(int64_t n, const double* S, int64_t p0, int64_t q0, int64_t r0, int64_t sp, int64_t sq, int64_t sr, double* out);
int qemb_op_unpack_pair_block(int64_t n, int64_t o, const double* S, double* Mv, int64_t ld);
int qemb_op_ladder_pack_vvvv_pf_ld(int64_t n, int64_t o, const double* Mp, int64_t ld, double* Vp, int64_t ldp, double* Vm, int64_t ldm);
int qemb_op_pack_pm_ovvv(int64_t o, int64_t v, const double* ovvv, double* Op, int64_t ldp, double* Om, int64_t ldm);
int qemb_op_df_pair_product(int64_t np, int64_t naux, const double* bb, double* out);
int qemb_op_unpack_tril_rows(int64_t rows, int64_t n, const double* packed, double* full);
int qemb_op_pack_tril_rows(int64_t rows, int64_t n, const double* full, double* packed);
int qemb_op_jacobi_eigh(int64_t n, double* A, double* w, double* V, int* sweeps);
/* The SCF cycle of a SMALL fragment in two fused launches (round 5; n <= qemb_op_scf_fused_max(), 80 on the device; reference: molbe/helper.py:73-151, PySCF scf.hf.kernel):
 * qemb_op_scf_fock_small: F = h + J - K/2, err = F D - D F, scal2 = [sum (h + F) o D, sum err^2] (device);
 * qemb_op_jacobi_eigh_in_basis: eigenproblem of F in the orthonormal basis Cp (NULL: as given) -- w ascending, C_out = Cp V, the same to C2_out (NULL or any buffer, Cp itself
 * allowed), dm_out (NULL or) 2 C_occ C_occ^T of the lowest nocc columns;  qemb_op_pack_density_sym: Dp[P(r,s)] = D[r,s] + D[s,r] (r > s), D[r,r]. */
int qemb_op_scf_fused_max(void);
int qemb_op_jacobi_eigh_in_basis(int64_t n, const double* F, const double* Cp, double* w, double* C_out, double* C2_out, int nocc, double* dm_out, double stop_below, int* sweeps);
int qemb_op_scf_fock_small(int64_t n, const double* h, const double* J, const double* K, const double* D, double* F, double* err, double* scal2);
int qemb_op_pack_density_sym(int64_t n, const double* D, double* Dp);
int qemb_op_jacobi_svd(int64_t m, int64_t n, double* G, double* s, double* U, double* V, int* sweeps);
int qemb_op_cholesky_lower(int64_t n, double* A);
int qemb_op_tri_inverse_lower(int64_t n, const double* L, double* Linv);


/* MP2 amplitudes in one pass (PySCF mp2.kernel, mp/mp2.py: t2 = (ia|jb) / e_ijab, E = sum t2 (2 (ia|jb) - (ib|ja))): from ovov[i,a,j,b] and the
 * orbital energies (all on the device) t2[i,j,a,b], G[i,a,j,b] = 2 t2[i,j,a,b] - t2[j,i,a,b] and the energy (host).  Outputs must not alias ovov. */
int qemb_op_mp2_amplitudes(int64_t o, int64_t v, const double* ovov, const double* eo, const double* ev, double* t2, double* G, double* e_host);

/* The fragment 2-RDM from amplitudes that are handed in (all pointers on the device): kind QEMB_RDM2_CCSD (t1 [o][v], t2 [o][o][v][v]) or QEMB_RDM2_MP2 (t2; t1 is
 * not read), dm1c = dm1 - 2 I_occ ([n][n]) or NULL for with_dm1 = 0, out [n]^4 with n = o + v.  Every element of out is written once.  Returns after the kernel. */
int qemb_op_rdm2_assemble(int kind, int64_t o, int64_t v, const double* t1, const double* t2, const double* dm1c, double* out);
/* E_(T) of qemb_frag_ccsd_t from handed-in DEVICE arrays: t1 [o][v], t2 [o][o][v][v], ovvv [o][v][v][v] = (ia|bc), ovoo [o][v][o][o] = (ia|jk),
 * ovov [o][v][o][v] = (ia|jb), eo [o], ev [v]; tile >= 1: the tile of the virtual orbitals (cut to v), forced.  *e_t: host.  o < 2 or v < 2 (no triples): 0.0 without a launch. */
int qemb_op_ccsd_t(int o, int v, const double* t1, const double* t2, const double* ovvv, const double* ovoo, const double* ovov, const double* eo, const double* ev, int tile, double* e_t);
/* The full-basis passes of BE.rdm12_fullbasis / compute_energy_full on [m]^4 tensors (device pointers; molbe/mbe.py:543-620, :781-789):
 *   rdm2_add_nc:     X[i,j,k,l] += alpha (g[i,j] g[k,l] - g[i,l] g[j,k] / 2), g m x m
 *   rdm2_symmetrize: X = (X + X^T) / 2 in place with X^T[p,q,r,s] = X[s,r,q,p]; g != NULL: plus the non-connected part of g
 *   rdm2_eri_dot:    *e_host = sum eri[pqrs] K[pqrs]; eri in the form sym = 1 ([m]^4), 4 ([npair][npair]) or 8 (npair(npair)), unpacked in the kernel;
 *                    two-stage reduction with a partition fixed by m (the same bits on every run) */
int qemb_op_rdm2_add_nc(int64_t m, const double* g, double alpha, double* X);
int qemb_op_rdm2_symmetrize(int64_t m, const double* g, double* X);
int qemb_op_rdm2_eri_dot(int64_t m, int sym, const double* eri, const double* K, double* e_host);

/* The three passes of the k-point DF transform on their own (device pointers; return after the kernel).  ld = nao rounded up to 16 doubles.
 *   kdf_split: z [rows][nao] interleaved complex128 -> planes [rows][re (ld) | im (ld)], zero beyond nao
 *   kdf_stack: ta [nk][nao][n] interleaved complex128 -> Cs [nk][2 ld][2 n] = [[C_re, C_im], [-C_im, C_re]] and Dk [nk][2 nao][2 n], rows (mu, re) = [C_re | -C_im], (mu, im) = [C_im | C_re]
 *   kdf_pack:  M [naux][2][n][n] -> F[P][pair(p,q)] = w Re M, F[naux + P][pair(p,q)] = w Im M (the latter when paired), rows ldf apart; out2_host = {largest component
 *              of M[P,p,q] - M[P,q,p] (not paired: and of Im M), largest |component| of M}                                                                     */
int qemb_op_kdf_split(int64_t rows, int64_t nao, const double* z, double* planes);
int qemb_op_kdf_stack(int64_t nk, int64_t nao, int64_t n, const double* ta, double* Cs, double* Dk);
int qemb_op_kdf_pack(int64_t naux, int64_t n, const double* M, int paired, double w, double* F, int64_t ldf, double* out2_host);

/* measurement hooks: set up SCF + integrals once, then run/timed single CCSD iterations                */
int qemb_frag_prepare_ccsd(qemb_frag_t f, int nsocc, const double* h, const double* dm0, const qemb_solver_opts* opts);
int qemb_frag_ccsd_iterate(qemb_frag_t f, int niter, double* e_corr, double* normt);
int qemb_frag_ccsd_reset(qemb_frag_t f);
/* copy one MO-integral block of the prepared CCSD problem to the host: "oooo" "ovoo" "ovov" "ovvv" "Vl" (= (ac|bd) at
 * [a,b,c,d]) "W1base" (= ovvo[k,c,a,i] at [i,a,k,c]) "W2base" (= oovv[k,i,a,c] at [i,a,k,c]) "eo" "ev" "Vp" "Vm" ((+/-) pair-packed ladder operands) "mo_coeff" (n x n)                     */
int qemb_frag_ccsd_export(qemb_frag_t f, const char* name, double* host, int64_t nelem);


/* DF integrals (csrc/int3c_ops.hip).  qemb_op_boys: out[i * (m_max + 1) + m] = F_m(x[i]) (device pointers, m_max <= 12).
 * qemb_op_int3c_class: one block (a b|P) of explicit shells -- bf_*: the record (qemb_int_basis_create) of the first Cartesian component of each shell,
 * la, lb <= 2, lP <= 4, c2s as qemb_int_basis_create; out_host[(a * (2 lb + 1) + b) * (2 lP + 1) + m] (all host pointers). */
int qemb_op_boys(int m_max, int64_t n, const double* x, double* out);
int qemb_op_int3c_class(int la, int lb, int lP, const void* bf_a, const void* bf_b, const void* bf_P, const double* c2s, double* out_host);
/* Four-centre AO integrals (csrc/int4c_ops.hip).  qemb_op_int4c_class: one block (a b|c d) of explicit orbital shells in ANY order of angular momenta (the kernels run
 * the canonical class l_a >= l_b, l_c >= l_d, bra pair class >= ket pair class; the block is put back into the caller's order) -- bf_*: the record of the first
 * Cartesian component of each shell, l <= 2, c2s as qemb_int_basis_create; out_host[((a * (2 lb + 1) + b) * (2 lc + 1) + c) * (2 ld + 1) + d] (all host pointers). */
int qemb_op_int4c_class(int la, int lb, int lc, int ld, const void* bf_a, const void* bf_b, const void* bf_c, const void* bf_d, const double* c2s, double* out_host);
/* One explicit tile of the 4-fold packed tensor as qemb_ao2mo_direct forms it (the kTile form of the class kernels).  basis: a handle of qemb_int_basis_create
 * (void*).  pairs_r / pairs_s: n_r / n_s canonical shell pairs (I, J), I >= J, two int32 each; the two lists are the same list or have no shell pair in common.
 * Rows: the AO pairs of the shell pairs of pairs_r in list order, inside a shell pair in increasing AO pair index; columns likewise from pairs_s.
 * out_host[row * n_cols + col] = (mu nu|la si), host.  thresh as qemb_int4c2e. */
int qemb_op_int4c_tile(void* basis, const int32_t* pairs_r, int64_t n_r, const int32_t* pairs_s, int64_t n_s, double thresh, double* out_host);
/* The kernels of the Cholesky decomposition of the AO integrals on their own (csrc/cd_ops.hip), host arrays in and out.
 * qemb_op_cd_panel_factor: pivoted, rank-revealing Cholesky of the symmetric positive semidefinite n x n block A by one workgroup: pivots by the largest remaining
 *   diagonal (ties: the lower column) until it is <= thr.  piv[j]: the pivot column of step j < *rank; T[j * n + c]: vector j at column c, so that
 *   A ~ sum_j T[j][:]^T T[j][:] with a residual diagonal <= thr (rows >= *rank of T are zero).  *in_lds (nullable): 1 when the block was held in LDS.
 * qemb_op_cd_diag_update: d[row] -= sum_{k < r} Lnew[k * np + row]^2 over np rows, the r rows pivrow[k] set to exactly 0 and negative residue clamped to 0; spmax[w]:
 *   the largest d of rows row0[w] .. row0[w] + cnt[w] - 1 (nsp shell pairs), *dmax their maximum.
 * qemb_op_cd_permute: out[k][ij] = L[k * npair + pos[ij]] (full = 0: [M][npair(N)]) or out[k][mu][nu] = L[k * npair + pos[pair(mu, nu)]] (full = 1: [M][N][N]).
 * qemb_op_df_get_ints: the dense [naux][N][N] tensor of a DF context (qemb_df_t as void*) to the host; *identity_metric (nullable): 1 for a context filled by
 *   qemb_df_set_ints_from_cholesky. */
int qemb_op_cd_panel_factor(int n, const double* A_host, double thr, double* T_host, int32_t* piv_host, int32_t* rank, int* in_lds);
int qemb_op_cd_diag_update(int64_t np, int r, const double* Lnew_host, const int32_t* pivrow_host, double* d_host, int64_t nsp, const int32_t* row0_host, const int32_t* cnt_host,
                           double* spmax_host, double* dmax_host);
int qemb_op_cd_permute(int64_t M, int64_t N, const double* L_host, const int32_t* pos_host, int full, double* out_host);
int qemb_op_df_get_ints(void* df, double* out_host, int* identity_metric);

/* ---- determinant-space FCI (csrc/fci.cpp, kernels csrc/fci_ops.hip): the two operations behind qemb_frag_solve_fci on handed-in data.  Determinants and strings as
 * in qemb_hip.h.  h_host: [n][n] (host); V_dev: [n^2][n^2] = (pq|rs), c_dev: N_det (device).
 * qemb_op_fci_sigma: sigma_dev = H c.   qemb_op_fci_rdm12: dm1_host [n][n] (symmetrised) and, when dm2_dev != NULL, dm2 (n^4, device); cumulant != 0: minus the
 * mean-field part with nsocc occupied orbitals.   qemb_op_fci_links: the link table of one spin, nsocc (n - nsocc + 1) x ns words (host, nullable: the counts only). */
int qemb_op_fci_sigma(int n, int nsocc, const double* h_host, const double* V_dev, const double* c_dev, double* sigma_dev);
int qemb_op_fci_rdm12(int n, int nsocc, const double* c_dev, int cumulant, double* dm1_host, double* dm2_dev);
/* measurement hook (tools/fci_bench.py): one untimed application of H, then one whose three steps are bracketed by device timers; ms3 = D gather, G = V D, sigma gather */
int qemb_op_fci_sigma_timed(int n, int nsocc, const double* h_host, const double* V_dev, const double* c_dev, double* sigma_dev, double* ms3);
/* the same two operations in slabs of `rows` > 0 alpha rows (qemb_frag_fci_slab; rows >= ns: one slab); ms3 nullable: the three steps timed, summed over the slabs */
int qemb_op_fci_sigma_slab(int n, int nsocc, const double* h_host, const double* V_dev, const double* c_dev, double* sigma_dev, int64_t rows, double* ms3);
int qemb_op_fci_rdm12_slab(int n, int nsocc, const double* c_dev, int cumulant, int64_t rows, double* dm1_host, double* dm2_dev);
int qemb_op_fci_links(int n, int nsocc, int64_t* ns, int* nlink, int32_t* strings_host, int32_t* links_host);
/* ---- selected CI (csrc/sci.cpp, kernels csrc/sci_ops.hip): the operations behind qemb_frag_solve_sci on handed-in data.  A space is ndet keys alpha[k], beta[k]
 * (64-bit occupation words, bit p = orbital p occupied) sorted by (alpha, beta); every array but V_dev ([n^2][n^2] = (pq|rs)) is a host array.
 * qemb_op_sci_screen: the determinants outside the space that pass |H_ai c_i| >= eps for some member i, spin partners included, sorted; slab / cap: determinants per
 *   pass and keys of the candidate buffer (0: the defaults); *njoined always, the keys when njoined <= max_out.
 * qemb_op_sci_pt2: the second-order correction of qemb_frag_sci_pt2 for a handed-in space, vector and e_var (max_ext <= 0: no bound; outputs nullable).
 * qemb_op_sci_merge: the space merged with sorted keys outside it, the vector padded with zeros (outputs: ndet + njoined).
 * qemb_op_sci_matrix: the CSR matrix of H over the space (both triangles, columns ascending, the diagonal included): *nnz and rowptr[ndet + 1] always, col / val when
 *   nnz <= max_nnz.   qemb_op_sci_spmv: y = H x.   qemb_op_sci_rdm12: dm1 [n][n] (symmetrised) and dm2 [n]^4 of the vector c; cumulant != 0: minus the mean-field part.
 * qemb_frag_sci_stage_ms: host wall time (ms) of the five stages of the fragment's last SCI solve: screen, sort / merge, matrix, Davidson, RDMs (tools/sci_bench.py). */
int qemb_op_sci_screen(int n, int nsocc, const double* h_host, const double* V_dev, int64_t ndet, const uint64_t* alpha, const uint64_t* beta, const double* c, double eps,
                       int64_t slab, int64_t cap, int64_t max_out, int64_t* njoined, uint64_t* out_alpha, uint64_t* out_beta);
int qemb_op_sci_pt2(int n, int nsocc, const double* h_host, const double* V_dev, int64_t ndet, const uint64_t* alpha, const uint64_t* beta, const double* c, double e_var, double eps_pt,
                    int64_t max_ext, int64_t slab, int64_t cap, double* e_pt2, int64_t* n_ext, int* batches);
int qemb_op_sci_merge(int64_t ndet, const uint64_t* alpha, const uint64_t* beta, const double* c, int64_t njoined, const uint64_t* jalpha, const uint64_t* jbeta,
                      uint64_t* out_alpha, uint64_t* out_beta, double* out_c);
int qemb_op_sci_matrix(int n, const double* h_host, const double* V_dev, int64_t ndet, const uint64_t* alpha, const uint64_t* beta, int64_t max_nnz, int64_t* nnz,
                       int64_t* rowptr, int32_t* col, double* val);
int qemb_op_sci_spmv(int n, const double* h_host, const double* V_dev, int64_t ndet, const uint64_t* alpha, const uint64_t* beta, const double* x, double* y);
int qemb_op_sci_rdm12(int n, int nsocc, const double* h_host, const double* V_dev, int64_t ndet, const uint64_t* alpha, const uint64_t* beta, const double* c, int cumulant,
                      double* dm1, double* dm2);
int qemb_frag_sci_stage_ms(qemb_frag_t f, double* ms5);

/* ---- orbital localisation (csrc/loc_ops.hip): joint diagonalisation of a stack of symmetric matrices by Jacobi sweeps -- Boys (K = 3 dipole matrices), Pipek-Mezey
 * (K = atoms) and Edmiston-Ruedenberg on a 3-index factor (K = naux) are this one problem.  Q_dev [K][m][m] and U_dev [m][m] are device pointers.  On return U is
 * orthogonal (started from the identity: the orbitals rotate as C U), Q^k = U^T Q^k U, and *f = sum_k sum_i (Q^k_ii)^2 is maximal over plane rotations.  A sweep is
 * the m - 1 rounds of the circle-method tournament; the pair (p, q) turns by 4 theta = atan2(2 sum_k a_k d_k, sum_k d_k^2 - sum_k a_k^2), a_k = Q^k_pq,
 * d_k = (Q^k_pp - Q^k_qq) / 2.  Stops after a sweep whose largest |theta| < stop_angle (*converged = 1) or after max_sweeps (max_sweeps = 0: nothing is rotated and
 * *f is that of the input).  m <= 1 or K = 0: U = 1.  m > 512 (the launch-per-round variant's limit, csrc/loc_core.h): QEMB_ERR_UNSUPPORTED naming it.  All sums run in one fixed order: two calls give the same bits.  Before anything is allocated the footprint
 * (qemb_op_joint_diag_bytes: 8 (K m^2 + 2 m^2) and the workspace) is checked against the limit of qemb_op_joint_diag_mem_limit (bytes < 0: none; calling host thread)
 * and the workspace against the free memory: QEMB_ERR_ALLOC naming K and m.  *in_lds (nullable) of _bytes: 1 when the one-workgroup variant (stack in LDS) serves. */
int qemb_op_joint_diag(int64_t K, int64_t m, double* Q_dev, double* U_dev, double stop_angle, int max_sweeps, int* sweeps, double* f, int* converged);
int qemb_op_joint_diag_bytes(int64_t K, int64_t m, int64_t* bytes, int* in_lds);
int qemb_op_joint_diag_mem_limit(int64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* QEMB_HIP_OPS_H */
