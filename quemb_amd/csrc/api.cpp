// api.cpp -- extern "C" surface of libqemb_hip.so (declared in include/qemb_hip.h).
// Thin argument marshalling only; the work is in the drivers (ccsd.cpp, scf.cpp, ao2mo.cpp, schmidt.cpp)
// and the device layer (dev_ops.h).
#include <cstring>
#include <cstdlib>
#include <vector>
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
#include "../../include/qemb_hip_ops.h"
#include "dev_ops.h"
#include "ccsd.h"
#include "fragment.h"
#include "ao2mo.h"
#include "kdf.h"
#include "int3c.h"
#include "int4c.h"
#include "cd_core.h"
#include "loc_core.h"
#include "sci_core.h"
#include <algorithm>
#include <cmath>
#include <mutex>
#include <set>

using namespace qemb;
namespace qemb {
int dev_mfma_f64_peak(int iters, int blocks_per_cu, double* tflops);
int schmidt_eigh(const double* lmo, int N, int nmo, int nocc, const int64_t* frag, int n_f, double thr, double* TA_out,
                 int ld_out, int* n_b_out, int* sweeps_out);
int schmidt_subspace(const double* lmo, int N, int nmo, int nocc, const int64_t* frag, int n_f, double thr, double* TA_out,
                     int ld_out, int* n_b_out, int* sweeps_out);
int schmidt_svd(const double* rdm, int N, const int64_t* frag_in, int n_f, double thr, double* TA_out, int ld_out, int* n_b_out,
                int* sweeps_out);
int nsocc_guess(const double* Cproj, int n, int nocc, double* P_out, int* nsocc, double* mo_out);
}

static thread_local int g_test_ksplit = 0;   // qemb_set_gemm_ksplit: split-K override of qemb_op_gemm (tests / tuning), per calling thread
#ifdef QEMB_HOSTCHECK
// The host-check build has no dispatcher: qemb_gemm_last_launch reports the two launch properties that are pure functions of the descriptor, by the rules the
// real dispatcher uses (dev_ops.h), recorded where qemb_op_gemm builds the descriptor; no tile, loop or split is chosen there, so the rest stays zero
static thread_local GemmLaunchRecord g_hostcheck_last{};
#endif

extern "C" {

// QEMB_BACKTRACE=1: native frames to stderr on SIGSEGV / SIGABRT (a debugging aid: where inside the library did a host fault happen?)
static void qemb_fault_handler(int sig) {
  void* frames[64];
  const int nfr = backtrace(frames, 64);
  const char msg[] = "[qemb] fatal signal; native backtrace:\n";
  (void)!write(2, msg, sizeof(msg) - 1);
  backtrace_symbols_fd(frames, nfr, 2);
  signal(sig, SIG_DFL);
  raise(sig);
}
int qemb_init(int device) {
  static const bool bt = [] { if (env_flag("QEMB_BACKTRACE", false)) { signal(SIGSEGV, qemb_fault_handler); signal(SIGABRT, qemb_fault_handler); } return true; }();
  (void)bt;
  return dev_init(device);
}
const char* qemb_last_error(void) { return last_error(); }
const char* qemb_backend(void) { return dev_backend_name(); }
int qemb_sync(void) { return dev_sync(); }
int qemb_device_sync(void) { return dev_sync_device(); }
int qemb_mem_info(size_t* f, size_t* t) { return dev_mem_info(f, t); }
int qemb_malloc(void** p, size_t bytes) { return dev_alloc(p, bytes); }
int qemb_free(void* p) { return dev_free(p); }
int qemb_trim(void) { return dev_trim(); }
int qemb_trim_all(void) { return dev_trim_all(); }
int qemb_h2d(void* d, const void* h, size_t b) { return dev_h2d(d, h, b); }
int qemb_d2h(void* h, const void* d, size_t b) { return dev_d2h(h, d, b); }
int qemb_h2d_async(void* d, const void* h, size_t b) { return dev_h2d_async(d, h, b); }
int qemb_d2d(void* d, const void* s, size_t b) { return dev_d2d(d, s, b); }
int qemb_timer_begin(int s) { return dev_timer_begin(s); }
int qemb_timer_end(int s) { return dev_timer_end(s); }
int qemb_timer_read(int s, double* ms, int64_t* c) { return dev_timer_read(s, ms, c); }
int qemb_timer_reset(int s) { return dev_timer_reset(s); }
int qemb_timer_live_events(int s) { return dev_timer_live_events(s); }

int qemb_op_gemm(int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t lda, int a_kcontig,
                 int64_t strideA, const double* B, int64_t ldb, int b_kcontig, int64_t strideB, double beta,
                 double* C, int64_t ldc, int64_t strideC, int64_t batch) {
  GemmDesc g{M, N, K, alpha, beta, A, lda, a_kcontig, strideA, B, ldb, b_kcontig, strideB, C, ldc, strideC, batch, -1, g_test_ksplit};
#ifdef QEMB_HOSTCHECK
  g_hostcheck_last = GemmLaunchRecord{};
  g_hostcheck_last.vec2 = gemm_desc_vec2(g) ? 1 : 0;
  g_hostcheck_last.wide_c = gemm_wide_c(C, ldc, N, strideC, batch) ? 1 : 0;
#endif
  return dev_gemm(g);
}
int qemb_op_gemm_probe(int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, int a_kcontig, const double* B, int64_t ldb, int b_kcontig,
                       double* C, int64_t ldc, int cfg, int ksplit, double* ms, double* clock_ghz, int64_t* workgroups) {
  GemmDesc g{M, N, K, 1.0, 0.0, A, lda, a_kcontig, 0, B, ldb, b_kcontig, 0, C, ldc, 0, 1, cfg, ksplit};
  long long wg = 0;
  const int rc = dev_gemm_probe(g, ms, clock_ghz, &wg);
  if (workgroups) *workgroups = wg;
  return rc;
}
int qemb_op_gemm_stamps(int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, int cfg, int ksplit,
                        double* out7) {
  GemmDesc g{M, N, K, 1.0, 0.0, A, lda, 1, 0, B, ldb, 1, 0, C, ldc, 0, 1, cfg, ksplit};
  return dev_gemm_stamps(g, 8, out7);
}
int qemb_gemm_tile_table(int index, int* id, int* rows, int* cols, int* bk, int* mode1, int* has_classic, int* ladder_twin) {
  GemmTileEntry e;
  if (!gemm_tile_entry(index, &e)) { set_error("qemb_gemm_tile_table: index past the end of the table"); return QEMB_ERR_ARG; }
  if (id) *id = e.id;
  if (rows) *rows = e.rows;
  if (cols) *cols = e.cols;
  if (bk) *bk = e.bk;
  if (mode1) *mode1 = e.mode1;
  if (has_classic) *has_classic = e.has_classic;
  if (ladder_twin) *ladder_twin = e.ladder_twin;
  return QEMB_OK;
}
int qemb_gemm_last_launch(int* cfg, int* vec2, int* mode, int* ksplit, int* sb_m, int* sb_n, int* wide_c) {
#ifdef QEMB_HOSTCHECK
  const GemmLaunchRecord r = g_hostcheck_last;
#else
  GemmLaunchRecord r;
  dev_gemm_last_launch(&r);
#endif
  if (cfg) *cfg = r.cfg;
  if (vec2) *vec2 = r.vec2;
  if (mode) *mode = r.mode;
  if (ksplit) *ksplit = r.ksplit;
  if (sb_m) *sb_m = r.sb_m;
  if (sb_n) *sb_n = r.sb_n;
  if (wide_c) *wide_c = r.wide_c;
  return QEMB_OK;
}
int qemb_set_gemm_ksplit(int ks) { g_test_ksplit = ks; return QEMB_OK; }
int qemb_set_gemm_config(int cfg) { dev_gemm_set_force_cfg(cfg); return QEMB_OK; }
#ifndef QEMB_HOSTCHECK
int qemb_mfma_f64_peak(int iters, int blocks_per_cu, double* tflops) { return dev_mfma_f64_peak(iters, blocks_per_cu, tflops); }
#else
int qemb_mfma_f64_peak(int, int, double*) { set_error("not available in the hostcheck build"); return QEMB_ERR_DEVICE; }
#endif
int qemb_pair_gemm_choice(int64_t rows, int64_t cols, int* cfg, int* ksplit) {
  const GemmPlan p = pick_pair_gemm(rows, cols);
  if (cfg) *cfg = p.cfg;
  if (ksplit) *ksplit = p.ks;
  return QEMB_OK;
}
int qemb_ccsd_gemm_plans(int o, int v, int64_t* out) {
  if (o < 1 || v < 0 || !out) { set_error("qemb_ccsd_gemm_plans: bad arguments"); return QEMB_ERR_ARG; }
  const CcsdGemmPlans p = ccsd_gemm_plans(o, v);
  for (const GemmPlan* g : {&p.fvv, &p.pa, &p.pb, &p.ladder_p, &p.ladder_m, &p.xw_p, &p.xw_m, &p.x_p, &p.x_m})
    for (const int64_t x : {g->M, g->N, g->K, (int64_t)g->cfg, (int64_t)g->ks, (int64_t)g->S}) *out++ = x;
  return QEMB_OK;
}
int qemb_ccsd_ring_plan(int o, int v, int64_t* out) {
  if (o < 1 || v < 0 || !out) { set_error("qemb_ccsd_ring_plan: bad arguments"); return QEMB_ERR_ARG; }
  const CcsdRingPlan r = ccsd_ring_plan(o, v);
  out[0] = ((int64_t)o * o * v * v <= (int64_t)1 << 22) ? 1 : 0; out[1] = r.cfg; out[2] = r.ks; out[3] = r.region_ws_bytes;
  return QEMB_OK;
}
int qemb_set_gemm_splitk(int enabled) { dev_gemm_set_auto_splitk(enabled); return QEMB_OK; }
int qemb_op_copy4(const int64_t dim[4], const double* in, const int64_t si[4], double* out, const int64_t so[4],
                  double alpha, double beta) {
  Copy4Desc c{};
  for (int k = 0; k < 4; ++k) { c.dim[k] = dim[k]; c.si[k] = si[k]; c.so[k] = so[k]; }
  c.in = in; c.out = out; c.alpha = alpha; c.beta = beta;
  return dev_copy4(c);
}
int qemb_op_outer4(const int64_t dim[4], const double* u, int64_t su0, int64_t su2, const double* v, int64_t sv1,
                   int64_t sv3, double* out, const int64_t so[4], double alpha, double beta) {
  Outer4Desc o{};
  for (int k = 0; k < 4; ++k) { o.dim[k] = dim[k]; o.so[k] = so[k]; }
  o.u = u; o.su0 = su0; o.su2 = su2; o.v = v; o.sv1 = sv1; o.sv3 = sv3; o.out = out; o.alpha = alpha; o.beta = beta;
  return dev_outer4(o);
}
int qemb_op_div_denom(double* x, int64_t d0, int64_t d1, int64_t d2, int64_t d3, const double* ea, const double* eb,
                      const double* ec, const double* ed) { return dev_div_denom(x, d0, d1, d2, d3, ea, eb, ec, ed); }
int qemb_op_ladder_pack_vvvv(int64_t n, int64_t o, const double* M, double* Vp, int64_t ldp, double* Vm, int64_t ldm) { return dev_ladder_pack_vvvv(n, o, M, Vp, ldp, Vm, ldm); }
int qemb_op_ladder_pack_tau(int64_t o, int64_t v, const double* tau, double* Tp, int64_t ldp, double* Tm, int64_t ldm) { return dev_ladder_pack_tau(o, v, tau, Tp, ldp, Tm, ldm); }
int qemb_op_ladder_scatter_pm(int64_t o, int64_t v, const double* Rp, int64_t ldp, const double* Rm, int64_t ldm, double* t2) { return dev_ladder_scatter_pm(o, v, Rp, ldp, Rm, ldm, t2); }
int qemb_op_dot(int64_t n, const double* x, const double* y, double* o) { return dev_dot(n, x, y, o); }
int qemb_op_absmax(int64_t n, const double* x, double* o) { return dev_absmax(n, x, o); }
int qemb_op_gemv_rows(int64_t rows, int64_t cols, const double* T, int64_t ldt, const double* x, double* y, double alpha,
                      double beta) { return dev_gemv_rows(rows, cols, T, ldt, x, y, alpha, beta); }
int qemb_op_gemv_rows_batched(int64_t rows, int64_t cols, int64_t nbatch, const double* T, int64_t ldt, int64_t strideT, const double* x,
                              int64_t stridex, double* y, double alpha, double beta) { return dev_gemv_rows_batched(rows, cols, nbatch, T, ldt, strideT, x, stridex, y, alpha, beta); }
int qemb_op_contract_mid(int64_t outer, int64_t mid, int64_t inner, const double* T, const double* x, double* Y,
                         int64_t ldy, double alpha, double beta) { return dev_contract_mid(outer, mid, inner, T, x, Y, ldy, alpha, beta); }
int qemb_op_unpack_s4(int64_t n, const double* s4, double* s1) { return dev_unpack_s4(n, s4, s1); }
int qemb_op_pack_s4(int64_t n, const double* s1, double* s4) { return dev_pack_s4(n, s1, s4); }
int qemb_op_unpack_s8_to_s4(int64_t n, const double* s8, double* s4) { return dev_unpack_s8_to_s4(n, s8, s4); }
int qemb_comm_unique_id(void* id) { return dev_comm_unique_id(id); }
int qemb_comm_init(int rank, int world, const void* id) { return dev_comm_init(rank, world, id); }
int qemb_comm_info(int* rank, int* world) { return dev_comm_info(rank, world); }
int qemb_comm_allreduce(double* buf, int64_t n, int op) { return dev_comm_allreduce(buf, n, op); }
int qemb_comm_destroy(void) { return dev_comm_destroy(); }
int qemb_ctx_count(int n) { return dev_ctx_count(n); }
int qemb_ctx_bind(int k) { return dev_ctx_bind(k); }
int qemb_ctx_partition(int parts) { return dev_ctx_partition(parts); }
int qemb_op_gemm_slab_rows(int64_t M, int64_t N, int64_t K, const double* A, int64_t lda, int64_t a_slab, int64_t a_slab_skip, const double* B, int64_t ldb,
                           int b_kcontig, double* C, int64_t ldc, int cfg) {
  GemmDesc g{};
  g.M = M; g.N = N; g.K = K; g.alpha = 1.0; g.beta = 0.0;
  g.A = A; g.lda = lda; g.a_kcontig = 0; g.strideA = 0; g.a_slab = a_slab; g.a_slab_skip = a_slab_skip;
  g.B = B; g.ldb = ldb; g.b_kcontig = b_kcontig; g.strideB = 0;
  g.C = C; g.ldc = ldc; g.strideC = 0; g.batch = 1; g.cfg = cfg; g.ksplit = 0;
  return dev_gemm(g);
}
int qemb_gemm_flop_count(double* flops, int reset) { return dev_gemm_flop_count(flops, reset); }
int qemb_tape_cache_counters(int64_t* reused, int64_t* recorded, int reset) {
  long long a = 0, b = 0;
  tape_cache_counters(&a, &b, reset);
  if (reused) *reused = a;
  if (recorded) *recorded = b;
  return QEMB_OK;
}
int qemb_alloc_stats(long long* n, long long* nfree, double* ms, double* gb, int reset) { return dev_alloc_stats(n, nfree, ms, gb, reset); }
int qemb_ctx_timer_read(int ctx, int slot, double* total_ms, int64_t* count, int reset) { return dev_ctx_timer_read(ctx, slot, total_ms, count, reset); }
int qemb_op_k_from_pairs(int64_t n, const double* H, const double* D, double* K) { return dev_k_from_pairs(n, H, D, K); }
int qemb_op_jk_from_packed(int64_t n, const double* S4, const double* D, const double* Dp, double* Jp, double* K) { return dev_jk_from_packed(n, S4, D, Dp, Jp, K); }
int qemb_op_pack_pm_cols(int64_t rows, int64_t v, const double* in, double* Op, int64_t ldp, double* Om, int64_t ldm) { return dev_pack_pm_cols(rows, v, in, Op, ldp, Om, ldm); }
int qemb_op_scatter_pm_rows(int64_t o, int64_t ncols, const double* Xp, const double* Xm, double* out) { return dev_scatter_pm_rows(o, ncols, Xp, Xm, out); }
int qemb_op_pack_w_pm(int64_t o, const double* W, double* Ap, int64_t lda_p, double* Am, int64_t lda_m) { return dev_pack_w_pm(o, W, Ap, lda_p, Am, lda_m); }
int qemb_op_ladder_scatter_pm2(int64_t o, int64_t v, const double* Rp, int64_t ldp, const double* Rm, int64_t ldm, const double* Hp, const double* Hm,
                               int assign, double* t2) { return dev_ladder_scatter_pm2(o, v, Rp, ldp, Rm, ldm, Hp, Hm, assign, t2); }
int qemb_op_lincomb2(int64_t n, double a, const double* x, double b, const double* y, double beta, double* out) {
  const double c[2] = {a, b};
  const double* xs[2] = {x, y};
  return dev_lincomb(n, 2, c, xs, beta, out);
}
int qemb_op_mirror_lower(int64_t n, double* A, int64_t lda) { return dev_mirror_lower(n, A, lda); }
int qemb_op_small_k_update(int64_t batch, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t sA, const double* B, int64_t sB, double* C, int64_t sC) {
  return dev_small_k_update(batch, M, N, K, alpha, A, sA, B, sB, C, sC);
}
int qemb_op_ccsd_ph_layouts(int64_t o, int64_t v, const double* t2, const double* t1, double* T, double* Tp, double* S, double* Ut, double* Tpt, double* Th) {
  return dev_ccsd_ph_layouts(o, v, t2, t1, T, Tp, S, Ut, Tpt, Th);
}
int qemb_op_ccsd_ph_layouts_ring(int64_t o, int64_t v, const double* t2, const double* t1, double* Tp, double* S, double* Ut, double* Tpt) {
  return dev_ccsd_ph_layouts_ring(o, v, t2, t1, Tp, S, Ut, Tpt);
}
int qemb_op_ccsd_ring_prep(int64_t o, int64_t v, const double* t1, const double* P1, const double* W1base, const double* W2base, const double* ZB, const double* ZC,
                           const double* OB, const double* OC, double* R, double* W2) {
  return dev_ccsd_ring_prep(o, v, t1, P1, W1base, W2base, ZB, ZC, OB, OC, R, W2);
}
int qemb_op_ccsd_u_update(int64_t o, int64_t v, const double* A, const double* t1, const double* Z, double* U) { return dev_ccsd_u_update(o, v, A, t1, Z, U); }
int qemb_op_ccsd_ring_prep_rule(int64_t o, int64_t v, int replay) { return ccsd_use_ring_prep(o, v, replay != 0) ? 1 : 0; }
int qemb_op_ccsd_ovvv_slabs(int64_t o, int64_t v) { return dev_ccsd_ovvv_slabs(o, v); }
int qemb_op_ccsd_ovvv_pass(int64_t o, int64_t v, const double* ovvv, const double* t1, const double* Thk, double* ZB, double* PA) {
  return dev_ccsd_ovvv_pass(o, v, ovvv, t1, Thk, ZB, PA);
}
int qemb_op_copy4_two(const int64_t dim[4], const double* in, const int64_t si[4], double* out, const int64_t so[4], double alpha, double beta, const double* base,
                      double* out2, const double* in2, double c2a, double c2b) {
  Copy4Desc c{};
  for (int k = 0; k < 4; ++k) { c.dim[k] = dim[k]; c.si[k] = si[k]; c.so[k] = so[k]; }
  c.in = in; c.out = out; c.alpha = alpha; c.beta = beta; c.base = base;
  c.out2 = out2; c.in2 = in2; c.c2a = c2a; c.c2b = c2b;
  return dev_copy4(c);
}
int qemb_op_scatter_pm_rows_add(int64_t o, int64_t ncols, const double* Xp, const double* Xm, double* out, const double* add) { return dev_scatter_pm_rows(o, ncols, Xp, Xm, out, add); }
int qemb_op_ccsd_y_traces_add(int64_t o, int64_t v, const double* ZC, const double* ZB, double* Y, const double* add) { return dev_ccsd_y_traces(o, v, ZC, ZB, Y, add); }
int qemb_op_pack_w_pm_sum(int64_t o, const double* Wt, const double* X, const double* At, double* Ap, int64_t lda_p, double* Am, int64_t lda_m) {
  return dev_pack_w_pm_sum(o, Wt, X, At, Ap, lda_p, Am, lda_m);
}
int qemb_op_ccsd_t1_assemble(int64_t o, int64_t v, const double* t1, const double* Lvv, const double* Loo, const double* Fov, const double* S, const double* Lph1,
                             const double* PA, int SA, int64_t strideA, const double* PB, int SB, int64_t strideB, double* t1n) {
  return dev_ccsd_t1_assemble(o, v, t1, Lvv, Loo, Fov, S, Lph1, PA, SA, strideA, PB, SB, strideB, t1n);
}
int qemb_op_gemv_rows_two(int64_t rows1, int64_t cols1, const double* T1, int64_t ld1, const double* x1, double* y1, double a1, double b1,
                          int64_t rows2, int64_t cols2, const double* T2, int64_t ld2, const double* x2, double* y2, double a2, double b2) {
  return dev_gemv_rows_two(rows1, cols1, T1, ld1, x1, y1, a1, b1, rows2, cols2, T2, ld2, x2, y2, a2, b2);
}
int qemb_op_ccsd_y_traces_slabs(int64_t o, int64_t v, const double* ZC, const double* ZB, double* Y, const double* add, int S, int64_t stride, double scale) {
  return dev_ccsd_y_traces(o, v, ZC, ZB, Y, add, S, stride, scale);
}
int qemb_op_ccsd_finish_t2_rings(int64_t o, int64_t v, double* t2n, const double* U, const double* OV, const double* RS, const double* M, const double* eo, const double* ev, double* t1n) {
  return dev_ccsd_finish_t2_rings(o, v, t2n, U, OV, RS, M, eo, ev, t1n);
}
int qemb_op_diis_push(int64_t n, const double* trial, const double* prev, double* e, double* xcopy, int m, const double* const* ys, int self, double* row_dev, double* row_host) {
  void* pin = nullptr;
  QTRY(dev_pinned_alloc(&pin, sizeof(double) * 8));
  int rc = dev_diis_push(n, trial, prev, e, xcopy, m, ys, self, row_dev, (double*)pin);
  if (!rc) rc = dev_sync();
  if (!rc) for (int j = 0; j < m; ++j) row_host[j] = ((double*)pin)[j];
  dev_pinned_free(pin);
  return rc;
}
int qemb_op_ccsd_extrapolate_energy(int64_t o, int64_t v, int nterms, const double* coef, const double* const* xs, double* amp, const double* L, double* tau, double* e_host) {
  void* pin = nullptr;
  DBuf e_dev;
  QTRY(e_dev.alloc(1));
  QTRY(dev_pinned_alloc(&pin, sizeof(double) * 8));
  int rc = dev_ccsd_extrapolate_energy(o, v, nterms, coef, xs, amp, L, tau, e_dev, (double*)pin);
  if (!rc) rc = dev_sync();
  if (!rc) *e_host = *(double*)pin;
  dev_pinned_free(pin);
  return rc;
}
int qemb_op_ccsd_y_traces(int64_t o, int64_t v, const double* ZC, const double* ZB, double* Y) { return dev_ccsd_y_traces(o, v, ZC, ZB, Y); }
int qemb_op_gather_rows(int64_t nrows, int64_t len, const int64_t* idx_dev, const double* src, int64_t ld, double* dst) { return dev_gather_rows(nrows, len, idx_dev, src, ld, dst); }
int qemb_op_scale_rows(int64_t nrows, int64_t len, double* x, const double* s) { return dev_scale_rows(nrows, len, x, s); }
int qemb_op_pack_pair_rows(int64_t n, int64_t ncols, const double* in, double* out) { return dev_pack_pair_rows(n, ncols, in, out); }
int qemb_op_extract_pf(int64_t n, const double* Mp, int64_t p0, int64_t q0, int64_t r0, int64_t s0, int64_t sp, int64_t sq, int64_t sr, int64_t ss, double* out) {
  return dev_extract_pf(n, Mp, p0, q0, r0, s0, sp, sq, sr, ss, out);
}
int qemb_op_extract_pf_t(int64_t n, const double* T, int64_t x0, int64_t r0, int64_t s0, int64_t c0, int64_t sx, int64_t sr, int64_t ss, int64_t sc, double* out) {
  return dev_extract_pf_t(n, T, x0, r0, s0, c0, sx, sr, ss, sc, out);
}
int qemb_op_ladder_pack_vvvv_pf(int64_t n, int64_t o, const double* Mp, double* Vp, int64_t ldp, double* Vm, int64_t ldm) { return dev_ladder_pack_vvvv_pf(n, o, Mp, Vp, ldp, Vm, ldm); }
int qemb_op_extract_pf_t_compact(int64_t n, const double* T, int64_t x0, int64_t c0, int64_t sx, int64_t sr, int64_t ss, int64_t sc, double* out, int64_t slab) {
  return dev_extract_pf_t_compact(n, T, x0, c0, sx, sr, ss, sc, out, slab);
}
int qemb_op_gather_pair_cols(int64_t rows, int64_t n, const double* in, int64_t r0, int64_t s0, int64_t sr, int64_t ss, double* out) {
  return dev_gather_pair_cols(rows, n, in, r0, s0, sr, ss, out);
}
int qemb_op_extract_ps(int64_t n, const double* S, int64_t p0, int64_t q0, int64_t r0, int64_t s0, int64_t sp, int64_t sq, int64_t sr, int64_t ss, double* out) {
  return dev_extract_ps(n, S, p0, q0, r0, s0, sp, sq, sr, ss, out);
}
int qemb_op_extract_ps_packed(int64_t n, const double* S, int64_t p0, int64_t q0, int64_t r0, int64_t sp, int64_t sq, int64_t sr, double* out) {
  return dev_extract_ps_packed(n, S, p0, q0, r0, sp, sq, sr, out);
}
int qemb_op_unpack_pair_block(int64_t n, int64_t o, const double* S, double* Mv, int64_t ld) { return dev_unpack_pair_block(n, o, S, Mv, ld); }
int qemb_op_ladder_pack_vvvv_pf_ld(int64_t n, int64_t o, const double* Mp, int64_t ld, double* Vp, int64_t ldp, double* Vm, int64_t ldm) {
  return dev_ladder_pack_vvvv_pf_ld(n, o, Mp, ld, Vp, ldp, Vm, ldm);
}
int qemb_op_pack_pm_ovvv(int64_t o, int64_t v, const double* ovvv, double* Op, int64_t ldp, double* Om, int64_t ldm) { return dev_pack_pm_ovvv(o, v, ovvv, Op, ldp, Om, ldm); }
int qemb_op_df_pair_product(int64_t np, int64_t naux, const double* bb, double* out) { return df_pair_product(np, naux, bb, out); }
int qemb_op_unpack_tril_pair_rows(int64_t nr, int64_t n, const double* in, double* full) { return dev_unpack_tril_pair_rows(nr, n, in, full); }
int qemb_op_unpack_tril_rows(int64_t rows, int64_t n, const double* p, double* f) { return dev_unpack_tril_rows(rows, n, p, f); }
int qemb_op_pack_tril_rows(int64_t rows, int64_t n, const double* f, double* p) { return dev_pack_tril_rows(rows, n, f, p); }
int qemb_op_jacobi_eigh(int64_t n, double* A, double* w, double* V, int* sweeps) { return dev_jacobi_eigh(n, A, w, V, sweeps); }
// the fused steps of the fragment RHF of small fragments (scf.cpp), each on its own
int qemb_op_scf_fused_max(void) { return dev_scf_fused_max(); }
int qemb_op_jacobi_eigh_in_basis(int64_t n, const double* F, const double* Cp, double* w, double* C_out, double* C2_out, int nocc, double* dm_out, double stop_below, int* sweeps) {
  DBuf st;
  QTRY(st.alloc(1));
  QTRY(dev_jacobi_eigh_in_basis(n, F, Cp, w, C_out, C2_out, nocc, dm_out, stop_below, reinterpret_cast<int*>(st.p)));
  double word = 0.0;
  QTRY(dev_d2h(&word, st.p, sizeof(double)));
  int sw; std::memcpy(&sw, &word, sizeof(int));
  if (sweeps) *sweeps = sw;
  return jacobi_status_code(sw, "dev_jacobi_eigh_in_basis");
}
int qemb_op_scf_fock_small(int64_t n, const double* h, const double* J, const double* K, const double* D, double* F, double* err, double* scal2) { return dev_scf_fock_small(n, h, J, K, D, F, err, scal2); }
int qemb_op_pack_density_sym(int64_t n, const double* D, double* Dp) { return dev_pack_density_sym(n, D, Dp); }
int qemb_op_jacobi_svd(int64_t m, int64_t n, double* G, double* s, double* U, double* V, int* sweeps) { return dev_jacobi_svd(m, n, G, s, U, V, sweeps); }
int qemb_op_cholesky_lower(int64_t n, double* A) { return dev_cholesky_lower(n, A); }
// orbital localisation: the guard, then the sweeps (loc_ops.hip)
static thread_local int64_t g_joint_diag_limit = -1;
int qemb_op_joint_diag_mem_limit(int64_t bytes) { g_joint_diag_limit = bytes; return QEMB_OK; }
int qemb_op_joint_diag_bytes(int64_t K, int64_t m, int64_t* bytes, int* in_lds) {
  if (K < 0 || m < 0 || !bytes) { set_error("qemb_op_joint_diag_bytes: bad arguments"); return QEMB_ERR_ARG; }
  *bytes = (int64_t)loc::footprint_bytes(K, m);
  if (in_lds) *in_lds = loc::in_lds(K, m) ? 1 : 0;
  return QEMB_OK;
}
// the one guard of the localisation calls: the footprint (stack, U, workspace, and what the caller forms the stack with) against the limit, what is still to be
// allocated against the free memory
static int joint_diag_guard(const char* who, int64_t K, int64_t m, double extra_bytes, double to_allocate) {
  size_t free_b = 0, total_b = 0;
  QTRY(dev_mem_info(&free_b, &total_b));
  const double need = loc::footprint_bytes(K, m) + extra_bytes;
  if ((g_joint_diag_limit >= 0 && need > (double)g_joint_diag_limit) || to_allocate > (double)free_b) {
    set_error(std::string(who) + ": with K = " + std::to_string(K) + " and m = " + std::to_string(m) + " the stack, U and the workspace take " + std::to_string(need * 1e-9) +
              " GB (" + std::to_string(to_allocate * 1e-9) + " GB still to allocate), more than the " +
              std::to_string((g_joint_diag_limit >= 0 && (double)g_joint_diag_limit < (double)free_b ? (double)g_joint_diag_limit : (double)free_b) * 1e-9) + " GB they may take");
    return QEMB_ERR_ALLOC;
  }
  return QEMB_OK;
}
int qemb_op_joint_diag(int64_t K, int64_t m, double* Q_dev, double* U_dev, double stop_angle, int max_sweeps, int* sweeps, double* f, int* converged) {
  QTRY(loc::check_joint_diag("qemb_op_joint_diag", K, m, Q_dev != nullptr, U_dev != nullptr, stop_angle, max_sweeps));
  QTRY(joint_diag_guard("qemb_op_joint_diag", K, m, 0.0, 8.0 * (double)loc::work_doubles(K, m)));
  return dev_joint_diag(K, m, Q_dev, U_dev, stop_angle, max_sweeps, sweeps, f, converged);
}
// Edmiston-Ruedenberg on the factorised integrals: the 3-index factor of the columns C from the quarter transforms of the DF transform (DfContext::transform with no
// 4-index product), unpacked to the stack Q[P][i][j] = B^P_ij on the device, then the sweeps with K = naux
int qemb_df_localize_er(qemb_df_t df, const double* C_host, int m, double stop_angle, int max_sweeps, double* U_host, int* sweeps, double* f_before, double* f_after, int* converged) {
  if (!df || !C_host || !U_host) { set_error("qemb_df_localize_er: null argument"); return QEMB_ERR_ARG; }
  const DfContext* d = reinterpret_cast<const DfContext*>(df);
  if (d->Usp.p || d->Lpq_im.p) { set_error("qemb_df_localize_er: a semi-sparse or periodic context holds no dense real 3-index tensor"); return QEMB_ERR_UNSUPPORTED; }
  if ((!d->Linv.p && !d->identity_metric) || !d->Lpq.p || d->N <= 0 || d->naux <= 0) { set_error("qemb_df_localize_er: metric and 3-index integrals must be set"); return QEMB_ERR_ARG; }
  if (m <= 0 || m > d->N) { set_error("qemb_df_localize_er: need 0 < m <= N"); return QEMB_ERR_ARG; }
  const int64_t K = d->naux, N = d->N, np = (int64_t)m * (m + 1) / 2;
  QTRY(loc::check_joint_diag("qemb_df_localize_er", K, m, true, true, stop_angle, max_sweeps));      // (the stack and U are this call's own buffers)
  const double transform_b = 8.0 * ((double)K * m * N + (double)K * m * m + (d->identity_metric ? 1.0 : 2.0) * (double)K * np + (double)N * m);
  QTRY(joint_diag_guard("qemb_df_localize_er", K, m, transform_b, transform_b + loc::footprint_bytes(K, m)));
  DBuf dC, bb, Q, U;
  QTRY(dC.alloc(N * m));
  QTRY(dev_h2d(dC, C_host, sizeof(double) * N * m));
  QTRY(d->transform(dC, m, nullptr, nullptr, 0.0, &bb));
  QTRY(Q.alloc(K * m * m));
  QTRY(dev_unpack_tril_rows(K, m, bb, Q));
  bb.release();
  QTRY(U.alloc((int64_t)m * m));
  int cv0 = 0;
  QTRY(dev_joint_diag(K, m, Q, U, stop_angle, 0, nullptr, f_before, &cv0));
  QTRY(dev_joint_diag(K, m, Q, U, stop_angle, max_sweeps, sweeps, f_after, converged));
  return dev_d2h(U_host, U, sizeof(double) * m * m);
}

int qemb_op_tri_inverse_lower(int64_t n, const double* L, double* Linv) { return dev_tri_inverse_lower(n, L, Linv); }
int qemb_op_boys(int m_max, int64_t n, const double* x, double* out) { QTRY(dev_boys(m_max, n, x, out)); return dev_sync(); }
int qemb_op_int4c_class(int la, int lb, int lc, int ld, const void* bf_a, const void* bf_b, const void* bf_c, const void* bf_d, const double* c2s, double* out_host) {
  const int l[4] = {la, lb, lc, ld};
  const BfRecord* const rec[4] = {reinterpret_cast<const BfRecord*>(bf_a), reinterpret_cast<const BfRecord*>(bf_b), reinterpret_cast<const BfRecord*>(bf_c), reinterpret_cast<const BfRecord*>(bf_d)};
  return int4c_block(l, rec, c2s, out_host);
}
int qemb_op_int3c_class(int la, int lb, int lP, const void* bf_a, const void* bf_b, const void* bf_P, const double* c2s, double* out_host) {
  return int3c_block(la, lb, lP, reinterpret_cast<const BfRecord*>(bf_a), reinterpret_cast<const BfRecord*>(bf_b), reinterpret_cast<const BfRecord*>(bf_P), c2s, out_host);
}
int qemb_op_mp2_amplitudes(int64_t o, int64_t v, const double* ovov, const double* eo, const double* ev, double* t2, double* G, double* e_host) {
  DBuf part, e;
  QTRY(part.alloc(dev_mp2_partial_count(o, v))); QTRY(e.alloc(1));
  QTRY(dev_mp2_amplitudes(o, v, ovov, eo, ev, t2, G, part, e));
  return e_host ? dev_d2h(e_host, e, sizeof(double)) : dev_sync();
}

int qemb_op_rdm2_assemble(int kind, int64_t o, int64_t v, const double* t1, const double* t2, const double* dm1c, double* out) {
  QTRY(dev_rdm2_assemble(kind, o, v, t1, t2, dm1c, out));
  return dev_sync();
}

int qemb_op_ccsd_t(int o, int v, const double* t1, const double* t2, const double* ovvv, const double* ovoo, const double* ovov, const double* eo, const double* ev, int tile, double* e_t) {
  if (!e_t) { set_error("qemb_op_ccsd_t: e_t is NULL"); return QEMB_ERR_ARG; }
  return ccsd_t_energy(o, v, t1, t2, ovvv, ovoo, ovov, eo, ev, tile, e_t, nullptr);
}

int qemb_op_rdm2_add_nc(int64_t m, const double* g, double alpha, double* X) { return dev_rdm2_add_nc(m, g, alpha, X); }
int qemb_op_rdm2_symmetrize(int64_t m, const double* g, double* X) { return dev_rdm2_symmetrize(m, g, X); }
int qemb_op_rdm2_eri_dot(int64_t m, int sym, const double* eri, const double* K, double* e_host) {
  if (!e_host) { set_error("qemb_op_rdm2_eri_dot: e_host is NULL"); return QEMB_ERR_ARG; }
  DBuf w;
  QTRY(w.alloc(rdm2_full_grid(m > 0 ? m : 1) + 1));
  QTRY(dev_rdm2_eri_dot(m, sym, eri, K, w.p + 1, w.p));
  return dev_d2h(e_host, w.p, sizeof(double));
}

int qemb_op_kdf_split(int64_t rows, int64_t nao, const double* z, double* planes) { QTRY(dev_kdf_split(rows, nao, z, planes)); return dev_sync(); }
int qemb_op_kdf_stack(int64_t nk, int64_t nao, int64_t n, const double* ta, double* Cs, double* Dk) { QTRY(dev_kdf_stack(nk, nao, n, ta, Cs, Dk)); return dev_sync(); }
int qemb_op_kdf_pack(int64_t naux, int64_t n, const double* M, int paired, double w, double* F, int64_t ldf, double* out2_host) {
  if (!out2_host) { set_error("qemb_op_kdf_pack: out2_host is NULL"); return QEMB_ERR_ARG; }
  DBuf wk;
  QTRY(wk.alloc(dev_kdf_partial_count(naux > 0 ? naux : 1, n > 0 ? n : 1) + 2));
  QTRY(dev_kdf_pack(naux, n, M, paired, w, F, ldf, wk.p + 2, wk.p));
  return dev_d2h(out2_host, wk.p, 2 * sizeof(double));
}

// ---------------------------------------------------------------- fragment solver ----------------
void qemb_default_opts(qemb_solver_opts* o) {
  CcsdOptions c; ScfOptions s;
  memset(o, 0, sizeof *o);
  o->struct_size = (uint32_t)sizeof(qemb_solver_opts);
  o->cc_conv_tol = c.conv_tol; o->cc_conv_tol_normt = c.conv_tol_normt; o->cc_max_cycle = c.max_cycle; o->cc_diis_space = c.diis_space;
  o->scf_conv_tol = s.conv_tol; o->scf_conv_tol_grad = s.conv_tol_grad; o->scf_max_cycle = s.max_cycle; o->scf_diis_space = s.diis_space;
  o->warm_start = 0; o->verbose = 0;
  LambdaOptions l;
  o->relax_density = 0; o->lambda_conv_tol = l.conv_tol; o->lambda_max_cycle = l.max_cycle;
  o->strict_convergence = 1;
}
static FragmentOptions to_opts(const qemb_solver_opts* o) {
  FragmentOptions f;
  if (o) {
    f.cc.conv_tol = o->cc_conv_tol; f.cc.conv_tol_normt = o->cc_conv_tol_normt; f.cc.max_cycle = o->cc_max_cycle;
    f.cc.diis_space = o->cc_diis_space; f.cc.verbose = o->verbose;
    f.scf.conv_tol = o->scf_conv_tol; f.scf.conv_tol_grad = o->scf_conv_tol_grad; f.scf.max_cycle = o->scf_max_cycle;
    f.scf.diis_space = o->scf_diis_space; f.scf.verbose = o->verbose;
    f.warm_start = o->warm_start;
    f.relax_density = o->relax_density; f.lam.conv_tol = o->lambda_conv_tol; f.lam.max_cycle = o->lambda_max_cycle;
    f.lam.diis_space = o->cc_diis_space; f.lam.verbose = o->verbose;
    f.strict = o->strict_convergence;
  }
  return f;
}
// NULL options = defaults; anything else must carry the size of THIS header's struct (set by qemb_default_opts)
#define CHECK_OPTS(o)                                                                                                     \
  do {                                                                                                                    \
    if ((o) && (o)->struct_size != (uint32_t)sizeof(qemb_solver_opts)) {                                                  \
      set_error("qemb_solver_opts.struct_size is " + std::to_string((o)->struct_size) + ", this library expects " +       \
                std::to_string(sizeof(qemb_solver_opts)) + ": initialise the struct with qemb_default_opts() (binding built " \
                "against another qemb_hip.h?)");                                                                          \
      return QEMB_ERR_ARG;                                                                                                \
    }                                                                                                                     \
  } while (0)
#define FRAG(f) (reinterpret_cast<Fragment*>(f))
#define CHECK_FRAG(f) do { if (!(f)) { set_error("null fragment handle"); return QEMB_ERR_ARG; } } while (0)

int qemb_frag_create(int n, int n_f, qemb_frag_t* out) {
  if (n <= 0 || n_f < 0 || n_f > n || !out) { set_error("qemb_frag_create: bad arguments"); return QEMB_ERR_ARG; }
  *out = new Fragment(n, n_f);
  return QEMB_OK;
}
int qemb_frag_free(qemb_frag_t f) { delete FRAG(f); return QEMB_OK; }
int qemb_frag_set_eri_s4(qemb_frag_t f, const double* s4) { CHECK_FRAG(f); return FRAG(f)->set_eri_s4_host(s4); }
int qemb_frag_set_eri_s4_dev(qemb_frag_t f, const double* s4) { CHECK_FRAG(f); return FRAG(f)->set_eri_s4_dev(s4); }
int qemb_frag_set_df_factor(qemb_frag_t f, int naux, const double* B) { CHECK_FRAG(f); return FRAG(f)->set_df_factor_host(naux, B); }
int qemb_frag_set_df_factor_dev(qemb_frag_t f, int naux, const double* B) { CHECK_FRAG(f); return FRAG(f)->set_df_factor_dev(naux, B); }
int qemb_frag_set_df_only(qemb_frag_t f, int naux, const double* B) { CHECK_FRAG(f); return FRAG(f)->set_df_only_host(naux, B); }
int qemb_frag_set_df_only_dev(qemb_frag_t f, int naux, const double* B) { CHECK_FRAG(f); return FRAG(f)->set_df_only_dev(naux, B); }
int qemb_frag_resident_bytes(qemb_frag_t f, int64_t* bytes) { CHECK_FRAG(f); if (!bytes) { set_error("qemb_frag_resident_bytes: null argument"); return QEMB_ERR_ARG; } *bytes = FRAG(f)->resident_bytes(); return QEMB_OK; }
int qemb_frag_mo_route(qemb_frag_t f, int route) { CHECK_FRAG(f); return FRAG(f)->set_mo_route(route); }
int qemb_frag_mo_route_used(qemb_frag_t f, int* used_factor, int* naux) {
  CHECK_FRAG(f);
  if (used_factor) *used_factor = FRAG(f)->last_route_was_factor() ? 1 : 0;
  if (naux) *naux = FRAG(f)->df_naux();
  return QEMB_OK;
}
int qemb_frag_get_eri_s4(qemb_frag_t f, double* s4) {
  CHECK_FRAG(f);
  if (!s4) { set_error("qemb_frag_get_eri_s4: null buffer"); return QEMB_ERR_ARG; }
  return FRAG(f)->export_eri_s4(s4);      // the resident block, or B^T B of a fragment that lives on its factor (formed for this call)
}
int qemb_frag_get_df_factor(qemb_frag_t f, double* B) {
  CHECK_FRAG(f);
  if (!B) { set_error("qemb_frag_get_df_factor: null buffer"); return QEMB_ERR_ARG; }
  return FRAG(f)->export_df_factor(B);
}
int qemb_frag_set_energy_data(qemb_frag_t f, const double* h1, const double* veff0, const double* veff, double weight,
                              const int* centers, int ncenter) {
  CHECK_FRAG(f);
  for (int i = 0; i < ncenter; ++i) if (centers[i] < 0 || centers[i] >= FRAG(f)->nf()) { set_error("centre index outside the fragment sites"); return QEMB_ERR_ARG; }
  FRAG(f)->set_energy_data(h1, veff0, veff, weight, centers, ncenter);
  return QEMB_OK;
}
int qemb_frag_jk(qemb_frag_t f, const double* P, double* J, double* K) { CHECK_FRAG(f); return FRAG(f)->hf_veff_from_dm(P, J, K); }
// What a solve entry hands back through its nullable out-pointers, for fragment f of the call (0 of a single solve): the counters always, the energies of a call
// that did not fail.  e_total: the entry reports e_scf + e_corr_mo (the FCI eigenvalue) where the others report e_corr_mo.
static void store_result(Fragment* fr, const FragmentResult& r, int rc, int f, bool e_total, double* e_frag, double* e, double* e_scf, double* ebe_hf, int* n_iter, int* scf_cycles) {
  if (n_iter) n_iter[f] = r.n_iter;
  if (scf_cycles) scf_cycles[f] = r.scf_cycles;
  fr->last_lambda_iters = r.lambda_iters;
  if (rc < 0) return;
  if (e_frag) for (int k = 0; k < 3; ++k) e_frag[3 * f + k] = r.e_frag[k];
  if (e) e[f] = e_total ? r.e_scf + r.e_corr_mo : r.e_corr_mo;
  if (e_scf) e_scf[f] = r.e_scf;
  if (ebe_hf) ebe_hf[f] = r.ebe_hf;
}
// The handles, nsocc, h, dm0 and output pointers of a batched entry `name` as the Fragment batch calls take them; a foreign opts struct and null or repeated handles are refused
static int gather_batch(const char* name, int nfrag, const qemb_frag_t* frags, const int* nsocc, const double* const* h, const double* const* dm0, const qemb_solver_opts* opts,
                        double* const* mo_coeff, double* const* mo_energy, double* const* rdm1_emb, double* const* rdm1_mo, double* const* t1, double* const* t2,
                        std::vector<Fragment*>& frs, std::vector<int>& o, std::vector<const double*>& hs, std::vector<const double*>& dms, std::vector<Fragment::BatchOutputs>& outs) {
  if (nfrag < 0 || (nfrag > 0 && (!frags || !nsocc || !h))) { set_error(std::string(name) + ": bad arguments"); return QEMB_ERR_ARG; }
  CHECK_OPTS(opts);
  outs.assign(nfrag > 0 ? nfrag : 0, Fragment::BatchOutputs());
  for (int f = 0; f < nfrag; ++f) {
    if (!frags[f] || !h[f]) { set_error(std::string(name) + ": null fragment handle or h"); return QEMB_ERR_ARG; }
    for (int g = 0; g < f; ++g) if (frags[g] == frags[f]) { set_error(std::string(name) + ": the same fragment twice"); return QEMB_ERR_ARG; }
    frs.push_back(FRAG(frags[f])); o.push_back(nsocc[f]); hs.push_back(h[f]); dms.push_back(dm0 ? dm0[f] : nullptr);
    auto pick = [&](double* const* arr) { return arr ? arr[f] : nullptr; };
    outs[f].mo_coeff = pick(mo_coeff); outs[f].mo_energy = pick(mo_energy); outs[f].rdm1_emb = pick(rdm1_emb);
    outs[f].rdm1_mo = pick(rdm1_mo); outs[f].t1 = pick(t1); outs[f].t2 = pick(t2);
  }
  return QEMB_OK;
}
int qemb_frag_solve(qemb_frag_t f, int nsocc, const double* h, const double* dm0, const qemb_solver_opts* opts, int eeval,
                    double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* t1, double* t2,
                    double* e_frag, double* e_corr_mo, double* e_scf, double* ebe_hf, int* n_iter, int* scf_cycles) {
  CHECK_FRAG(f); CHECK_OPTS(opts);
  if (!h) { set_error("qemb_frag_solve: h is NULL"); return QEMB_ERR_ARG; }
  FragmentResult r;
  const int rc = FRAG(f)->solve(nsocc, h, dm0, to_opts(opts), eeval, &r, mo_coeff, mo_energy, rdm1_emb, rdm1_mo, t1, t2);
  store_result(FRAG(f), r, rc, 0, false, e_frag, e_corr_mo, e_scf, ebe_hf, n_iter, scf_cycles);
  return rc;        // QEMB_OK, or QEMB_WARN_NOCONV with strict_convergence = 0
}
int qemb_frag_solve_batch(int nfrag, const qemb_frag_t* frags, const int* nsocc, const double* const* h, const double* const* dm0,
                          const qemb_solver_opts* opts, int eeval, double* const* mo_coeff, double* const* mo_energy,
                          double* const* rdm1_emb, double* const* rdm1_mo, double* const* t1, double* const* t2, double* e_frag,
                          double* e_corr_mo, double* e_scf, double* ebe_hf, int* n_iter, int* scf_cycles, int64_t* stats) {
  std::vector<Fragment*> frs; std::vector<int> o; std::vector<const double*> hs, dms; std::vector<Fragment::BatchOutputs> outs;
  QTRY(gather_batch("qemb_frag_solve_batch", nfrag, frags, nsocc, h, dm0, opts, mo_coeff, mo_energy, rdm1_emb, rdm1_mo, t1, t2, frs, o, hs, dms, outs));
  std::vector<FragmentResult> res;
  LockstepStats st;
  const int rc = Fragment::solve_batch(frs, o, hs, dms, to_opts(opts), eeval, res, outs, &st);
  for (int f = 0; f < (int)res.size(); ++f) store_result(frs[f], res[f], rc, f, false, e_frag, e_corr_mo, e_scf, ebe_hf, n_iter, scf_cycles);
  if (stats) { stats[0] = st.merged_runs; stats[1] = st.launches; stats[2] = st.grouped; stats[3] = st.operations; stats[4] = st.max_group; }
  return rc;
}
int qemb_frag_solve_mp2(qemb_frag_t f, int nsocc, const double* h, const double* dm0, const qemb_solver_opts* opts, int eeval,
                        double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* t2, double* e_frag,
                        double* e_corr_mo, double* e_scf, double* ebe_hf, int* scf_cycles) {
  CHECK_FRAG(f); CHECK_OPTS(opts);
  if (!h) { set_error("qemb_frag_solve_mp2: h is NULL"); return QEMB_ERR_ARG; }
  FragmentResult r;
  const int rc = FRAG(f)->solve_mp2(nsocc, h, dm0, to_opts(opts), eeval, &r, mo_coeff, mo_energy, rdm1_emb, rdm1_mo, t2);
  store_result(FRAG(f), r, rc, 0, false, e_frag, e_corr_mo, e_scf, ebe_hf, nullptr, scf_cycles);
  return rc;        // QEMB_OK, or QEMB_WARN_NOCONV with strict_convergence = 0
}
int qemb_frag_solve_mp2_batch(int nfrag, const qemb_frag_t* frags, const int* nsocc, const double* const* h, const double* const* dm0,
                              const qemb_solver_opts* opts, int eeval, double* const* mo_coeff, double* const* mo_energy,
                              double* const* rdm1_emb, double* const* rdm1_mo, double* const* t2, double* e_frag, double* e_corr_mo,
                              double* e_scf, double* ebe_hf, int* scf_cycles) {
  std::vector<Fragment*> frs; std::vector<int> o; std::vector<const double*> hs, dms; std::vector<Fragment::BatchOutputs> outs;
  QTRY(gather_batch("qemb_frag_solve_mp2_batch", nfrag, frags, nsocc, h, dm0, opts, mo_coeff, mo_energy, rdm1_emb, rdm1_mo, nullptr, t2, frs, o, hs, dms, outs));
  std::vector<FragmentResult> res;
  const int rc = Fragment::solve_mp2_batch(frs, o, hs, dms, to_opts(opts), eeval, res, outs);
  for (int f = 0; f < (int)res.size(); ++f) store_result(frs[f], res[f], rc, f, false, e_frag, e_corr_mo, e_scf, ebe_hf, nullptr, scf_cycles);
  return rc;
}
// ---- solver == "FCI-hip"
void qemb_default_fci_opts(qemb_fci_opts* o) {
  FciOptions d;
  memset(o, 0, sizeof *o);
  o->struct_size = (uint32_t)sizeof(qemb_fci_opts);
  o->conv_tol = d.conv_tol; o->max_cycle = d.max_cycle; o->max_space = d.max_space; o->lindep = d.lindep;
}
int qemb_frag_solve_fci(qemb_frag_t f, int nsocc, const double* h, const double* dm0, const qemb_solver_opts* opts, const qemb_fci_opts* fci_opts, int eeval,
                        double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* civec, double* e_frag, double* e_fci, double* e_scf,
                        double* ebe_hf, int* n_iter, int* scf_cycles) {
  CHECK_FRAG(f); CHECK_OPTS(opts);
  if (fci_opts && fci_opts->struct_size != (uint32_t)sizeof(qemb_fci_opts)) {
    set_error("qemb_fci_opts.struct_size is " + std::to_string(fci_opts->struct_size) + ", this library expects " + std::to_string(sizeof(qemb_fci_opts)) +
              ": initialise the struct with qemb_default_fci_opts()");
    return QEMB_ERR_ARG;
  }
  if (!h) { set_error("qemb_frag_solve_fci: h is NULL"); return QEMB_ERR_ARG; }
  FciOptions fo;
  if (fci_opts) { fo.conv_tol = fci_opts->conv_tol; fo.max_cycle = fci_opts->max_cycle; fo.max_space = fci_opts->max_space; fo.lindep = fci_opts->lindep; }
  FragmentResult r;
  const int rc = FRAG(f)->solve_fci(nsocc, h, dm0, to_opts(opts), fo, eeval, &r, mo_coeff, mo_energy, rdm1_emb, rdm1_mo, civec);
  store_result(FRAG(f), r, rc, 0, true, e_frag, e_fci, e_scf, ebe_hf, n_iter, scf_cycles);
  return rc;        // QEMB_OK, or QEMB_WARN_NOCONV with strict_convergence = 0
}
int qemb_frag_fci_bytes(int n, int nsocc, int max_space, int64_t* bytes) {
  if (n <= 0 || nsocc <= 0 || nsocc > n || max_space < 2 || !bytes) { set_error("qemb_frag_fci_bytes: bad arguments"); return QEMB_ERR_ARG; }
  if (n > kFciMaxOrb) { set_error("qemb_frag_fci_bytes: n = " + std::to_string(n) + " embedding orbitals; the determinant-space solver takes at most " + std::to_string(kFciMaxOrb)); return QEMB_ERR_UNSUPPORTED; }
  *bytes = fci_bytes_slab(n, nsocc, max_space, 0);
  return QEMB_OK;
}
int qemb_frag_fci_bytes_slab(int n, int nsocc, int max_space, int64_t rows, int64_t* bytes) {
  if (n <= 0 || nsocc <= 0 || nsocc > n || max_space < 2 || rows < 0 || !bytes) { set_error("qemb_frag_fci_bytes_slab: bad arguments"); return QEMB_ERR_ARG; }
  if (n > kFciMaxOrb) { set_error("qemb_frag_fci_bytes_slab: n = " + std::to_string(n) + " embedding orbitals; the determinant-space solver takes at most " + std::to_string(kFciMaxOrb)); return QEMB_ERR_UNSUPPORTED; }
  *bytes = fci_bytes_slab(n, nsocc, max_space, rows);
  return QEMB_OK;
}
int qemb_frag_fci_slab(qemb_frag_t f, int64_t rows) { CHECK_FRAG(f); return FRAG(f)->set_fci_slab(rows); }
int qemb_frag_fci_slab_used(qemb_frag_t f, int64_t* rows, int64_t* n_slab) { CHECK_FRAG(f); FRAG(f)->fci_slab_used(rows, n_slab); return QEMB_OK; }
int qemb_frag_fci_mem_limit(qemb_frag_t f, int64_t bytes) { CHECK_FRAG(f); FRAG(f)->set_fci_mem_limit(bytes); return QEMB_OK; }
int qemb_frag_fci_residual(qemb_frag_t f, double* residual) { CHECK_FRAG(f); if (residual) *residual = FRAG(f)->fci_residual(); return QEMB_OK; }
int qemb_op_fci_links(int n, int nsocc, int64_t* ns, int* nlink, int32_t* strings_host, int32_t* links_host) {
  const FciTables* T = nullptr;
  QTRY(fci_tables(n, nsocc, &T));
  if (ns) *ns = T->ns;
  if (nlink) *nlink = T->nlink;
  if (strings_host) std::memcpy(strings_host, T->strings.data(), sizeof(int32_t) * T->strings.size());
  if (links_host) std::memcpy(links_host, T->links.data(), sizeof(int32_t) * T->links.size());
  return QEMB_OK;
}
namespace {
// sigma = H c on handed-in data in slabs of `rows` alpha rows (fci_apply; 0: the whole space): k on the device, D and G, one untimed application; ms3 (nullable):
// then one more whose three steps are bracketed by device timers, summed over the slabs: ms3 = gather, product, sigma gather (tools/fci_bench.py)
int fci_sigma_op(const std::string& who, int n, int nsocc, const double* h_host, const double* V_dev, const double* c_dev, double* sigma_dev, int64_t rows, double* ms3) {
  if (!h_host || !V_dev || !c_dev || !sigma_dev) { set_error(who + ": null argument"); return QEMB_ERR_ARG; }
  const FciTables* T = nullptr;
  QTRY(fci_tables(n, nsocc, &T));
  const int64_t n2 = (int64_t)n * n, ns = T->ns, R = rows > 0 ? std::min(rows, ns) : ns;
  std::vector<double> Vh((size_t)(n2 * n2)), kh((size_t)n2);
  QTRY(dev_d2h(Vh.data(), V_dev, sizeof(double) * n2 * n2));
  fci_one_body(n, h_host, Vh.data(), kh.data());
  DBuf kd, D, G;
  QTRY(kd.alloc(n2)); QTRY(D.alloc(n2 * R * ns)); QTRY(G.alloc(n2 * R * ns));
  QTRY(dev_h2d(kd, kh.data(), sizeof(double) * n2));
  QTRY(fci_apply(*T, kd, V_dev, c_dev, D, G, sigma_dev, R));
  if (!ms3) return dev_sync();
  const int slot[3] = {10, 11, 12};
  for (int s : slot) QTRY(dev_timer_reset(s));
  for (int64_t a0 = 0; a0 < ns; a0 += R) {
    const int64_t a1 = std::min(ns, a0 + R), Ns = (a1 - a0) * ns;
    { TimerScope t(slot[0]); QTRY(dev_fci_gather_slab(n, ns, T->nlink, T->links_dev, c_dev, a0, a1, D)); QTRY(t.close()); }
    { TimerScope t(slot[1]); QTRY(gemm(n2, Ns, n2, 1.0, V_dev, n2, true, D, Ns, false, 0.0, G, Ns)); QTRY(t.close()); }
    { TimerScope t(slot[2]); QTRY(dev_fci_sigma_slab(n, ns, T->nlink, T->links_dev, kd, a0, a1, D, G, sigma_dev)); QTRY(t.close()); }
  }
  for (int k = 0; k < 3; ++k) { int64_t cnt = 0; QTRY(dev_timer_read(slot[k], &ms3[k], &cnt)); }
  return QEMB_OK;
}
int fci_rdm12_op(const std::string& who, int n, int nsocc, const double* c_dev, int cumulant, int64_t rows, double* dm1_host, double* dm2_dev) {
  if (!c_dev || !dm1_host) { set_error(who + ": null argument"); return QEMB_ERR_ARG; }
  const FciTables* T = nullptr;
  QTRY(fci_tables(n, nsocc, &T));
  return fci_rdm12(*T, c_dev, cumulant ? nsocc : -1, dm1_host, dm2_dev, rows);
}
}  // namespace
int qemb_op_fci_sigma(int n, int nsocc, const double* h_host, const double* V_dev, const double* c_dev, double* sigma_dev) {
  return fci_sigma_op("qemb_op_fci_sigma", n, nsocc, h_host, V_dev, c_dev, sigma_dev, 0, nullptr);
}
int qemb_op_fci_sigma_timed(int n, int nsocc, const double* h_host, const double* V_dev, const double* c_dev, double* sigma_dev, double* ms3) {
  if (!ms3) { set_error("qemb_op_fci_sigma_timed: null argument"); return QEMB_ERR_ARG; }
  return fci_sigma_op("qemb_op_fci_sigma_timed", n, nsocc, h_host, V_dev, c_dev, sigma_dev, 0, ms3);
}
int qemb_op_fci_sigma_slab(int n, int nsocc, const double* h_host, const double* V_dev, const double* c_dev, double* sigma_dev, int64_t rows, double* ms3) {
  if (h_host && V_dev && c_dev && sigma_dev && rows <= 0) { set_error("qemb_op_fci_sigma_slab: rows must be positive"); return QEMB_ERR_ARG; }
  return fci_sigma_op("qemb_op_fci_sigma_slab", n, nsocc, h_host, V_dev, c_dev, sigma_dev, rows, ms3);
}
int qemb_op_fci_rdm12(int n, int nsocc, const double* c_dev, int cumulant, double* dm1_host, double* dm2_dev) {
  return fci_rdm12_op("qemb_op_fci_rdm12", n, nsocc, c_dev, cumulant, 0, dm1_host, dm2_dev);
}
int qemb_op_fci_rdm12_slab(int n, int nsocc, const double* c_dev, int cumulant, int64_t rows, double* dm1_host, double* dm2_dev) {
  if (c_dev && dm1_host && rows <= 0) { set_error("qemb_op_fci_rdm12_slab: rows must be positive"); return QEMB_ERR_ARG; }
  return fci_rdm12_op("qemb_op_fci_rdm12_slab", n, nsocc, c_dev, cumulant, rows, dm1_host, dm2_dev);
}
// ---- solver == "SCI-hip"
void qemb_default_sci_opts(qemb_sci_opts* o) {
  SciOptions d;
  memset(o, 0, sizeof *o);
  o->struct_size = (uint32_t)sizeof(qemb_sci_opts);
  o->eps_var = d.eps_var; o->conv_tol = d.conv_tol; o->max_cycle = d.max_cycle; o->max_space = d.max_space; o->max_round = d.max_round; o->max_det = d.max_det;
}
int qemb_frag_solve_sci(qemb_frag_t f, int nsocc, const double* h, const double* dm0, const qemb_solver_opts* opts, const qemb_sci_opts* sci_opts, int eeval,
                        double* mo_coeff, double* mo_energy, double* rdm1_emb, double* rdm1_mo, double* e_frag, double* e_sci, double* e_scf,
                        double* ebe_hf, int* n_iter, int* scf_cycles) {
  CHECK_FRAG(f); CHECK_OPTS(opts);
  if (sci_opts && sci_opts->struct_size != (uint32_t)sizeof(qemb_sci_opts)) {
    set_error("qemb_sci_opts.struct_size is " + std::to_string(sci_opts->struct_size) + ", this library expects " + std::to_string(sizeof(qemb_sci_opts)) +
              ": initialise the struct with qemb_default_sci_opts()");
    return QEMB_ERR_ARG;
  }
  if (!h) { set_error("qemb_frag_solve_sci: h is NULL"); return QEMB_ERR_ARG; }
  SciOptions so;
  if (sci_opts) {
    so.eps_var = sci_opts->eps_var; so.conv_tol = sci_opts->conv_tol; so.max_cycle = sci_opts->max_cycle; so.max_space = sci_opts->max_space;
    so.max_round = sci_opts->max_round; so.max_det = sci_opts->max_det;
  }
  FragmentResult r;
  const int rc = FRAG(f)->solve_sci(nsocc, h, dm0, to_opts(opts), so, eeval, &r, mo_coeff, mo_energy, rdm1_emb, rdm1_mo);
  store_result(FRAG(f), r, rc, 0, true, e_frag, e_sci, e_scf, ebe_hf, n_iter, scf_cycles);
  return rc;        // QEMB_OK, or QEMB_WARN_NOCONV with strict_convergence = 0
}
int qemb_frag_sci_stats(qemb_frag_t f, int64_t* ndet, int* rounds, int64_t* nnz, double* residual) {
  CHECK_FRAG(f);
  const SciResult& r = FRAG(f)->sci_result();
  if (ndet) *ndet = r.ndet;
  if (rounds) *rounds = r.rounds;
  if (nnz) *nnz = r.nnz;
  if (residual) *residual = r.residual;
  return QEMB_OK;
}
int qemb_frag_sci_stage_ms(qemb_frag_t f, double* ms5) {
  CHECK_FRAG(f);
  if (!ms5) { set_error("qemb_frag_sci_stage_ms: null argument"); return QEMB_ERR_ARG; }
  for (int k = 0; k < SCI_T_COUNT; ++k) ms5[k] = FRAG(f)->sci_result().ms[k];
  return QEMB_OK;
}
int qemb_frag_sci_dets(qemb_frag_t f, uint64_t* alpha, uint64_t* beta, double* c) { CHECK_FRAG(f); return FRAG(f)->sci_dets(alpha, beta, c); }
int qemb_frag_sci_bytes(int n, int nsocc, int64_t max_det, int max_space, int64_t* bytes) {
  if (n <= 0 || nsocc <= 0 || nsocc > n || max_det < 1 || max_space < 2 || !bytes) { set_error("qemb_frag_sci_bytes: bad arguments"); return QEMB_ERR_ARG; }
  if (n > kSciMaxOrb) { set_error("qemb_frag_sci_bytes: n = " + std::to_string(n) + " embedding orbitals; the selected CI takes at most " + std::to_string(kSciMaxOrb)); return QEMB_ERR_UNSUPPORTED; }
  *bytes = sci_bytes(n, nsocc, max_det, max_space);
  return QEMB_OK;
}
int qemb_frag_sci_mem_limit(qemb_frag_t f, int64_t bytes) { CHECK_FRAG(f); FRAG(f)->set_sci_mem_limit(bytes); return QEMB_OK; }
int qemb_frag_sci_pt2(qemb_frag_t f, double eps_pt, int64_t max_ext, double* e_pt2, int64_t* n_ext, int* batches, double* ms3) {
  CHECK_FRAG(f);
  return FRAG(f)->sci_pt2(eps_pt, max_ext, e_pt2, n_ext, batches, ms3);
}
int qemb_frag_sci_pt2_bytes(int n, int nsocc, int64_t ndet, int64_t max_ext, int64_t* bytes) {
  if (n <= 0 || nsocc <= 0 || nsocc > n || ndet < 1 || max_ext < 1 || !bytes) { set_error("qemb_frag_sci_pt2_bytes: bad arguments"); return QEMB_ERR_ARG; }
  if (n > kSciMaxOrb) { set_error("qemb_frag_sci_pt2_bytes: n = " + std::to_string(n) + " embedding orbitals; the selected CI takes at most " + std::to_string(kSciMaxOrb)); return QEMB_ERR_UNSUPPORTED; }
  *bytes = Fragment::sci_pt2_work_bytes(n, nsocc, ndet, max_ext);
  return QEMB_OK;
}
// ---- the operations of the selected CI on handed-in data (host arrays but V_dev); a space: ndet sorted keys alpha[k], beta[k]
namespace {
int sci_upload(int64_t ndet, const uint64_t* alpha, const uint64_t* beta, const double* c, SciSpace& V) {
  if (ndet <= 0 || !alpha || !beta) { set_error("qemb_op_sci: a space needs ndet > 0 keys"); return QEMB_ERR_ARG; }
  std::vector<uint64_t> k((size_t)(2 * ndet));
  for (int64_t i = 0; i < ndet; ++i) {
    k[(size_t)(2 * i)] = alpha[i]; k[(size_t)(2 * i + 1)] = beta[i];
    if (i > 0 && !sci_key_less(alpha[i - 1], beta[i - 1], alpha[i], beta[i])) { set_error("qemb_op_sci: the keys must be sorted by (alpha, beta) and distinct"); return QEMB_ERR_ARG; }
  }
  QTRY(V.keys.alloc(2 * ndet)); QTRY(V.c.alloc(ndet));
  QTRY(dev_h2d(V.keys, k.data(), sizeof(uint64_t) * 2 * ndet));
  if (c) QTRY(dev_h2d(V.c, c, sizeof(double) * ndet)); else QTRY(dev_fill(V.c, ndet, 0.0));
  V.N = ndet;
  return 0;
}
int sci_download(const uint64_t* keys_dev, int64_t N, uint64_t* alpha, uint64_t* beta) {
  std::vector<uint64_t> k((size_t)(2 * N));
  if (N > 0) QTRY(dev_d2h(k.data(), keys_dev, sizeof(uint64_t) * 2 * N));
  for (int64_t i = 0; i < N; ++i) { alpha[i] = k[(size_t)(2 * i)]; beta[i] = k[(size_t)(2 * i + 1)]; }
  return 0;
}
int sci_op_integrals(int n, const double* h_host, const double* V_dev, DBuf& hd, double* dbl_bound) {
  const int64_t n2 = (int64_t)n * n;
  if (n <= 0 || n > kSciMaxOrb || !h_host || !V_dev) { set_error("qemb_op_sci: need 0 < n <= 64, h and V"); return QEMB_ERR_ARG; }
  QTRY(hd.alloc(n2));
  QTRY(dev_h2d(hd, h_host, sizeof(double) * n2));
  if (dbl_bound) QTRY(sci_double_bound(n, V_dev, dbl_bound));
  return 0;
}
}  // namespace
int qemb_op_sci_screen(int n, int nsocc, const double* h_host, const double* V_dev, int64_t ndet, const uint64_t* alpha, const uint64_t* beta, const double* c, double eps,
                       int64_t slab, int64_t cap, int64_t max_out, int64_t* njoined, uint64_t* out_alpha, uint64_t* out_beta) {
  if (!c || !njoined || max_out < 0 || (max_out > 0 && (!out_alpha || !out_beta)) || !(eps > 0.0) || nsocc <= 0 || nsocc >= n) { set_error("qemb_op_sci_screen: bad arguments"); return QEMB_ERR_ARG; }
  DBuf hd, joined; SciSpace V; double bound = 0.0;
  QTRY(sci_op_integrals(n, h_host, V_dev, hd, &bound));
  QTRY(sci_upload(ndet, alpha, beta, c, V));
  QTRY(sci_screen(n, nsocc, hd, V_dev, bound, V, eps, slab, cap, (int64_t)1 << 40, joined, njoined));
  if (*njoined > max_out) return QEMB_OK;      // the count alone: call again with room
  return sci_download((const uint64_t*)joined.p, *njoined, out_alpha, out_beta);
}
int qemb_op_sci_pt2(int n, int nsocc, const double* h_host, const double* V_dev, int64_t ndet, const uint64_t* alpha, const uint64_t* beta, const double* c, double e_var, double eps_pt,
                    int64_t max_ext, int64_t slab, int64_t cap, double* e_pt2, int64_t* n_ext, int* batches) {
  if (!c || !(eps_pt > 0.0) || nsocc <= 0 || nsocc >= n) { set_error("qemb_op_sci_pt2: bad arguments (need c, eps_pt > 0 and 0 < nsocc < n)"); return QEMB_ERR_ARG; }
  DBuf hd; SciSpace V; double bound = 0.0, e = 0.0; int64_t next = 0; int nb = 0;
  QTRY(sci_op_integrals(n, h_host, V_dev, hd, &bound));
  QTRY(sci_upload(ndet, alpha, beta, c, V));
  const int rc = sci_pt2(n, nsocc, hd, V_dev, bound, V, e_var, eps_pt, max_ext > 0 ? max_ext : (int64_t)1 << 40, slab, cap, &e, &next, &nb);
  if (e_pt2) *e_pt2 = e;
  if (n_ext) *n_ext = next;
  if (batches) *batches = nb;
  return rc;
}
int qemb_op_sci_merge(int64_t ndet, const uint64_t* alpha, const uint64_t* beta, const double* c, int64_t njoined, const uint64_t* jalpha, const uint64_t* jbeta,
                      uint64_t* out_alpha, uint64_t* out_beta, double* out_c) {
  if (!c || !out_alpha || !out_beta || !out_c) { set_error("qemb_op_sci_merge: null argument"); return QEMB_ERR_ARG; }
  SciSpace V, J, W;
  QTRY(sci_upload(ndet, alpha, beta, c, V));
  QTRY(sci_upload(njoined, jalpha, jbeta, nullptr, J));
  QTRY(sci_merge(V, J.k(), J.N, W));
  QTRY(sci_download(W.k(), W.N, out_alpha, out_beta));
  return dev_d2h(out_c, W.c, sizeof(double) * W.N);
}
int qemb_op_sci_matrix(int n, const double* h_host, const double* V_dev, int64_t ndet, const uint64_t* alpha, const uint64_t* beta, int64_t max_nnz, int64_t* nnz,
                       int64_t* rowptr, int32_t* col, double* val) {
  if (!nnz || !rowptr) { set_error("qemb_op_sci_matrix: null argument"); return QEMB_ERR_ARG; }
  DBuf hd; SciSpace V; SciMatrix H;
  QTRY(sci_op_integrals(n, h_host, V_dev, hd, nullptr));
  QTRY(sci_upload(ndet, alpha, beta, nullptr, V));
  QTRY(sci_build(n, hd, V_dev, V.k(), V.N, -1, "qemb_op_sci_matrix", H));
  *nnz = H.nnz;
  QTRY(dev_d2h(rowptr, H.rowptr, sizeof(int64_t) * (ndet + 1)));
  if (H.nnz > max_nnz || !col || !val) return QEMB_OK;      // the counts alone: call again with room
  QTRY(dev_d2h(col, H.col, sizeof(int32_t) * H.nnz));
  return dev_d2h(val, H.val, sizeof(double) * H.nnz);
}
int qemb_op_sci_spmv(int n, const double* h_host, const double* V_dev, int64_t ndet, const uint64_t* alpha, const uint64_t* beta, const double* x, double* y) {
  if (!x || !y) { set_error("qemb_op_sci_spmv: null argument"); return QEMB_ERR_ARG; }
  DBuf hd, yd; SciSpace V; SciMatrix H;
  QTRY(sci_op_integrals(n, h_host, V_dev, hd, nullptr));
  QTRY(sci_upload(ndet, alpha, beta, x, V));
  QTRY(sci_build(n, hd, V_dev, V.k(), V.N, -1, "qemb_op_sci_spmv", H));
  QTRY(yd.alloc(ndet));
  QTRY(dev_sci_spmv(ndet, H.rp(), H.ci(), H.val, V.c, yd));
  return dev_d2h(y, yd, sizeof(double) * ndet);
}
int qemb_op_sci_rdm12(int n, int nsocc, const double* h_host, const double* V_dev, int64_t ndet, const uint64_t* alpha, const uint64_t* beta, const double* c, int cumulant,
                      double* dm1, double* dm2) {
  if (!c || !dm1 || !dm2) { set_error("qemb_op_sci_rdm12: null argument"); return QEMB_ERR_ARG; }
  const int64_t n2 = (int64_t)n * n;
  DBuf hd, G; SciSpace V; SciMatrix H;
  QTRY(sci_op_integrals(n, h_host, V_dev, hd, nullptr));
  QTRY(sci_upload(ndet, alpha, beta, c, V));
  QTRY(sci_build(n, hd, V_dev, V.k(), V.N, -1, "qemb_op_sci_rdm12", H));
  QTRY(G.alloc(n2 * n2));
  QTRY(sci_rdm12(n, V.k(), V.N, H.rp(), H.ci(), V.c, cumulant ? nsocc : -1, dm1, G));
  return dev_d2h(dm2, G, sizeof(double) * n2 * n2);
}
int qemb_frag_rdm2(qemb_frag_t f, int kind, int with_dm1, double* out) {
  CHECK_FRAG(f);
  if (!out) { set_error("qemb_frag_rdm2: out is NULL"); return QEMB_ERR_ARG; }
  return FRAG(f)->rdm2(kind, with_dm1, out);
}
int qemb_frag_rdm2_dev(qemb_frag_t f, int kind, int with_dm1, double* out_dev) {
  CHECK_FRAG(f);
  if (!out_dev) { set_error("qemb_frag_rdm2_dev: out_dev is NULL"); return QEMB_ERR_ARG; }
  return FRAG(f)->rdm2(kind, with_dm1, out_dev, true);
}
int qemb_rdm2_full_guard(int64_t nao, int64_t need_bytes, int64_t limit_bytes) {
  size_t free_b = 0, total_b = 0;
  QTRY(dev_mem_info(&free_b, &total_b));
  double room = (double)free_b;
  if (limit_bytes >= 0 && (double)limit_bytes < room) room = (double)limit_bytes;
  if (nao <= 0 || need_bytes < 0) { set_error("qemb_rdm2_full_guard: bad arguments"); return QEMB_ERR_ARG; }
  if ((double)need_bytes > room) {
    const double n4 = 8e-9 * (double)nao * (double)nao * (double)nao * (double)nao;
    set_error("full-basis 2-RDM: with N = " + std::to_string(nao) + " the N^4 accumulator takes " + std::to_string(n4) + " GB and the workspace " +
              std::to_string((double)need_bytes * 1e-9 - n4) + " GB, more than the " + std::to_string(room * 1e-9) + " GB of device memory they may take");
    return QEMB_ERR_ALLOC;
  }
  return QEMB_OK;
}
int qemb_frag_rdm2_mem_limit(qemb_frag_t f, int64_t bytes) { CHECK_FRAG(f); FRAG(f)->set_rdm2_mem_limit(bytes); return QEMB_OK; }
int qemb_frag_ccsd_t(qemb_frag_t f, double* e_t, int* tile, int64_t* n_tile_triples, double* ms4) {
  CHECK_FRAG(f);
  CcsdTStats st;
  double ms_int = 0.0;
  const int rc = FRAG(f)->ccsd_t(e_t, &st, &ms_int);
  if (tile) *tile = st.tile;
  if (n_tile_triples) *n_tile_triples = st.n_tile_triples;
  if (ms4) { ms4[0] = st.ms_images; ms4[1] = st.ms_gemm; ms4[2] = st.ms_assemble; ms4[3] = ms_int; }
  return rc;
}
int qemb_frag_ccsd_t_bytes(qemb_frag_t f, int nsocc, int tile, int64_t* bytes) {
  CHECK_FRAG(f);
  if (nsocc == 0) nsocc = FRAG(f)->last_nsocc();      // as many as the last solve had
  if (nsocc <= 0 || nsocc > FRAG(f)->n() || tile < 1 || !bytes) { set_error("qemb_frag_ccsd_t_bytes: bad arguments (need 0 < nsocc <= n -- or 0 after a solve -- and tile >= 1)"); return QEMB_ERR_ARG; }
  *bytes = FRAG(f)->ccsd_t_work_bytes(nsocc, tile);
  return QEMB_OK;
}
int qemb_frag_ccsd_t_mem_limit(qemb_frag_t f, int64_t bytes) { CHECK_FRAG(f); FRAG(f)->set_ccsd_t_mem_limit(bytes); return QEMB_OK; }
int qemb_frag_drop_amplitudes(qemb_frag_t f) { CHECK_FRAG(f); FRAG(f)->drop_amplitudes(); return QEMB_OK; }
int qemb_frag_lambda_iters(qemb_frag_t f, int* n_iter) { CHECK_FRAG(f); if (n_iter) *n_iter = FRAG(f)->last_lambda_iters; return QEMB_OK; }
int qemb_frag_scf(qemb_frag_t f, int nsocc, const double* h, const double* dm0, const qemb_solver_opts* opts, double* mo_coeff,
                  double* mo_energy, double* J, double* K, double* e_scf, int* converged, int* cycles) {
  CHECK_FRAG(f); CHECK_OPTS(opts);
  if (!h) { set_error("qemb_frag_scf: h is NULL"); return QEMB_ERR_ARG; }
  ScfResult r;
  int rc = FRAG(f)->scf_only(nsocc, h, dm0, to_opts(opts).scf, mo_coeff, mo_energy, J, K, &r);
  if (rc) return rc;
  if (e_scf) *e_scf = r.e_tot;
  if (converged) *converged = r.converged ? 1 : 0;
  if (cycles) *cycles = r.cycles;
  return QEMB_OK;
}
int qemb_frag_cphf(qemb_frag_t f, int nsocc, const double* h, const double* dm0, const qemb_solver_opts* opts, const double* vpots,
                   int npot, double* dPs) {
  CHECK_FRAG(f); CHECK_OPTS(opts);
  if (!h || !vpots || !dPs) { set_error("qemb_frag_cphf: null argument"); return QEMB_ERR_ARG; }
  return FRAG(f)->cphf_response(nsocc, h, dm0, to_opts(opts).scf, vpots, npot, dPs);
}
int qemb_ccsd_solve(int n, int nsocc, int n_f, const double* h, const double* eri_s4, const double* dm0,
                    const qemb_solver_opts* opts, const double* h1, const double* veff0, double weight, const int* centers,
                    int ncenter, double* mo_coeff, double* mo_energy, double* t1, double* t2, double* rdm1_emb, double* e_frag,
                    double* e_corr_mo, int* n_iter) {
  if (n <= 0 || n_f < 0 || n_f > n || !eri_s4) { set_error("qemb_ccsd_solve: bad arguments"); return QEMB_ERR_ARG; }
  CHECK_OPTS(opts);
  Fragment fr(n, n_f);
  int rc = fr.set_eri_s4_host(eri_s4);
  if (rc) return rc;
  const int eeval = (h1 && veff0 && e_frag) ? 1 : 0;
  if (eeval) fr.set_energy_data(h1, veff0, nullptr, weight, centers, ncenter);
  FragmentResult r;
  rc = fr.solve(nsocc, h, dm0, to_opts(opts), eeval, &r, mo_coeff, mo_energy, rdm1_emb, nullptr, t1, t2);
  if (n_iter) *n_iter = r.n_iter;
  if (rc < 0) return rc;
  if (e_frag && eeval) { e_frag[0] = r.e_frag[0]; e_frag[1] = r.e_frag[1]; e_frag[2] = r.e_frag[2]; }
  if (e_corr_mo) *e_corr_mo = r.e_corr_mo;
  return rc;
}
int qemb_frag_prepare_ccsd(qemb_frag_t f, int nsocc, const double* h, const double* dm0, const qemb_solver_opts* opts) {
  CHECK_FRAG(f); CHECK_OPTS(opts); return FRAG(f)->prepare_ccsd(nsocc, h, dm0, to_opts(opts));
}
int qemb_frag_ccsd_iterate(qemb_frag_t f, int niter, double* e, double* nt) { CHECK_FRAG(f); return FRAG(f)->ccsd_iterate(niter, e, nt); }
int qemb_frag_ccsd_export(qemb_frag_t f, const char* name, double* host, int64_t nelem) { CHECK_FRAG(f); return FRAG(f)->ccsd_export(name, host, nelem); }
int qemb_frag_ccsd_reset(qemb_frag_t f) { CHECK_FRAG(f); return FRAG(f)->ccsd_reset(); }

// ---------------------------------------------------------------- ERI transforms ------------------
static int deliver_s4(DBuf& s4, int n, double* out_host, qemb_frag_t frag, DBuf* factor = nullptr, int naux = 0) {
  const int64_t np = (int64_t)n * (n + 1) / 2;
  if (out_host) { int rc = dev_d2h(out_host, s4, sizeof(double) * np * np); if (rc) return rc; }
  if (frag) {
    if (FRAG(frag)->n() != n) { set_error("fragment handle has a different n"); return QEMB_ERR_ARG; }
    int rc = FRAG(frag)->adopt_eri_s4(std::move(s4));    // the transform's result block becomes the fragment's resident ERIs (round 4: no 4.7 GB copy)
    if (rc == 0 && factor && factor->p) rc = FRAG(frag)->adopt_df_factor(std::move(*factor), naux);      // ... and the factor it was formed from goes with it
    return rc;
  }
  return QEMB_OK;
}
int qemb_aoeri_upload(int N, const double* eri, int sym, qemb_aoeri_t* out) {
  if (N <= 0 || !eri || !out) { set_error("qemb_aoeri_upload: bad arguments"); return QEMB_ERR_ARG; }
  AoEri* a = new AoEri();
  int rc = a->upload(N, eri, sym);
  if (rc) { delete a; return rc; }
  *out = a;
  return QEMB_OK;
}
int qemb_aoeri_free(qemb_aoeri_t ao) { delete reinterpret_cast<AoEri*>(ao); return QEMB_OK; }
int qemb_ao2mo_dense(qemb_aoeri_t ao, const double* TA, int n, double* out_s4_host, qemb_frag_t frag) {
  if (!ao || !TA) { set_error("qemb_ao2mo_dense: null argument"); return QEMB_ERR_ARG; }
  AoEri* a = reinterpret_cast<AoEri*>(ao);
  DBuf dTA, s4;
  int rc;
  if ((rc = dTA.alloc((int64_t)a->N * n))) return rc;
  if ((rc = dev_h2d(dTA, TA, sizeof(double) * a->N * n))) return rc;
  if ((rc = s4.alloc(((int64_t)n * (n + 1) / 2) * ((int64_t)n * (n + 1) / 2)))) return rc;
  if ((rc = ao2mo_dense(*a, dTA, n, s4))) return rc;
  return deliver_s4(s4, n, out_s4_host, frag);
}
int qemb_df_create(int naux, const double* j2c, qemb_df_t* out) {
  if (naux <= 0 || !j2c || !out) { set_error("qemb_df_create: bad arguments"); return QEMB_ERR_ARG; }
  DfContext* d = new DfContext();
  int rc = d->set_metric(naux, j2c);
  if (rc) { delete d; return rc; }
  *out = d;
  return QEMB_OK;
}
int qemb_lpq_upload(const double* L, int naux, qemb_df_t* out) {
  if (naux <= 0 || !L || !out) { set_error("qemb_lpq_upload: bad arguments"); return QEMB_ERR_ARG; }
  DfContext* d = new DfContext();
  int rc = d->set_cholesky_factor(naux, L);
  if (rc) { delete d; return rc; }
  *out = d;
  return QEMB_OK;
}
int qemb_df_create_pbc(int naux, const double* j2c, qemb_df_t* out, int* ischol) {
  if (naux <= 0 || !j2c || !out) { set_error("qemb_df_create_pbc: bad arguments"); return QEMB_ERR_ARG; }
  DfContext* d = new DfContext();
  int rc = d->set_metric_pbc(naux, j2c, ischol);
  if (rc) { delete d; return rc; }
  *out = d;
  return QEMB_OK;
}
int qemb_df_alloc_ints(qemb_df_t df, int N) {
  if (!df) { set_error("qemb_df_alloc_ints: null handle"); return QEMB_ERR_ARG; }
  return reinterpret_cast<DfContext*>(df)->alloc_ints(N);
}
int qemb_df_add_pw_block(qemb_df_t df, int nG, const double* F_re, const double* F_im, const double* pw_re, const double* pw_im) {
  if (!df) { set_error("qemb_df_add_pw_block: null handle"); return QEMB_ERR_ARG; }
  return reinterpret_cast<DfContext*>(df)->add_pw_block(nG, F_re, F_im, pw_re, pw_im);
}
int qemb_df_add_rs_block(qemb_df_t df, int p0, int p1, const double* block) {
  if (!df) { set_error("qemb_df_add_rs_block: null handle"); return QEMB_ERR_ARG; }
  return reinterpret_cast<DfContext*>(df)->add_rs_block(p0, p1, block);
}
int qemb_df_pw_imag_absmax(qemb_df_t df, double* out) {
  if (!df) { set_error("qemb_df_pw_imag_absmax: null handle"); return QEMB_ERR_ARG; }
  return reinterpret_cast<DfContext*>(df)->imag_absmax(out);
}
int qemb_df_pw_select(qemb_df_t df, int part) {
  if (!df) { set_error("qemb_df_pw_select: null handle"); return QEMB_ERR_ARG; }
  return reinterpret_cast<DfContext*>(df)->select_part(part);
}
int qemb_df_jk(qemb_df_t ctx, int N, const double* dm, const double* Cw, int npos, int nneg, int occ_block, double* J_out, double* K_out) {
  if (!ctx) { set_error("qemb_df_jk: null handle"); return QEMB_ERR_ARG; }
  const DfContext* d = reinterpret_cast<const DfContext*>(ctx);
  if (d->N > 0 && N != d->N) { set_error("qemb_df_jk: N = " + std::to_string(N) + ", the context holds N = " + std::to_string(d->N)); return QEMB_ERR_ARG; }
  return d->jk(dm, Cw, npos, nneg, occ_block, J_out, K_out);
}
int qemb_df_jk_bytes(qemb_df_t ctx, int ncol, int occ_block, int64_t* bytes) {
  if (!ctx) { set_error("qemb_df_jk_bytes: null handle"); return QEMB_ERR_ARG; }
  return reinterpret_cast<const DfContext*>(ctx)->jk_bytes(ncol, occ_block, bytes);
}
int qemb_df_jk_mem_limit(qemb_df_t ctx, int64_t bytes) {
  if (!ctx) { set_error("qemb_df_jk_mem_limit: null handle"); return QEMB_ERR_ARG; }
  reinterpret_cast<DfContext*>(ctx)->jk_mem_limit = bytes;
  return QEMB_OK;
}
int qemb_df_free(qemb_df_t df) { delete reinterpret_cast<DfContext*>(df); return QEMB_OK; }

// ---- DF integrals from the basis (int3c.cpp) ----
static std::mutex g_basis_mu;
static std::set<IntBasis*> g_basis_live;      // a freed or foreign handle is an argument error, not a crash
static IntBasis* live_basis(qemb_int_basis_t b, const char* who) {
  std::lock_guard<std::mutex> lk(g_basis_mu);
  IntBasis* p = reinterpret_cast<IntBasis*>(b);
  if (!p || !g_basis_live.count(p)) { set_error(std::string(who) + ": not a live basis handle (null, freed or foreign)"); return nullptr; }
  return p;
}
int qemb_int_basis_create(int n_bf, const void* bf_records, size_t record_bytes, const double* c2s, qemb_int_basis_t* out) {
  if (!out) { set_error("qemb_int_basis_create: bad arguments"); return QEMB_ERR_ARG; }
  if (record_bytes != sizeof(BfRecord)) { set_error("qemb_int_basis_create: record_bytes is " + std::to_string(record_bytes) + ", the record of this library has " + std::to_string(sizeof(BfRecord))); return QEMB_ERR_ARG; }
  IntBasis* b = new IntBasis();
  int rc = b->create(n_bf, reinterpret_cast<const BfRecord*>(bf_records), c2s);
  if (rc) { delete b; return rc; }
  { std::lock_guard<std::mutex> lk(g_basis_mu); g_basis_live.insert(b); }
  *out = b;
  return QEMB_OK;
}
int qemb_int_basis_free(qemb_int_basis_t b) {
  if (!b) return QEMB_OK;
  IntBasis* p = live_basis(b, "qemb_int_basis_free");
  if (!p) return QEMB_ERR_ARG;
  { std::lock_guard<std::mutex> lk(g_basis_mu); g_basis_live.erase(p); }
  delete p;
  return QEMB_OK;
}
int qemb_int3c2e(qemb_int_basis_t basis, qemb_int_basis_t auxbasis, const int64_t* pairs, int64_t n_pairs, int layout, double* out, int out_on_device) {
  IntBasis* o = live_basis(basis, "qemb_int3c2e"); if (!o) return QEMB_ERR_ARG;
  IntBasis* a = live_basis(auxbasis, "qemb_int3c2e"); if (!a) return QEMB_ERR_ARG;
  if (!out) { set_error("qemb_int3c2e: null output"); return QEMB_ERR_ARG; }
  if (out_on_device) return int3c_fill(*o, *a, layout, pairs, n_pairs, out);
  const int64_t N = o->nao, na = a->nao;
  const int64_t sz = layout == INT_LAYOUT_PAIRS ? std::max<int64_t>(n_pairs, 0) * na : layout == INT_LAYOUT_PACKED ? na * (N * (N + 1) / 2) : na * N * N;
  DBuf d;
  QTRY(d.alloc(sz));
  QTRY(int3c_fill(*o, *a, layout, pairs, n_pairs, d));
  return sz > 0 ? dev_d2h(out, d, sizeof(double) * sz) : QEMB_OK;
}
int qemb_int2c2e(qemb_int_basis_t auxbasis, double* out, int out_on_device) {
  IntBasis* a = live_basis(auxbasis, "qemb_int2c2e"); if (!a) return QEMB_ERR_ARG;
  if (!out) { set_error("qemb_int2c2e: null output"); return QEMB_ERR_ARG; }
  if (out_on_device) return int2c_fill(*a, out);
  DBuf d;
  QTRY(d.alloc((int64_t)a->nao * a->nao));
  QTRY(int2c_fill(*a, d));
  return dev_d2h(out, d, sizeof(double) * a->nao * a->nao);
}
int qemb_int1e(qemb_int_basis_t basis, int natm, const double* xyz, const double* Z, double* S_out, double* T_out, double* V_out) {
  IntBasis* o = live_basis(basis, "qemb_int1e"); if (!o) return QEMB_ERR_ARG;
  return int1e_fill(*o, natm, xyz, Z, S_out, T_out, V_out);
}
int qemb_int1e_dipole(qemb_int_basis_t basis, const double* origin, double* out) {
  IntBasis* o = live_basis(basis, "qemb_int1e_dipole"); if (!o) return QEMB_ERR_ARG;
  return int1e_dipole_fill(*o, origin, out);
}
// ---- four-centre AO integrals from the basis (int4c.cpp) ----
int qemb_int4c2e(qemb_int_basis_t basis, int sym, double thresh, double* out, int out_on_device) {
  IntBasis* o = live_basis(basis, "qemb_int4c2e"); if (!o) return QEMB_ERR_ARG;
  if (!out) { set_error("qemb_int4c2e: null output"); return QEMB_ERR_ARG; }
  QTRY(int4c_guard(*o, sym, !out_on_device, "qemb_int4c2e"));
  if (out_on_device) return int4c_fill(*o, sym, thresh, out);
  const int64_t sz = int4c_out_words(o->nao, sym);
  DBuf d;
  QTRY(d.alloc(sz));
  QTRY(int4c_fill(*o, sym, thresh, d));
  return dev_d2h(out, d, sizeof(double) * sz);
}
int qemb_int4c_mem_limit(qemb_int_basis_t basis, int64_t bytes) {
  IntBasis* o = live_basis(basis, "qemb_int4c_mem_limit"); if (!o) return QEMB_ERR_ARG;
  o->int4c_mem_limit = bytes;
  return QEMB_OK;
}
int qemb_int4c_stats(qemb_int_basis_t basis, int64_t* n_quartets, int64_t* n_screened) {
  IntBasis* o = live_basis(basis, "qemb_int4c_stats"); if (!o) return QEMB_ERR_ARG;
  if (n_quartets) *n_quartets = o->int4c_stats[0];
  if (n_screened) *n_screened = o->int4c_stats[1];
  return QEMB_OK;
}
int qemb_int_jk_direct(qemb_int_basis_t basis, const double* dm, double thresh, double* J, double* K, int io_on_device) {
  IntBasis* o = live_basis(basis, "qemb_int_jk_direct"); if (!o) return QEMB_ERR_ARG;
  return int4c_jk_direct(*o, dm, thresh, J, K, io_on_device);
}
int qemb_int_jk_direct_bytes(qemb_int_basis_t basis, int64_t* bytes) {
  IntBasis* o = live_basis(basis, "qemb_int_jk_direct_bytes"); if (!o) return QEMB_ERR_ARG;
  if (!bytes) { set_error("qemb_int_jk_direct_bytes: bad arguments"); return QEMB_ERR_ARG; }
  *bytes = int4c_jk_bytes(*o);
  return QEMB_OK;
}
int qemb_int4c_tile_stats(qemb_int_basis_t basis, int64_t* n_visited, int64_t* n_skipped) {
  IntBasis* o = live_basis(basis, "qemb_int4c_tile_stats"); if (!o) return QEMB_ERR_ARG;
  if (n_visited) *n_visited = o->int4c_tiles[0];
  if (n_skipped) *n_skipped = o->int4c_tiles[1];
  return QEMB_OK;
}
int qemb_ao2mo_direct_bytes(qemb_int_basis_t basis, int nfrag, const int* n, int64_t tile_pairs, int64_t* bytes) {
  IntBasis* o = live_basis(basis, "qemb_ao2mo_direct_bytes"); if (!o) return QEMB_ERR_ARG;
  return int4c_ao2mo_direct_bytes(*o, nfrag, n, tile_pairs, bytes);
}
int qemb_ao2mo_direct(qemb_int_basis_t basis, int nfrag, const double* const* TA, const int* n, double* const* out_s4_host, const qemb_frag_t* frags, int64_t tile_pairs,
                      double thresh) {
  IntBasis* o = live_basis(basis, "qemb_ao2mo_direct"); if (!o) return QEMB_ERR_ARG;
  if (nfrag <= 0 || !n) { set_error("qemb_ao2mo_direct: need at least one fragment"); return QEMB_ERR_ARG; }
  if (frags)
    for (int f = 0; f < nfrag; ++f)
      if (frags[f] && FRAG(frags[f])->n() != n[f]) { set_error("qemb_ao2mo_direct: fragment handle " + std::to_string(f) + " has a different n"); return QEMB_ERR_ARG; }
  std::vector<DBuf> g;
  QTRY(int4c_ao2mo_direct(*o, nfrag, TA, n, tile_pairs, thresh, g));
  for (int f = 0; f < nfrag; ++f) QTRY(deliver_s4(g[(size_t)f], n[f], out_s4_host ? out_s4_host[f] : nullptr, frags ? frags[f] : nullptr));
  return QEMB_OK;
}
int qemb_op_int4c_tile(qemb_int_basis_t basis, const int32_t* pairs_r, int64_t n_r, const int32_t* pairs_s, int64_t n_s, double thresh, double* out_host) {
  IntBasis* o = live_basis(basis, "qemb_op_int4c_tile"); if (!o) return QEMB_ERR_ARG;
  return int4c_tile(*o, pairs_r, n_r, pairs_s, n_s, thresh, out_host);
}
int qemb_aoeri_from_basis(qemb_int_basis_t basis, double thresh, qemb_aoeri_t* out) {
  IntBasis* o = live_basis(basis, "qemb_aoeri_from_basis"); if (!o) return QEMB_ERR_ARG;
  if (!out) { set_error("qemb_aoeri_from_basis: bad arguments"); return QEMB_ERR_ARG; }
  QTRY(int4c_guard(*o, 4, true, "qemb_aoeri_from_basis"));
  AoEri* a = new AoEri();
  a->N = o->nao;
  int rc = a->s4.alloc(int4c_out_words(o->nao, 4));
  if (!rc) rc = int4c_fill(*o, 4, thresh, a->s4);      // written in place by the kernels: the operand of ao2mo_dense
  if (rc) { delete a; return rc; }
  *out = a;
  return QEMB_OK;
}
int qemb_df_create_empty(qemb_df_t* out) {
  if (!out) { set_error("qemb_df_create_empty: bad arguments"); return QEMB_ERR_ARG; }
  *out = new DfContext();
  return QEMB_OK;
}
static int df_metric_from_basis(DfContext* d, IntBasis* a) {
  DBuf J;
  QTRY(J.alloc((int64_t)a->nao * a->nao));
  QTRY(int2c_fill(*a, J));
  return d->set_metric_from_device(a->nao, std::move(J));
}
int qemb_df_set_ints_from_basis(qemb_df_t df, qemb_int_basis_t basis, qemb_int_basis_t auxbasis) {
  if (!df) { set_error("qemb_df_set_ints_from_basis: null handle"); return QEMB_ERR_ARG; }
  IntBasis* o = live_basis(basis, "qemb_df_set_ints_from_basis"); if (!o) return QEMB_ERR_ARG;
  IntBasis* a = live_basis(auxbasis, "qemb_df_set_ints_from_basis"); if (!a) return QEMB_ERR_ARG;
  DfContext* d = reinterpret_cast<DfContext*>(df);
  QTRY(df_metric_from_basis(d, a));
  QTRY(d->begin_ints_Lpq(o->nao));
  return int3c_fill(*o, *a, INT_LAYOUT_LPQ, nullptr, 0, d->Lpq);
}
// ---- Cholesky-decomposed AO integrals (int4c.cpp: int4c_cholesky) ----
int qemb_int_cholesky(qemb_int_basis_t basis, double tol, double span, int64_t panel_pairs, int64_t max_rank, double* out_packed_host, int64_t* rank) {
  IntBasis* o = live_basis(basis, "qemb_int_cholesky"); if (!o) return QEMB_ERR_ARG;
  return int4c_cholesky(*o, tol, span, panel_pairs, max_rank, out_packed_host, rank);
}
int qemb_int_cholesky_bytes(qemb_int_basis_t basis, int64_t panel_pairs, int64_t max_rank, int64_t* bytes) {
  IntBasis* o = live_basis(basis, "qemb_int_cholesky_bytes"); if (!o) return QEMB_ERR_ARG;
  return int4c_cholesky_bytes(*o, panel_pairs, max_rank, bytes);
}
int qemb_int_cholesky_stats(qemb_int_basis_t basis, double* out4) {
  IntBasis* o = live_basis(basis, "qemb_int_cholesky_stats"); if (!o) return QEMB_ERR_ARG;
  if (!out4) { set_error("qemb_int_cholesky_stats: bad arguments"); return QEMB_ERR_ARG; }
  for (int k = 0; k < 3; ++k) out4[k] = (double)o->cd_stats[k];
  out4[3] = o->cd_dmax;
  return QEMB_OK;
}
int qemb_df_set_ints_from_cholesky(qemb_df_t df, qemb_int_basis_t basis, double tol, double span, int64_t panel_pairs, int64_t max_rank) {
  if (!df) { set_error("qemb_df_set_ints_from_cholesky: null handle"); return QEMB_ERR_ARG; }
  IntBasis* o = live_basis(basis, "qemb_df_set_ints_from_cholesky"); if (!o) return QEMB_ERR_ARG;
  return int4c_cholesky_to_df(*o, tol, span, panel_pairs, max_rank, *reinterpret_cast<DfContext*>(df));
}
// the op-level hooks of the decomposition's own kernels: host arrays in and out
int qemb_op_cd_panel_factor(int n, const double* A_host, double thr, double* T_host, int32_t* piv_host, int32_t* rank, int* in_lds) {
  if (n <= 0 || !A_host || !T_host || !piv_host || !rank) { set_error("qemb_op_cd_panel_factor: bad arguments"); return QEMB_ERR_ARG; }
  DBuf A, T, work, ib;
  QTRY(A.alloc((int64_t)n * n)); QTRY(T.alloc((int64_t)n * n)); QTRY(work.alloc(n)); QTRY(ib.alloc(n + 2));
  int32_t *srow = reinterpret_cast<int32_t*>(ib.p), *piv = srow + n, *rk = piv + n;
  std::vector<int32_t> id((size_t)n);
  for (int c = 0; c < n; ++c) id[(size_t)c] = c;
  QTRY(dev_h2d(A, A_host, sizeof(double) * n * n)); QTRY(dev_h2d(srow, id.data(), sizeof(int32_t) * n));
  QTRY(dev_fill(T, (int64_t)n * n, 0.0));
  if (int rc = dev_cd_panel_factor(A, n, srow, n, thr, nullptr, T, piv, rk, work)) { dev_sync(); return rc; }
  QTRY(dev_d2h(rank, rk, sizeof(int32_t))); QTRY(dev_d2h(piv_host, piv, sizeof(int32_t) * n)); QTRY(dev_d2h(T_host, T, sizeof(double) * n * n));
  if (in_lds) *in_lds = cd::panel_in_lds(n) ? 1 : 0;
  return dev_sync();
}
int qemb_op_cd_diag_update(int64_t np, int r, const double* Lnew_host, const int32_t* pivrow_host, double* d_host, int64_t nsp, const int32_t* row0_host, const int32_t* cnt_host,
                           double* spmax_host, double* dmax_host) {
  if (np <= 0 || r < 0 || (r > 0 && (!Lnew_host || !pivrow_host)) || !d_host || nsp <= 0 || !row0_host || !cnt_host || !spmax_host || !dmax_host) {
    set_error("qemb_op_cd_diag_update: bad arguments"); return QEMB_ERR_ARG;
  }
  for (int64_t w = 0; w < nsp; ++w)
    if (row0_host[w] < 0 || cnt_host[w] < 0 || (int64_t)row0_host[w] + cnt_host[w] > np) { set_error("qemb_op_cd_diag_update: a shell pair leaves the diagonal"); return QEMB_ERR_ARG; }
  for (int k = 0; k < r; ++k)
    if (pivrow_host[k] < 0 || pivrow_host[k] >= np) { set_error("qemb_op_cd_diag_update: a pivot row leaves the diagonal"); return QEMB_ERR_ARG; }
  const int64_t nb = cd::pair_max_partials(nsp);
  DBuf Ln, d, red, ib;
  QTRY(Ln.alloc(std::max<int64_t>(1, r * np))); QTRY(d.alloc(np)); QTRY(red.alloc(1 + nsp + nb)); QTRY(ib.alloc(nsp + r + 2));
  int32_t *row0 = reinterpret_cast<int32_t*>(ib.p), *cnt = row0 + nsp, *srow = cnt + nsp, *piv = srow + r;      // srow = the pivot rows, piv = 0 .. r - 1
  std::vector<int32_t> id((size_t)r);
  for (int k = 0; k < r; ++k) id[(size_t)k] = k;
  QTRY(dev_h2d(d, d_host, sizeof(double) * np)); QTRY(dev_h2d(row0, row0_host, sizeof(int32_t) * nsp)); QTRY(dev_h2d(cnt, cnt_host, sizeof(int32_t) * nsp));
  if (r > 0) { QTRY(dev_h2d(Ln, Lnew_host, sizeof(double) * r * np)); QTRY(dev_h2d(srow, pivrow_host, sizeof(int32_t) * r)); QTRY(dev_h2d(piv, id.data(), sizeof(int32_t) * r)); }
  if (int rc = dev_cd_diag_update(np, r, Ln, np, piv, srow, d, nsp, row0, cnt, red.p + 1, red.p + 1 + nsp, red.p)) { dev_sync(); return rc; }
  QTRY(dev_d2h(d_host, d, sizeof(double) * np)); QTRY(dev_d2h(dmax_host, red, sizeof(double))); QTRY(dev_d2h(spmax_host, red.p + 1, sizeof(double) * nsp));
  return dev_sync();
}
int qemb_op_cd_permute(int64_t M, int64_t N, const double* L_host, const int32_t* pos_host, int full, double* out_host) {
  const int64_t np = N * (N + 1) / 2;
  if (M <= 0 || N <= 0 || N > 32767 || !L_host || !pos_host || !out_host) { set_error("qemb_op_cd_permute: bad arguments"); return QEMB_ERR_ARG; }
  for (int64_t k = 0; k < np; ++k)
    if (pos_host[k] < 0 || pos_host[k] >= np) { set_error("qemb_op_cd_permute: a table entry leaves the row"); return QEMB_ERR_ARG; }
  const int64_t nout = full ? M * N * N : M * np;
  DBuf L, out, ib;
  QTRY(L.alloc(M * np)); QTRY(out.alloc(nout)); QTRY(ib.alloc(np / 2 + 1));
  int32_t* pos = reinterpret_cast<int32_t*>(ib.p);
  QTRY(dev_h2d(L, L_host, sizeof(double) * M * np)); QTRY(dev_h2d(pos, pos_host, sizeof(int32_t) * np));
  if (int rc = full ? dev_cd_unpack(M, N, L, np, pos, out) : dev_cd_gather_cols(M, np, L, np, pos, out, np)) { dev_sync(); return rc; }
  QTRY(dev_d2h(out_host, out, sizeof(double) * nout));
  return dev_sync();
}
int qemb_op_df_get_ints(qemb_df_t df, double* out_host, int* identity_metric) {
  if (!df || !out_host) { set_error("qemb_op_df_get_ints: bad arguments"); return QEMB_ERR_ARG; }
  DfContext* d = reinterpret_cast<DfContext*>(df);
  if (!d->Lpq.p) { set_error("qemb_op_df_get_ints: the context holds no dense [naux][N][N] tensor"); return QEMB_ERR_ARG; }
  if (identity_metric) *identity_metric = d->identity_metric ? 1 : 0;
  return dev_d2h(out_host, d->Lpq, sizeof(double) * (int64_t)d->naux * d->N * d->N);
}
int qemb_df_set_ints_semisparse_from_basis(qemb_df_t df, qemb_int_basis_t basis, qemb_int_basis_t auxbasis, int64_t n_unique, const int64_t* pairs,
                                           const int64_t* reach_ptr, const int32_t* reach_nu, const int64_t* reach_off) {
  if (!df) { set_error("qemb_df_set_ints_semisparse_from_basis: null handle"); return QEMB_ERR_ARG; }
  IntBasis* o = live_basis(basis, "qemb_df_set_ints_semisparse_from_basis"); if (!o) return QEMB_ERR_ARG;
  IntBasis* a = live_basis(auxbasis, "qemb_df_set_ints_semisparse_from_basis"); if (!a) return QEMB_ERR_ARG;
  if (n_unique > 0 && !pairs) { set_error("qemb_df_set_ints_semisparse_from_basis: null pair list"); return QEMB_ERR_ARG; }
  DfContext* d = reinterpret_cast<DfContext*>(df);
  QTRY(df_metric_from_basis(d, a));
  QTRY(d->begin_ints_semisparse(o->nao, n_unique, reach_ptr, reach_nu, reach_off));
  if (n_unique == 0) return QEMB_OK;
  QTRY(dev_fill(d->Usp, n_unique * a->nao, 0.0));      // a row the pair list does not name stays zero rather than undefined
  return int3c_fill(*o, *a, INT_LAYOUT_PAIRS, pairs, n_unique, d->Usp);
}
int qemb_df_set_ints(qemb_df_t df, int N, const double* ints, int layout) {
  if (!df || !ints || N <= 0) { set_error("qemb_df_set_ints: bad arguments"); return QEMB_ERR_ARG; }
  DfContext* d = reinterpret_cast<DfContext*>(df);
  if (layout == 0) return d->set_ints_pqL(N, ints);
  if (layout == 1) return d->set_ints_Lpq(N, ints);
  if (layout == 2) return d->set_ints_packed(N, ints);
  set_error("qemb_df_set_ints: layout must be 0, 1 or 2");
  return QEMB_ERR_ARG;
}
int qemb_df_set_ints_semisparse(qemb_df_t df, int N, int64_t n_unique, const double* unique_dense_data, const int64_t* reach_ptr,
                                const int32_t* reach_nu, const int64_t* reach_off) {
  if (!df) { set_error("qemb_df_set_ints_semisparse: null handle"); return QEMB_ERR_ARG; }
  return reinterpret_cast<DfContext*>(df)->set_ints_semisparse(N, n_unique, unique_dense_data, reach_ptr, reach_nu, reach_off);
}
int qemb_df_transform_screened(qemb_df_t df, const double* TA, int n, const double* S_abs, double MO_coeff_epsilon,
                               double* out_s4_host, qemb_frag_t frag) {
  if (!df || !TA || !S_abs) { set_error("qemb_df_transform_screened: null argument"); return QEMB_ERR_ARG; }
  DfContext* d = reinterpret_cast<DfContext*>(df);
  DBuf dTA, dS, s4;
  int rc;
  if ((rc = dTA.alloc((int64_t)d->N * n)) || (rc = dS.alloc((int64_t)d->N * d->N))) return rc;
  if ((rc = dev_h2d(dTA, TA, sizeof(double) * d->N * n)) || (rc = dev_h2d(dS, S_abs, sizeof(double) * d->N * d->N))) return rc;
  if ((rc = s4.alloc(((int64_t)n * (n + 1) / 2) * ((int64_t)n * (n + 1) / 2)))) return rc;
  DBuf bb;
  if ((rc = d->transform(dTA, n, s4, dS, MO_coeff_epsilon, frag ? &bb : nullptr))) return rc;
  return deliver_s4(s4, n, out_s4_host, frag, &bb, d->naux);
}
// the fitted factor alone (no bb^T bb product): the fragment then lives on it (Fragment::adopt_df_only)
static int df_transform_factor(qemb_df_t df, const double* TA, int n, const double* S_abs, double eps, qemb_frag_t frag) {
  if (!df || !TA || !frag) { set_error("qemb_df_transform_factor: null argument"); return QEMB_ERR_ARG; }
  DfContext* d = reinterpret_cast<DfContext*>(df);
  if (FRAG(frag)->n() != n) { set_error("fragment handle has a different n"); return QEMB_ERR_ARG; }
  DBuf dTA, dS, bb;
  int rc;
  if ((rc = dTA.alloc((int64_t)d->N * n))) return rc;
  if ((rc = dev_h2d(dTA, TA, sizeof(double) * d->N * n))) return rc;
  if (S_abs) {
    if ((rc = dS.alloc((int64_t)d->N * d->N))) return rc;
    if ((rc = dev_h2d(dS, S_abs, sizeof(double) * d->N * d->N))) return rc;
  }
  if ((rc = d->transform(dTA, n, nullptr, S_abs ? dS.p : nullptr, eps, &bb))) return rc;
  return FRAG(frag)->adopt_df_only(std::move(bb), d->naux);
}
int qemb_df_transform_factor(qemb_df_t df, const double* TA, int n, qemb_frag_t frag) { return df_transform_factor(df, TA, n, nullptr, 0.0, frag); }
int qemb_df_transform_screened_factor(qemb_df_t df, const double* TA, int n, const double* S_abs, double MO_coeff_epsilon, qemb_frag_t frag) {
  if (!S_abs) { set_error("qemb_df_transform_screened_factor: null argument"); return QEMB_ERR_ARG; }
  return df_transform_factor(df, TA, n, S_abs, MO_coeff_epsilon, frag);
}
int qemb_df_transform(qemb_df_t df, const double* TA, int n, double* out_s4_host, qemb_frag_t frag) {
  if (!df || !TA) { set_error("qemb_df_transform: null argument"); return QEMB_ERR_ARG; }
  DfContext* d = reinterpret_cast<DfContext*>(df);
  DBuf dTA, s4;
  int rc;
  if ((rc = dTA.alloc((int64_t)d->N * n))) return rc;
  if ((rc = dev_h2d(dTA, TA, sizeof(double) * d->N * n))) return rc;
  if ((rc = s4.alloc(((int64_t)n * (n + 1) / 2) * ((int64_t)n * (n + 1) / 2)))) return rc;
  DBuf bb;
  if ((rc = d->transform(dTA, n, s4, nullptr, 0.0, frag ? &bb : nullptr))) return rc;
  return deliver_s4(s4, n, out_s4_host, frag, &bb, d->naux);
}

// ---------------------------------------------------------------- k-point DF (periodic) ------------
#define KDF(k) (reinterpret_cast<KdfContext*>(k))
int qemb_kdf_create(int nk, int naux, int nao, const int* qclass, const int* qconj, qemb_kdf_t* out) {
  if (!out) { set_error("qemb_kdf_create: bad arguments"); return QEMB_ERR_ARG; }
  KdfContext* k = new KdfContext();
  int rc = k->create(nk, naux, nao, qclass, qconj);
  if (rc) { delete k; return rc; }
  *out = k;
  return QEMB_OK;
}
int qemb_kdf_set_pair(qemb_kdf_t kdf, int ki, int kj, const double* L) {
  if (!kdf) { set_error("qemb_kdf_set_pair: null handle"); return QEMB_ERR_ARG; }
  return KDF(kdf)->set_pair(ki, kj, L);
}
int qemb_kdf_transform(qemb_kdf_t kdf, const double* TA_k, int n, double* out_s4_host, qemb_frag_t frag, int factor_only) {
  if (!kdf) { set_error("qemb_kdf_transform: null handle"); return QEMB_ERR_ARG; }
  return KDF(kdf)->transform(TA_k, n, out_s4_host, FRAG(frag), factor_only);
}
int qemb_kdf_free(qemb_kdf_t kdf) { delete KDF(kdf); return QEMB_OK; }
int qemb_kdf_guard(int nk, int naux, int nao, int n, int n_kept, int with_block, int64_t limit_bytes) {
  if (nk <= 0 || naux <= 0 || nao <= 0 || n <= 0 || n_kept <= 0 || n_kept > nk) { set_error("qemb_kdf_guard: bad arguments"); return QEMB_ERR_ARG; }
  return KdfContext::guard(nk, naux, nao, KdfContext::resident_bytes(nk, naux, nao, n_kept), KdfContext::work_bytes(nk, naux, nao, n, n_kept, with_block != 0), limit_bytes);
}

// ---------------------------------------------------------------- Schmidt ---------------------------
int qemb_schmidt(const double* lmo, int N, int nmo, int nocc, const int64_t* frag_idx, int n_f, double thr, double* TA, int ld,
                 int* n_b, int* sweeps) {
  if (!lmo || !frag_idx || !TA || !n_b) { set_error("qemb_schmidt: null argument"); return QEMB_ERR_ARG; }
  return schmidt_eigh(lmo, N, nmo, nocc, frag_idx, n_f, thr, TA, ld, n_b, sweeps);
}
int qemb_schmidt_subspace(const double* lmo, int N, int nmo, int nocc, const int64_t* frag_idx, int n_f, double thr, double* TA,
                          int ld, int* n_b, int* sweeps) {
  if (!lmo || !frag_idx || !TA || !n_b) { set_error("qemb_schmidt_subspace: null argument"); return QEMB_ERR_ARG; }
  return schmidt_subspace(lmo, N, nmo, nocc, frag_idx, n_f, thr, TA, ld, n_b, sweeps);
}
int qemb_schmidt_svd(const double* rdm, int N, const int64_t* frag_idx, int n_f, double thr, double* TA, int ld, int* n_b,
                     int* sweeps) {
  if (!rdm || !frag_idx || !TA || !n_b) { set_error("qemb_schmidt_svd: null argument"); return QEMB_ERR_ARG; }
  return schmidt_svd(rdm, N, frag_idx, n_f, thr, TA, ld, n_b, sweeps);
}
int qemb_nsocc_guess(const double* Cproj, int n, int nocc, double* P, int* nsocc, double* mo) {
  if (!Cproj || !nsocc || !mo) { set_error("qemb_nsocc_guess: null argument"); return QEMB_ERR_ARG; }
  return nsocc_guess(Cproj, n, nocc, P, nsocc, mo);
}
int qemb_abs_overlap_prim(int nsh, const int* l, const double* ex, const double* xyz, const int64_t* cart0, int64_t ncart, int nroots,
                          const double* roots, const double* weights, double* out) {
  if (nsh <= 0 || ncart <= 0 || nroots <= 0 || !l || !ex || !xyz || !cart0 || !roots || !weights || !out) { set_error("qemb_abs_overlap_prim: bad arguments"); return QEMB_ERR_ARG; }
  for (int i = 0; i < nsh; ++i) if (l[i] < 0 || l[i] > 4 || ex[i] <= 0.0) { set_error("qemb_abs_overlap_prim: shells need 0 <= l <= 4 and a positive exponent"); return QEMB_ERR_ARG; }
  DBuf dex, dxyz, droots, dw, dout, dl, dc0;      // (int arrays ride in double-sized buffers)
  int rc;
  if ((rc = dex.alloc(nsh)) || (rc = dxyz.alloc(3 * (int64_t)nsh)) || (rc = droots.alloc(nroots)) || (rc = dw.alloc(nroots)) ||
      (rc = dout.alloc(ncart * ncart)) || (rc = dl.alloc((nsh + 1) / 2 + 1)) || (rc = dc0.alloc(nsh))) return rc;
  if ((rc = dev_h2d(dex, ex, sizeof(double) * nsh)) || (rc = dev_h2d(dxyz, xyz, sizeof(double) * 3 * nsh)) ||
      (rc = dev_h2d(droots, roots, sizeof(double) * nroots)) || (rc = dev_h2d(dw, weights, sizeof(double) * nroots)) ||
      (rc = dev_h2d(dl, l, sizeof(int) * nsh)) || (rc = dev_h2d(dc0, cart0, sizeof(int64_t) * nsh))) return rc;
  if ((rc = dev_fill(dout, ncart * ncart, 0.0))) return rc;
  if ((rc = dev_abs_overlap_prim(nsh, reinterpret_cast<const int*>(dl.p), dex, dxyz, reinterpret_cast<const int64_t*>(dc0.p), ncart, nroots, droots, dw, dout))) return rc;
  return dev_d2h(out, dout, sizeof(double) * ncart * ncart);
}
int qemb_matmul(int64_t M, int64_t N, int64_t K, const double* A, int transA, const double* B, int transB, double* C) {
  DBuf dA, dB, dC;
  int rc;
  if ((rc = dA.alloc(M * K)) || (rc = dB.alloc(K * N)) || (rc = dC.alloc(M * N))) return rc;
  if ((rc = dev_h2d(dA, A, sizeof(double) * M * K)) || (rc = dev_h2d(dB, B, sizeof(double) * K * N))) return rc;
  // transA: A is stored K x M;  transB: B is stored N x K
  rc = gemm(M, N, K, 1.0, dA, transA ? M : K, !transA, dB, transB ? K : N, transB != 0, 0.0, dC, N);
  if (rc) return rc;
  return dev_d2h(C, dC, sizeof(double) * M * N);
}

}  // extern "C"
