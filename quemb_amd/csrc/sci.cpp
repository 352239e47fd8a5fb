// sci.cpp -- the selected CI on the device (sci.h): screen in slabs, sort / unique / difference / merge, the CSR matrix, Davidson on it, the RDMs, the round loop; the second-order correction over ranges of the alpha word.
#include "sci.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>

namespace qemb {
using namespace fci_detail;

namespace {
int64_t pow2_at_least(int64_t m) { int64_t p = 1; while (p < m) p <<= 1; return p; }
int64_t pairs(int64_t m) { return m * (m - 1) / 2; }
int64_t words_for_int32(int64_t count) { return (count + 1) / 2; }      // doubles that hold `count` int32
struct StageClock {      // host wall time of a stage, the device drained at both ends
  double* slot; std::chrono::steady_clock::time_point t0;
  explicit StageClock(double* s) : slot(s) { (void)dev_sync(); t0 = std::chrono::steady_clock::now(); }
  ~StageClock() { (void)dev_sync(); *slot += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};
}  // namespace

int64_t sci_excitations(int n, int nsocc) {
  const int64_t o = nsocc, v = n - nsocc, s = o * v;
  return 2 * s + 2 * pairs(o) * pairs(v) + s * s;
}
int64_t sci_candidate_capacity(int n, int nsocc) { return pow2_at_least(std::max<int64_t>(2 * sci_excitations(n, nsocc), (int64_t)1 << 20)); }
int64_t sci_bytes(int n, int nsocc, int64_t max_det, int max_space) {
  const int64_t n2 = (int64_t)n * n, cap = sci_candidate_capacity(n, nsocc);
  const int64_t spaces = 3 * (16 + 8) * max_det;                                   // V, the joined list (two copies while it grows), the merged space; keys and vectors
  const int64_t cand = cap * (16 + 4 + 8) + kSciSlab * kSciScreenLanes * (4 + 8);    // candidate keys, flags, offsets; lane counts and offsets of a slab
  const int64_t davidson = 8 * (2 * (int64_t)max_space + 4) * max_det;             // basis, images, residual, correction, diagonal, the kept vector
  const int64_t rows = (8 + 4 + 8) * max_det;                                      // row pointers, row counts, run offsets
  return spaces + cand + davidson + rows + 8 * (4 * n2 * n2 + 2 * n2);             // Vao, CC, Vmo and the 2-RDM; h and the 1-RDM
}

int sci_double_bound(int n, const double* V_dev, double* bound) {
  const int64_t n2 = (int64_t)n * n;
  std::vector<double> Vh((size_t)(n2 * n2));
  QTRY(dev_d2h(Vh.data(), V_dev, sizeof(double) * n2 * n2));
  double m = 0.0;
  for (double x : Vh) m = std::max(m, std::fabs(x));
  *bound = 2.0 * m;
  return 0;
}

int sci_screen(int n, int nsocc, const double* h_dev, const double* V_dev, double dbl_bound, const SciSpace& V, double eps, int64_t slab, int64_t cap, int64_t max_new,
               DBuf& joined, int64_t* njoined, double* ms, uint64_t alpha_lo, uint64_t alpha_hi) {
  double unclocked[SCI_T_COUNT] = {0, 0, 0, 0, 0};
  if (!ms) ms = unclocked;
  if (slab <= 0) slab = kSciSlab;
  if (cap <= 0) cap = sci_candidate_capacity(n, nsocc);
  if ((cap & (cap - 1)) || cap < 2 * sci_excitations(n, nsocc)) { set_error("sci_screen: the candidate buffer must be a power of two that holds the excitations of one determinant twice"); return QEMB_ERR_ARG; }
  const int64_t N = V.N;
  const int64_t slab_max = std::min(slab, N);
  slab = slab_max;
  DBuf cand, counts, offs, flags, foffs, Q, P2;
  QTRY(cand.alloc(2 * cap)); QTRY(counts.alloc(words_for_int32(slab * kSciScreenLanes))); QTRY(offs.alloc(slab * kSciScreenLanes + 1));
  QTRY(flags.alloc(words_for_int32(cap))); QTRY(foffs.alloc(cap + 1));
  joined.release();
  int64_t nP = 0, pos = 0;
  while (pos < N && nP <= max_new) {
    const int64_t nd = std::min(slab, N - pos), lanes = nd * kSciScreenLanes;
    int64_t total = 0;
    {
      StageClock clk(&ms[SCI_T_SCREEN]);
      QTRY(dev_sci_screen_count(n, h_dev, V_dev, nd, V.k() + 2 * pos, V.c.p + pos, eps, dbl_bound, (int32_t*)counts.p));
      QTRY(dev_sci_scan(lanes, (const int32_t*)counts.p, (int64_t*)offs.p));
      QTRY(dev_d2h(&total, offs.p + lanes, sizeof(int64_t)));
    }
    // the next slab from this one's yield: as many determinants as fill 3/4 of the buffer at the same rate (the vector is not sorted by magnitude, so the
    // rate drifts: a slab that overflows all the same is counted again at the size its own count gives; one determinant always fits)
    const int64_t fit = total > 0 ? std::max<int64_t>(1, (int64_t)(0.75 * (double)cap * (double)nd / (2.0 * (double)total))) : slab_max;
    if (2 * total > cap) {
      if (nd == 1) { set_error("sci_screen: one determinant emitted more keys than the candidate buffer holds"); return QEMB_ERR_ARG; }
      slab = std::min(fit, nd - 1);
      continue;
    }
    slab = std::min(slab_max, fit);
    if (total > 0) {
      const int64_t m = 2 * total;
      int64_t K = 0;
      { StageClock clk(&ms[SCI_T_SCREEN]); QTRY(dev_sci_screen_emit(n, h_dev, V_dev, nd, V.k() + 2 * pos, V.c.p + pos, eps, dbl_bound, (const int64_t*)offs.p, (uint64_t*)cand.p, alpha_lo, alpha_hi)); }
      StageClock clk(&ms[SCI_T_MERGE]);      // sort, unique, difference and the growth of the joined list
      QTRY(dev_sci_sort(m, pow2_at_least(m), (uint64_t*)cand.p));
      QTRY(dev_sci_flag_new(m, (const uint64_t*)cand.p, N, V.k(), nP, (const uint64_t*)joined.p, (int32_t*)flags.p));
      QTRY(dev_sci_scan(m, (const int32_t*)flags.p, (int64_t*)foffs.p));
      QTRY(dev_d2h(&K, foffs.p + m, sizeof(int64_t)));
      if (K > 0) {
        QTRY(Q.alloc(2 * K));
        QTRY(dev_sci_compact(m, (const uint64_t*)cand.p, (const int32_t*)flags.p, (const int64_t*)foffs.p, (uint64_t*)Q.p));
        if (nP == 0) joined = std::move(Q);
        else {
          QTRY(P2.alloc(2 * (nP + K)));
          QTRY(dev_sci_merge(nP, (const uint64_t*)joined.p, nullptr, K, (const uint64_t*)Q.p, (uint64_t*)P2.p, nullptr));
          QTRY(dev_sync());      // (the lists that go back to the pool below are still being read)
          joined = std::move(P2);
        }
        nP += K;
      }
    }
    pos += nd;
  }
  *njoined = nP;
  return dev_sync();
}

int sci_merge(const SciSpace& V, const uint64_t* joined, int64_t njoined, SciSpace& out) {
  const int64_t N = V.N + njoined;
  QTRY(out.keys.alloc(2 * N)); QTRY(out.c.alloc(N));
  QTRY(dev_sci_merge(V.N, V.k(), V.c.p, njoined, joined, (uint64_t*)out.keys.p, out.c.p));
  out.N = N;
  return 0;
}

int sci_alpha_runs(const uint64_t* keys, int64_t N, DBuf& segd, int64_t* nseg) {
  // on the host: one pass over the downloaded keys
  std::vector<uint64_t> kh((size_t)(2 * N));
  QTRY(dev_d2h(kh.data(), keys, sizeof(uint64_t) * 2 * N));
  std::vector<int64_t> seg;
  for (int64_t k = 0; k < N; ++k) if (k == 0 || kh[(size_t)(2 * k)] != kh[(size_t)(2 * k - 2)]) seg.push_back(k);
  *nseg = (int64_t)seg.size();
  seg.push_back(N);
  QTRY(segd.alloc(*nseg + 1));
  return dev_h2d(segd, seg.data(), sizeof(int64_t) * (*nseg + 1));
}

int sci_build(int n, const double* h_dev, const double* V_dev, const uint64_t* keys, int64_t N, int64_t max_bytes, const std::string& who, SciMatrix& H) {
  DBuf segd, counts;
  int64_t nseg = 0;
  QTRY(sci_alpha_runs(keys, N, segd, &nseg));
  QTRY(counts.alloc(words_for_int32(N)));
  const bool values = h_dev != nullptr;      // (without integrals: row pointers and columns alone, what the RDM pass reads)
  QTRY(H.rowptr.alloc(N + 1));
  if (values) QTRY(H.hdiag.alloc(N));
  QTRY(dev_sci_csr_count(N, keys, nseg, (const int64_t*)segd.p, (int32_t*)counts.p));
  QTRY(dev_sci_scan(N, (const int32_t*)counts.p, (int64_t*)H.rowptr.p));
  int64_t nnz = 0;
  QTRY(dev_d2h(&nnz, H.rowptr.p + N, sizeof(int64_t)));
  H.N = N; H.nnz = nnz;
  if (max_bytes >= 0 && (values ? 12 : 4) * nnz > max_bytes) {
    set_error(who + ": the matrix over " + std::to_string(N) + " determinants stores " + std::to_string(nnz) + " elements, " + std::to_string(12e-9 * (double)nnz) +
              " GB, more than the " + std::to_string(1e-9 * (double)max_bytes) + " GB of device memory left for it");
    return QEMB_ERR_ALLOC;
  }
  QTRY(H.col.alloc(words_for_int32(nnz)));
  if (values) QTRY(H.val.alloc(nnz));
  QTRY(dev_sci_csr_fill(n, h_dev, V_dev, N, keys, nseg, (const int64_t*)segd.p, H.rp(), (int32_t*)H.col.p, values ? H.val.p : nullptr, values ? H.hdiag.p : nullptr));
  return dev_sync();      // (the run offsets and counts go back to the pool on return)
}

// fci_detail::davidson over the CSR product, from the handed-in vector
int sci_davidson(const SciMatrix& H, const SciOptions& opt, double* c, FciResult* res) {
  const int64_t N = H.N;
  if (opt.max_space < 2 || opt.max_cycle < 1 || !(opt.conv_tol > 0.0) || !(opt.lindep >= 0.0)) {
    set_error("sci: need max_space >= 2, max_cycle >= 1, conv_tol > 0 and lindep >= 0"); return QEMB_ERR_ARG;
  }
  double cc = 0.0;
  {
    DBuf scal;
    QTRY(scal.alloc(8));
    std::vector<const double*> self(1, c);
    QTRY(dots(N, c, self, scal, &cc));
  }
  if (!(cc > 0.0)) { set_error("sci_davidson: the start vector is zero"); return QEMB_ERR_ARG; }
  QTRY(axpby(N, 1.0 / std::sqrt(cc), c, 0.0, c));
  auto apply = [&](const double* x, double* y) { return dev_sci_spmv(N, H.rp(), H.ci(), H.val, x, y); };
  QTRY(davidson(N, apply, H.hdiag, opt.conv_tol, opt.max_cycle, opt.max_space, opt.lindep, false, c, res));
  return dev_sync();
}

int sci_rdm12(int n, const uint64_t* keys, int64_t N, const int64_t* rowptr, const int32_t* col, const double* c, int o_cum, double* dm1_host, double* dm2_dev) {
  const int64_t n2 = (int64_t)n * n;
  DBuf d1, tmp;
  QTRY(d1.alloc(n2));
  if (!dm2_dev) { QTRY(tmp.alloc(n2 * n2)); dm2_dev = tmp; }
  QTRY(dev_fill(d1, n2, 0.0)); QTRY(dev_fill(dm2_dev, n2 * n2, 0.0));
  QTRY(dev_sci_rdm(n, N, keys, rowptr, col, c, d1, dm2_dev));
  QTRY(dev_d2h(dm1_host, d1, sizeof(double) * n2));
  symmetrise_dm1(n, dm1_host);
  if (o_cum >= 0) {
    QTRY(dev_h2d(d1, dm1_host, sizeof(double) * n2));
    QTRY(dev_sci_dm2_finish(n, o_cum, d1, dm2_dev));
  }
  return dev_sync();
}

int sci_solve(int n, int nsocc, const double* h_host, const double* V_dev, const SciOptions& opt, int64_t room, SciSpace& V, SciMatrix& H, SciResult* res) {
  const int64_t n2 = (int64_t)n * n;
  *res = SciResult();
  if (n <= 0 || n > kSciMaxOrb || nsocc <= 0 || nsocc >= n) { set_error("sci_solve: need 0 < nsocc < n <= " + std::to_string(kSciMaxOrb)); return QEMB_ERR_ARG; }
  if (!(opt.eps_var > 0.0) || opt.max_round < 1 || opt.max_det < 1) { set_error("sci: need eps_var > 0, max_round >= 1 and max_det >= 1"); return QEMB_ERR_ARG; }
  char head[96];
  snprintf(head, sizeof head, "SCI (n = %d, eps_var = %.3g)", n, opt.eps_var);
  const std::string who = head;
  // ---- h on the device; the bound on every double-excitation element: |(ai|bj) - (aj|bi)| <= 2 max |V|
  DBuf hd;
  QTRY(hd.alloc(n2));
  QTRY(dev_h2d(hd, h_host, sizeof(double) * n2));
  double dbl_bound = 0.0;
  QTRY(sci_double_bound(n, V_dev, &dbl_bound));
  // ---- V0 = {HF}
  {
    const uint64_t hf = nsocc == 64 ? ~(uint64_t)0 : (((uint64_t)1 << nsocc) - 1);
    const uint64_t key[2] = {hf, hf};
    const double one = 1.0;
    QTRY(V.keys.alloc(2)); QTRY(V.c.alloc(1));
    QTRY(dev_h2d(V.keys, key, sizeof key)); QTRY(dev_h2d(V.c, &one, sizeof one));
    V.N = 1;
  }
  auto state = [&](int round) {
    char b[160];
    snprintf(b, sizeof b, " in round %d: %lld determinants, energy so far %.10f", round, (long long)V.N, res->e);
    return std::string(b);
  };
  { StageClock clk(&res->ms[SCI_T_BUILD]); QTRY(sci_build(n, hd, V_dev, V.k(), V.N, room, who, H)); }
  QTRY(dev_d2h(&res->e, H.hdiag, sizeof(double)));
  res->ndet = 1; res->nnz = H.nnz;
  for (int round = 1; round <= opt.max_round; ++round) {
    DBuf joined;
    int64_t njoined = 0;
    QTRY(sci_screen(n, nsocc, hd, V_dev, dbl_bound, V, opt.eps_var, 0, 0, opt.max_det - V.N, joined, &njoined, res->ms));
    if (njoined == 0) { res->converged = true; break; }
    if (V.N + njoined > opt.max_det) {
      set_error(who + state(round) + " and at least " + std::to_string(njoined) + " more to join, beyond max_det = " + std::to_string(opt.max_det));
      return QEMB_ERR_ALLOC;
    }
    SciSpace W;
    { StageClock clk(&res->ms[SCI_T_MERGE]); QTRY(sci_merge(V, (const uint64_t*)joined.p, njoined, W)); QTRY(dev_sync()); }
    V = std::move(W);
    joined.release();
    H = SciMatrix();
    {
      StageClock clk(&res->ms[SCI_T_BUILD]);
      const int rc = sci_build(n, hd, V_dev, V.k(), V.N, room, who + state(round), H);
      if (rc) return rc;
    }
    FciResult fr;
    { StageClock clk(&res->ms[SCI_T_DAVIDSON]); QTRY(sci_davidson(H, opt, V.c, &fr)); }
    res->e = fr.e; res->residual = fr.residual; res->n_apply += fr.n_iter; res->rounds = round;
    res->ndet = V.N; res->nnz = H.nnz;
    if (!fr.converged) res->diag_converged = false;
  }
  return 0;
}

// ---- the second-order correction
int64_t sci_pt2_bytes(int n, int nsocc, int64_t ndet, int64_t max_ext) {
  const int64_t cap = sci_candidate_capacity(n, nsocc);
  const int64_t lists = 16 * (2 * max_ext + 2 * cap) + 8 * max_ext;      // joined (<= max_ext when a slab's yield of <= cap keys is merged into the second copy); contributions
  const int64_t cand = cap * (16 + 4 + 8) + kSciSlab * kSciScreenLanes * (4 + 8);
  return lists + cand + 8 * (ndet + 1) + 8;                                // run starts; the sum
}
int64_t sci_pt2_max_ext(int n, int nsocc, int64_t ndet, int64_t room) {
  const int64_t fixed = sci_pt2_bytes(n, nsocc, ndet, 0);
  return room < fixed ? 0 : (room - fixed) / 40;
}

int sci_pt2(int n, int nsocc, const double* h_dev, const double* V_dev, double dbl_bound, const SciSpace& V, double e_var, double eps_pt, int64_t max_ext, int64_t slab, int64_t cap,
            double* e_pt2, int64_t* n_ext, int* batches, double* ms) {
  double unclocked[SCI_PT2_T_COUNT] = {0, 0, 0};
  if (!ms) ms = unclocked;
  *e_pt2 = 0.0; *n_ext = 0; *batches = 0;
  if (n <= 0 || n > kSciMaxOrb || nsocc <= 0 || nsocc >= n || V.N <= 0) { set_error("sci_pt2: need 0 < nsocc < n <= " + std::to_string(kSciMaxOrb) + " and a space"); return QEMB_ERR_ARG; }
  if (!(eps_pt > 0.0) || max_ext < 1) { set_error("sci_pt2: need eps_pt > 0 and max_ext >= 1"); return QEMB_ERR_ARG; }
  DBuf segd, sum;
  int64_t nseg = 0;
  QTRY(sci_alpha_runs(V.k(), V.N, segd, &nseg));
  QTRY(sum.alloc(1));
  // the ranges still to do, the lowest on top: ascending order, and the sums are added in that order
  std::vector<std::pair<uint64_t, uint64_t>> todo(1, {(uint64_t)0, ~(uint64_t)0});
  double e = 0.0;
  int64_t next = 0;
  int nb = 0;
  while (!todo.empty()) {
    const uint64_t lo = todo.back().first, hi = todo.back().second;
    todo.pop_back();
    DBuf joined;
    int64_t nj = 0;
    double sms[SCI_T_COUNT] = {0, 0, 0, 0, 0};
    QTRY(sci_screen(n, nsocc, h_dev, V_dev, dbl_bound, V, eps_pt, slab, cap, max_ext, joined, &nj, sms, lo, hi));
    ms[SCI_PT2_T_SCREEN] += sms[SCI_T_SCREEN]; ms[SCI_PT2_T_MERGE] += sms[SCI_T_MERGE];
    if (nj > max_ext) {      // too many for one pass: cut at the alpha word in the middle of what joined so far (a word of its own when that is the lowest one)
      if (lo == hi) {
        char b[256];
        snprintf(b, sizeof b, "sci_pt2 (n = %d, eps_pt = %.3g): the alpha word %llx alone has at least %lld determinants outside the space, more than max_ext = %lld; %lld were summed before it",
                 n, eps_pt, (unsigned long long)lo, (long long)nj, (long long)max_ext, (long long)next);
        set_error(b);
        return QEMB_ERR_ALLOC;
      }
      uint64_t mid = 0;
      QTRY(dev_d2h(&mid, joined.p + 2 * (nj / 2), sizeof mid));
      if (mid == lo) { todo.push_back({lo + 1, hi}); todo.push_back({lo, lo}); }
      else { todo.push_back({mid, hi}); todo.push_back({lo, mid - 1}); }
      continue;
    }
    ++nb;
    if (nj == 0) continue;
    StageClock clk(&ms[SCI_PT2_T_ROWS]);
    DBuf contrib;
    double x = 0.0;
    QTRY(contrib.alloc(nj));
    QTRY(dev_sci_pt2_rows(n, h_dev, V_dev, V.N, V.k(), V.c, nseg, (const int64_t*)segd.p, nj, (const uint64_t*)joined.p, e_var, eps_pt, dbl_bound, contrib));
    QTRY(dev_sci_sum(nj, contrib, sum));
    QTRY(dev_d2h(&x, sum, sizeof x));
    e += x; next += nj;
  }
  *e_pt2 = e; *n_ext = next; *batches = nb;
  return dev_sync();
}

}  // namespace qemb
