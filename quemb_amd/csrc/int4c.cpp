// int4c.cpp -- driver of the four-centre AO integrals on the device (see int4c.h): shell pairs per pair class, the pair stage, one launch per canonical class.
#include "int4c.h"
#include "ao2mo.h"
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace qemb {

using int3c::Shell;
using int4c::ClassArgs;
using int4c::JkArgs;
using int4c::PairArgs;
using int4c::PairList;
using int4c::kNPairClass;

namespace {

const int kLa[kNPairClass] = {0, 1, 1, 2, 2, 2}, kLb[kNPairClass] = {0, 0, 1, 0, 1, 2};

// the shell pairs of a set of shells, sorted into the pair classes, with the layout of the pair stage
struct PairPlan {
  std::vector<int32_t> a[kNPairClass], b[kNPairClass];
  std::vector<int64_t> off[kNPairClass];
  int64_t data_words = 0, n_pairs = 0;
  void add(const std::vector<Shell>& sh, int I, int J) {      // I >= J in the caller's order; role A: the larger l
    const bool sw = sh[I].l < sh[J].l;
    const int A = sw ? J : I, B = sw ? I : J, c = int4c::pair_class(sh[A].l, sh[B].l);
    a[c].push_back(A); b[c].push_back(B); off[c].push_back(data_words);
    data_words += (int64_t)sh[A].nprim * sh[B].nprim * int4c::pair_stride(sh[A].l, sh[B].l);
    ++n_pairs;
  }
  int64_t bytes() const { return 8 * data_words + (4 + 4 + 8 + 8) * n_pairs + 8 * 25 * n_pairs + 4096; }      // data, a, b, off, q, the diagonal of the Schwarz pass
};

PairPlan plan_of(const IntBasis& orb) {
  PairPlan p;
  for (int I = 0; I < orb.nshell; ++I)
    for (int J = 0; J <= I; ++J) p.add(orb.shells, I, J);
  return p;
}

int check_orbital(const IntBasis& orb, const char* who) {
  for (int i = 0; i < orb.nshell; ++i)
    if (orb.shells[i].l > int4c::kMaxLOrb) {
      set_error(std::string(who) + ": orbital shell " + std::to_string(i) + " has l = " + std::to_string(orb.shells[i].l) + "; orbital shells beyond d are not supported");
      return QEMB_ERR_UNSUPPORTED;
    }
  return 0;
}

// the plan on the device: index lists, pair stage written
struct DevicePlan {
  DBuf d32, d64, dq, data;
  size_t o_a[kNPairClass], o_b[kNPairClass], o_off[kNPairClass];
  int64_t n[kNPairClass];
  PairList list(int c, bool with_q) const {
    PairList l{};
    l.a = reinterpret_cast<const int32_t*>(d32.p) + o_a[c]; l.b = reinterpret_cast<const int32_t*>(d32.p) + o_b[c];
    l.off = reinterpret_cast<const int64_t*>(d64.p) + o_off[c]; l.q = with_q ? dq.p + o_off[c] : nullptr; l.n = n[c];
    return l;
  }
  int upload(const PairPlan& p) {      // the index lists alone (a plan whose offsets point into another plan's pair stage)
    std::vector<int32_t> i32; std::vector<int64_t> i64;
    for (int c = 0; c < kNPairClass; ++c) {
      n[c] = (int64_t)p.a[c].size();
      o_a[c] = i32.size(); i32.insert(i32.end(), p.a[c].begin(), p.a[c].end());
      o_b[c] = i32.size(); i32.insert(i32.end(), p.b[c].begin(), p.b[c].end());
      o_off[c] = i64.size(); i64.insert(i64.end(), p.off[c].begin(), p.off[c].end());
    }
    QTRY(d32.alloc((int64_t)i32.size() / 2 + 1)); QTRY(d64.alloc((int64_t)i64.size() + 1));
    if (!i32.empty()) QTRY(dev_h2d(d32, i32.data(), sizeof(int32_t) * i32.size()));
    if (!i64.empty()) QTRY(dev_h2d(d64, i64.data(), sizeof(int64_t) * i64.size()));
    return 0;
  }
  int upload_q(const std::vector<double> (&qs)[kNPairClass]) {      // Schwarz factors in the order of the offsets list
    std::vector<double> q;
    for (int c = 0; c < kNPairClass; ++c) q.insert(q.end(), qs[c].begin(), qs[c].end());
    QTRY(dq.alloc((int64_t)q.size() + 1));
    return q.empty() ? 0 : dev_h2d(dq, q.data(), sizeof(double) * q.size());
  }
  int build(const PairPlan& p, const Shell* dsh, const double* dc2s) {
    QTRY(upload(p));
    QTRY(data.alloc(p.data_words));
    for (int c = 0; c < kNPairClass; ++c) {
      if (!n[c]) continue;
      PairArgs g{};
      g.sh = dsh; g.pairs = list(c, false); g.c2s = dc2s; g.data = data;
      QTRY(dev_int4c_pairs(kLa[c], kLb[c], g));
    }
    return 0;
  }
};

// Q = sqrt(max_ab (ab|ab)) per shell pair, from the diagonal quartets evaluated on the device; cached in the basis
int schwarz_factors(IntBasis& orb, const PairPlan& p, const DevicePlan& d) {
  for (int c = 0; c < kNPairClass; ++c) {
    if (orb.schwarz[c].size() == p.a[c].size()) continue;
    const int ncd = (2 * kLa[c] + 1) * (2 * kLb[c] + 1);
    const int64_t n = d.n[c];
    DBuf diag;
    QTRY(diag.alloc(n * ncd));
    ClassArgs g{};
    g.sh = orb.dev(); g.data = d.data; g.bra = g.ket = d.list(c, false); g.same = 1; g.thresh = 0.0; g.out = int4c::kDiag; g.N = orb.nao; g.dst = diag;
    QTRY(dev_int4c_class(kLa[c], kLb[c], kLa[c], kLb[c], g));
    std::vector<double> h((size_t)(n * ncd));
    QTRY(dev_d2h(h.data(), diag, sizeof(double) * h.size()));
    orb.schwarz[c].assign((size_t)n, 0.0);
    for (int64_t k = 0; k < n; ++k) {
      double m = 0.0;
      for (int e = 0; e < ncd; ++e) m = std::max(m, h[(size_t)(k * ncd + e)]);
      orb.schwarz[c][(size_t)k] = std::sqrt(m);
    }
  }
  return 0;
}

}  // namespace

struct Int4cCache {
  PairPlan plan;
  DevicePlan dev;
};

int64_t int4c_work_bytes(const IntBasis& orb) { return plan_of(orb).bytes(); }

int64_t int4c_out_words(int64_t N, int sym) {
  const int64_t np = N * (N + 1) / 2;
  return sym == 8 ? np * (np + 1) / 2 : sym == 4 ? np * np : sym == 1 ? N * N * N * N : -1;
}

int int4c_guard(const IntBasis& orb, int sym, bool with_output, const char* who) {
  if (int4c_out_words(orb.nao, sym) < 0) { set_error(std::string(who) + ": sym must be 1, 4 or 8, not " + std::to_string(sym)); return QEMB_ERR_ARG; }
  QTRY(check_orbital(orb, who));
  size_t free_b = 0, total_b = 0;
  QTRY(dev_mem_info(&free_b, &total_b));
  double room = (double)free_b;
  if (orb.int4c_mem_limit >= 0 && (double)orb.int4c_mem_limit < room) room = (double)orb.int4c_mem_limit;
  const double out_b = with_output ? 8.0 * (double)int4c_out_words(orb.nao, sym) : 0.0, work_b = (double)int4c_work_bytes(orb);
  if (out_b + work_b > room) {
    set_error(std::string(who) + ": with N = " + std::to_string(orb.nao) + " the integrals (sym = " + std::to_string(sym) + ") take " + std::to_string(out_b * 1e-9) +
              " GB and the pair stage " + std::to_string(work_b * 1e-9) + " GB, more than the " + std::to_string(room * 1e-9) + " GB of device memory they may take");
    return QEMB_ERR_ALLOC;
  }
  return 0;
}

int int4c_fill(IntBasis& orb, int sym, double thresh, double* out) {
  if (!out) { set_error("qemb_int4c2e: null output"); return QEMB_ERR_ARG; }
  if (int4c_out_words(orb.nao, sym) < 0) { set_error("qemb_int4c2e: sym must be 1, 4 or 8, not " + std::to_string(sym)); return QEMB_ERR_ARG; }
  if (!(thresh >= 0.0)) { set_error("qemb_int4c2e: the screening threshold must be >= 0"); return QEMB_ERR_ARG; }
  QTRY(check_orbital(orb, "qemb_int4c2e"));
  const PairPlan p = plan_of(orb);
  DevicePlan d;
  QTRY(d.build(p, orb.dev(), orb.dc2s));
  const bool screen = thresh > 0.0;
  if (screen) {
    int rc = schwarz_factors(orb, p, d);
    if (rc) { dev_sync(); return rc; }
    std::vector<double> q;
    for (int c = 0; c < kNPairClass; ++c) q.insert(q.end(), orb.schwarz[c].begin(), orb.schwarz[c].end());      // the order of the offsets list
    QTRY(d.dq.alloc((int64_t)q.size() + 1));
    if (!q.empty()) QTRY(dev_h2d(d.dq, q.data(), sizeof(double) * q.size()));
  }
  orb.int4c_stats[0] = orb.int4c_stats[1] = 0;
  for (int cb = 0; cb < kNPairClass; ++cb)
    for (int ck = 0; ck <= cb; ++ck) {
      if (!d.n[cb] || !d.n[ck]) continue;
      ClassArgs g{};
      g.sh = orb.dev(); g.data = d.data; g.bra = d.list(cb, screen); g.ket = d.list(ck, screen);
      g.same = cb == ck; g.thresh = thresh; g.out = sym; g.N = orb.nao; g.dst = out;
      if (int rc = dev_int4c_class(kLa[cb], kLb[cb], kLa[ck], kLb[ck], g)) { dev_sync(); return rc; }      // earlier launches still read the lists
      orb.int4c_stats[0] += g.same ? d.n[cb] * (d.n[cb] + 1) / 2 : d.n[cb] * d.n[ck];
      if (screen)      // the census of qemb_int4c_stats: a host loop over the quartets of the class pair, O(n_pairs^2) -- part of the call's time when thresh > 0
        for (int64_t i = 0; i < d.n[cb]; ++i)
          for (int64_t j = 0; j < (g.same ? i + 1 : d.n[ck]); ++j)
            if (orb.schwarz[cb][(size_t)i] * orb.schwarz[ck][(size_t)j] < thresh) ++orb.int4c_stats[1];
    }
  return dev_sync();      // the work buffers are released on return
}

namespace {
// lists, pair stage and Schwarz factors of the basis on the device, written by the first direct call (J / K or AO -> fragment transform) and kept
int ensure_cache(IntBasis& orb) {
  if (orb.jk_cache) return 0;
  auto c = std::make_shared<Int4cCache>();
  c->plan = plan_of(orb);
  int rc = c->dev.build(c->plan, orb.dev(), orb.dc2s);
  if (!rc) rc = schwarz_factors(orb, c->plan, c->dev);
  if (!rc) rc = c->dev.upload_q(orb.schwarz);
  if (rc) { dev_sync(); return rc; }
  orb.jk_cache = c;
  return 0;
}
int64_t jk_small_bytes(const IntBasis& orb) { return 8 * (3 * (int64_t)orb.nao * orb.nao + (int64_t)orb.nshell * orb.nshell) + 4096; }      // D, J, K, the shell-block table
}  // namespace

int64_t int4c_jk_bytes(const IntBasis& orb) { return int4c_work_bytes(orb) + jk_small_bytes(orb); }

int int4c_jk_direct(IntBasis& orb, const double* dm, double thresh, double* J, double* K, int io_on_device) {
  const char* who = "qemb_int_jk_direct";
  if (!dm) { set_error(std::string(who) + ": null density"); return QEMB_ERR_ARG; }
  if (!J && !K) { set_error(std::string(who) + ": J and K are both null"); return QEMB_ERR_ARG; }
  if (!(thresh >= 0.0)) { set_error(std::string(who) + ": the screening threshold must be >= 0"); return QEMB_ERR_ARG; }
  QTRY(check_orbital(orb, who));
  // the guard of qemb_int4c2e without an output term; what a cached basis holds already is not asked of the free memory again
  size_t free_b = 0, total_b = 0;
  QTRY(dev_mem_info(&free_b, &total_b));
  const double need = (double)int4c_jk_bytes(orb), fresh = orb.jk_cache ? (double)jk_small_bytes(orb) : need;
  if ((orb.int4c_mem_limit >= 0 && need > (double)orb.int4c_mem_limit) || fresh > (double)free_b) {
    const double room = orb.int4c_mem_limit >= 0 && (double)orb.int4c_mem_limit < (double)free_b ? (double)orb.int4c_mem_limit : (double)free_b;
    set_error(std::string(who) + ": with N = " + std::to_string(orb.nao) + " the pair stage, the lists and the N x N matrices take " + std::to_string(need * 1e-9) +
              " GB, more than the " + std::to_string(room * 1e-9) + " GB of device memory they may take");
    return QEMB_ERR_ALLOC;
  }
  QTRY(ensure_cache(orb));
  const DevicePlan& d = orb.jk_cache->dev;
  const int64_t N = orb.nao, nsh = orb.nshell;
  const bool screen = thresh > 0.0;
  DBuf bD, bJ, bK, btab;
  const double* dD = dm;
  double *dJ = J, *dK = K;
  if (!io_on_device) {
    QTRY(bD.alloc(N * N)); QTRY(dev_h2d(bD, dm, sizeof(double) * N * N)); dD = bD;
    if (J) { QTRY(bJ.alloc(N * N)); dJ = bJ; }
    if (K) { QTRY(bK.alloc(N * N)); dK = bK; }
  }
  std::vector<double> tab;
  if (screen) {
    QTRY(btab.alloc(nsh * nsh));
    QTRY(dev_int4c_dmax(orb.dev(), (int)nsh, N, dD, btab));
    tab.resize((size_t)(nsh * nsh));
    QTRY(dev_d2h(tab.data(), btab, sizeof(double) * tab.size()));      // for the census below
  }
  if (dJ) QTRY(dev_fill(dJ, N * N, 0.0));
  if (dK) QTRY(dev_fill(dK, N * N, 0.0));
  orb.int4c_stats[0] = orb.int4c_stats[1] = 0;
  const PairPlan& p = orb.jk_cache->plan;
  for (int cb = 0; cb < kNPairClass; ++cb)
    for (int ck = 0; ck <= cb; ++ck) {
      if (!d.n[cb] || !d.n[ck]) continue;
      JkArgs g{};
      g.sh = orb.dev(); g.data = d.data; g.bra = d.list(cb, screen); g.ket = d.list(ck, screen);
      g.same = cb == ck; g.thresh = thresh; g.N = N; g.nshell = (int)nsh; g.dm = dD; g.dmax = screen ? btab.p : nullptr; g.J = dJ; g.K = dK;
      if (int rc = dev_int4c_jk_class(kLa[cb], kLb[cb], kLa[ck], kLb[ck], g)) { dev_sync(); return rc; }
      orb.int4c_stats[0] += g.same ? d.n[cb] * (d.n[cb] + 1) / 2 : d.n[cb] * d.n[ck];
      if (screen)      // the census of qemb_int4c_stats: the decision of the items (int4c::jk_screened) repeated on the host, O(n_pairs^2) -- part of the call's time when thresh > 0
        for (int64_t i = 0; i < d.n[cb]; ++i)
          for (int64_t j = 0; j < (g.same ? i + 1 : d.n[ck]); ++j)
            if (int4c::jk_screened(thresh, orb.schwarz[cb][(size_t)i], orb.schwarz[ck][(size_t)j], tab.data(), (int)nsh, p.a[cb][(size_t)i], p.b[cb][(size_t)i],
                                   p.a[ck][(size_t)j], p.b[ck][(size_t)j])) ++orb.int4c_stats[1];
    }
  if (dJ) QTRY(dev_mirror_lower(N, dJ, N));
  if (dK) QTRY(dev_mirror_lower(N, dK, N));
  if (!io_on_device) {
    if (J) QTRY(dev_d2h(J, dJ, sizeof(double) * N * N));
    if (K) QTRY(dev_d2h(K, dK, sizeof(double) * N * N));
  }
  return dev_sync();
}

// ---- integral-direct AO -> fragment transform: tiles of the 4-fold packed tensor, consumed by every fragment before the next tile overwrites them ----
namespace {

inline int64_t npair_of(int64_t n) { return n * (n + 1) / 2; }

// the canonical shell pairs (I >= J, I outer: the order of plan_of) cut into slabs of at most tile_pairs AO pairs; a slab holds whole shell pairs, so the shell
// pairs of a slab are ONE sub-range [first, first + cnt) of each class list of the plan -- no list is written for a slab
struct Slab {
  int64_t first[kNPairClass], cnt[kNPairClass];
  int64_t rows = 0, c0 = 0;      // AO pairs of the slab; its first entry in the (mu, nu) tables
  double qmax = 0.0;             // largest Schwarz factor (filled when screening)
};
struct TileLayout {
  std::vector<Slab> slabs;
  std::vector<int32_t> pos, mu, nu;      // pos[ij]: row of the AO pair inside its slab; (mu, nu)[c0 + row]: the AO pair of a row
  int64_t max_rows = 0;
};

// the AO pairs of shell pair (I, J), I >= J, in increasing pair index: f(mu, nu)
template <class F>
void for_ao_pairs(const Shell& A, const Shell& B, bool same, F f) {
  for (int a = 0; a < 2 * A.l + 1; ++a)
    for (int b = 0; b < (same ? a + 1 : 2 * B.l + 1); ++b) f(A.ao0 + a, B.ao0 + b);
}
int64_t n_ao_pairs(const Shell& A, const Shell& B, bool same) {
  const int64_t na = 2 * A.l + 1, nb = 2 * B.l + 1;
  return same ? na * (na + 1) / 2 : na * nb;
}

TileLayout tile_layout(const IntBasis& orb, int64_t tile_pairs, bool with_maps) {
  TileLayout t;
  if (with_maps) { const size_t np = (size_t)npair_of(orb.nao); t.pos.assign(np, -1); t.mu.assign(np, 0); t.nu.assign(np, 0); }
  int64_t seen[kNPairClass] = {0, 0, 0, 0, 0, 0}, c = 0;
  Slab cur;
  auto open = [&]() { cur = Slab(); for (int k = 0; k < kNPairClass; ++k) { cur.first[k] = seen[k]; cur.cnt[k] = 0; } cur.c0 = c; };
  auto close = [&]() { if (cur.rows) { t.slabs.push_back(cur); t.max_rows = std::max(t.max_rows, cur.rows); } };
  open();
  for (int I = 0; I < orb.nshell; ++I)
    for (int J = 0; J <= I; ++J) {
      const Shell &A = orb.shells[I], &B = orb.shells[J];
      const int64_t sz = n_ao_pairs(A, B, I == J);
      if (cur.rows && cur.rows + sz > tile_pairs) { close(); open(); }
      const int cls = int4c::pair_class(std::max(A.l, B.l), std::min(A.l, B.l));
      ++cur.cnt[cls]; ++seen[cls];
      if (with_maps)
        for_ao_pairs(A, B, I == J, [&](int64_t m, int64_t n) {      // shells are in AO order: m >= n
          t.pos[(size_t)(m * (m + 1) / 2 + n)] = (int32_t)(c - cur.c0);
          t.mu[(size_t)c] = (int32_t)m; t.nu[(size_t)c] = (int32_t)n;
          ++c;
        });
      else c += sz;
      cur.rows += sz;
    }
  close();
  return t;
}

// the canonical shell quartets of tile (R, S), R >= S
int64_t tile_quartets(const Slab& R, const Slab& S, bool same) {
  int64_t q = 0;
  for (int cb = 0; cb < kNPairClass; ++cb)
    for (int ck = 0; ck <= cb; ++ck) {
      if (same) q += cb == ck ? R.cnt[cb] * (R.cnt[cb] + 1) / 2 : R.cnt[cb] * R.cnt[ck];
      else q += R.cnt[cb] * S.cnt[ck] + (cb != ck ? S.cnt[cb] * R.cnt[ck] : 0);
    }
  return q;
}

struct TileSide { PairList l[kNPairClass]; };

// One tile: rows = the AO pairs of the shell pairs of R, columns = those of S (R and S the same set, or disjoint).  Every canonical quartet with one pair in R
// and one in S is evaluated once, in the orientation the class kernels need (bra class >= ket class), and lands at [row[.]][col[.]]: every element of the tile
// is written exactly once (a screened quartet as zeros).
int fill_tile(const IntBasis& orb, const double* data, const TileSide& R, const TileSide& S, bool same, const int32_t* row, const int32_t* col, int64_t ld,
              double thresh, double* dst) {
  for (int cb = 0; cb < kNPairClass; ++cb)
    for (int ck = 0; ck <= cb; ++ck) {
      ClassArgs g{};
      g.sh = orb.dev(); g.data = data; g.thresh = thresh; g.out = int4c::kTile; g.N = orb.nao; g.dst = dst; g.row = row; g.col = col; g.ld = ld;
      if (same) {
        if (!R.l[cb].n || !R.l[ck].n) continue;
        g.bra = R.l[cb]; g.ket = R.l[ck]; g.same = cb == ck; g.store = int4c::kTileBoth;
        QTRY(dev_int4c_class(kLa[cb], kLb[cb], kLa[ck], kLb[ck], g));
        continue;
      }
      if (R.l[cb].n && S.l[ck].n) {
        g.bra = R.l[cb]; g.ket = S.l[ck]; g.same = 0; g.store = int4c::kTileAsIs;
        QTRY(dev_int4c_class(kLa[cb], kLb[cb], kLa[ck], kLb[ck], g));
      }
      if (cb != ck && S.l[cb].n && R.l[ck].n) {      // the pair of the higher class sits in the column set: computed as (S|R), stored transposed
        g.bra = S.l[cb]; g.ket = R.l[ck]; g.same = 0; g.store = int4c::kTileTransposed;
        QTRY(dev_int4c_class(kLa[cb], kLb[cb], kLa[ck], kLb[ck], g));
      }
    }
  return 0;
}

TileSide side_of(const DevicePlan& d, const Slab& s, bool with_q) {
  TileSide t;
  for (int c = 0; c < kNPairClass; ++c) {
    PairList l = d.list(c, with_q);
    l.a += s.first[c]; l.b += s.first[c]; l.off += s.first[c]; if (l.q) l.q += s.first[c];
    l.n = s.cnt[c];
    t.l[c] = l;
  }
  return t;
}

struct DirectSizes { int64_t sum_npq2 = 0, sum_ta = 0, npq_max = 0; };
int direct_sizes(const IntBasis& orb, int nfrag, const int* n, const char* who, DirectSizes* z) {
  if (nfrag <= 0 || !n) { set_error(std::string(who) + ": need at least one fragment"); return QEMB_ERR_ARG; }
  for (int f = 0; f < nfrag; ++f) {
    if (n[f] <= 0 || n[f] > orb.nao) { set_error(std::string(who) + ": fragment " + std::to_string(f) + " needs 0 < n <= N"); return QEMB_ERR_ARG; }
    const int64_t npq = npair_of(n[f]);
    z->sum_npq2 += npq * npq; z->sum_ta += (int64_t)orb.nao * n[f]; z->npq_max = std::max(z->npq_max, npq);
  }
  return 0;
}
// what a call holds beside the tile and the three tile-row operands: pair stage and lists, the three tables of the layout, the accumulators, the coefficients
int64_t direct_fixed_bytes(const IntBasis& orb, const DirectSizes& z) { return int4c_work_bytes(orb) + 12 * npair_of(orb.nao) + 8 * (z.sum_npq2 + z.sum_ta) + 4096; }
int64_t direct_tile_bytes(int64_t rows, const DirectSizes& z) { return 8 * (rows * rows + 3 * rows * z.npq_max); }
double direct_room(const IntBasis& orb) {
  size_t free_b = 0, total_b = 0;
  if (dev_mem_info(&free_b, &total_b)) return 0.0;
  double room = (double)free_b;
  if (orb.int4c_mem_limit >= 0 && (double)orb.int4c_mem_limit < room) room = (double)orb.int4c_mem_limit;
  return room;
}
// the default tile: the tile and its operands take at most half of what the fixed part leaves, at most 8192 AO pairs (a 512 MB tile: the products are long
// enough for the GEMM's best rate, and a larger tile saves nothing but launches)
int64_t default_tile_pairs(const IntBasis& orb, const DirectSizes& z) {
  const double avail = 0.5 * (direct_room(orb) - (double)direct_fixed_bytes(orb, z)) / 8.0, m = 1.5 * (double)z.npq_max;
  int64_t t = avail > 0.0 ? (int64_t)(-m + std::sqrt(m * m + avail)) : 1;
  return std::max<int64_t>(1, std::min<int64_t>(t, std::min<int64_t>(npair_of(orb.nao), 8192)));
}

}  // namespace

int int4c_ao2mo_direct_bytes(const IntBasis& orb, int nfrag, const int* n, int64_t tile_pairs, int64_t* bytes) {
  const char* who = "qemb_ao2mo_direct_bytes";
  if (!bytes) { set_error(std::string(who) + ": bad arguments"); return QEMB_ERR_ARG; }
  QTRY(check_orbital(orb, who));
  DirectSizes z;
  QTRY(direct_sizes(orb, nfrag, n, who, &z));
  if (tile_pairs <= 0) tile_pairs = default_tile_pairs(orb, z);
  *bytes = direct_fixed_bytes(orb, z) + direct_tile_bytes(tile_layout(orb, tile_pairs, false).max_rows, z);
  return 0;
}

int int4c_ao2mo_direct(IntBasis& orb, int nfrag, const double* const* TA_host, const int* n, int64_t tile_pairs, double thresh, std::vector<DBuf>& out) {
  const char* who = "qemb_ao2mo_direct";
  if (!TA_host) { set_error(std::string(who) + ": null coefficients"); return QEMB_ERR_ARG; }
  if (!(thresh >= 0.0)) { set_error(std::string(who) + ": the screening threshold must be >= 0"); return QEMB_ERR_ARG; }
  QTRY(check_orbital(orb, who));
  DirectSizes z;
  QTRY(direct_sizes(orb, nfrag, n, who, &z));
  for (int f = 0; f < nfrag; ++f)
    if (!TA_host[f]) { set_error(std::string(who) + ": null coefficients of fragment " + std::to_string(f)); return QEMB_ERR_ARG; }
  if (tile_pairs <= 0) tile_pairs = default_tile_pairs(orb, z);
  const int64_t N = orb.nao;
  TileLayout lay = tile_layout(orb, tile_pairs, true);
  {      // the guard, before anything is allocated; what a cached basis holds already is not asked of the free memory again
    size_t free_b = 0, total_b = 0;
    QTRY(dev_mem_info(&free_b, &total_b));
    const double need = (double)(direct_fixed_bytes(orb, z) + direct_tile_bytes(lay.max_rows, z)), fresh = need - (orb.jk_cache ? (double)int4c_work_bytes(orb) : 0.0);
    if ((orb.int4c_mem_limit >= 0 && need > (double)orb.int4c_mem_limit) || fresh > (double)free_b) {
      set_error(std::string(who) + ": with N = " + std::to_string(N) + ", " + std::to_string(nfrag) + " fragments and tiles of " + std::to_string(lay.max_rows) +
                " AO pairs the call takes " + std::to_string((int64_t)need) + " bytes, more than the " + std::to_string((int64_t)direct_room(orb)) +
                " bytes of device memory it may take");
      return QEMB_ERR_ALLOC;
    }
  }
  QTRY(ensure_cache(orb));
  const DevicePlan& d = orb.jk_cache->dev;
  const bool screen = thresh > 0.0;
  if (screen)
    for (Slab& s : lay.slabs)
      for (int c = 0; c < kNPairClass; ++c)
        for (int64_t k = s.first[c]; k < s.first[c] + s.cnt[c]; ++k) s.qmax = std::max(s.qmax, orb.schwarz[c][(size_t)k]);
  const int64_t np = npair_of(N), mr = lay.max_rows;
  DBuf maps, E, PR, PS, T;
  std::vector<DBuf> dTA((size_t)nfrag);
  out.clear(); out.resize((size_t)nfrag);
  QTRY(maps.alloc(3 * np / 2 + 2));
  int32_t* dpos = reinterpret_cast<int32_t*>(maps.p);
  int32_t *dmu = dpos + np, *dnu = dmu + np;
  QTRY(dev_h2d(dpos, lay.pos.data(), sizeof(int32_t) * np)); QTRY(dev_h2d(dmu, lay.mu.data(), sizeof(int32_t) * np)); QTRY(dev_h2d(dnu, lay.nu.data(), sizeof(int32_t) * np));
  QTRY(E.alloc(mr * mr)); QTRY(PR.alloc(mr * z.npq_max)); QTRY(PS.alloc(mr * z.npq_max)); QTRY(T.alloc(mr * z.npq_max));
  for (int f = 0; f < nfrag; ++f) {
    const int64_t npq = npair_of(n[f]);
    QTRY(dTA[(size_t)f].alloc(N * n[f])); QTRY(dev_h2d(dTA[(size_t)f], TA_host[f], sizeof(double) * N * n[f]));
    QTRY(out[(size_t)f].alloc(npq * npq)); QTRY(dev_fill(out[(size_t)f], npq * npq, 0.0));
  }
  orb.int4c_stats[0] = orb.int4c_stats[1] = 0;
  orb.int4c_tiles[0] = orb.int4c_tiles[1] = 0;
  TimerScope lap(TIMER_AO2MO);
  const int64_t ns = (int64_t)lay.slabs.size();
  for (int64_t r = 0; r < ns; ++r)
    for (int64_t s = 0; s <= r; ++s) {      // a fixed order and no atomics: the same bits run to run
      const Slab &R = lay.slabs[(size_t)r], &S = lay.slabs[(size_t)s];
      const bool same = r == s;
      const int64_t nq = tile_quartets(R, S, same);
      orb.int4c_stats[0] += nq;
      if (screen && R.qmax * S.qmax < thresh) {      // every quartet of the tile is below the threshold: the tile counts as zeros
        orb.int4c_stats[1] += nq; ++orb.int4c_tiles[1];
        continue;
      }
      ++orb.int4c_tiles[0];
      if (int rc = fill_tile(orb, d.data, side_of(d, R, screen), side_of(d, S, screen), same, dpos, dpos, S.rows, thresh, E)) { dev_sync(); return rc; }
      if (screen)      // the census of qemb_int4c_stats, as in int4c_fill: a host loop over the quartets of the tile
        for (int cb = 0; cb < kNPairClass; ++cb)
          for (int ck = 0; ck <= cb; ++ck)
            for (int pass = 0; pass < (same || cb == ck ? 1 : 2); ++pass) {
              const Slab &B = pass ? S : R, &K = pass ? R : S;
              for (int64_t i = B.first[cb]; i < B.first[cb] + B.cnt[cb]; ++i)
                for (int64_t j = K.first[ck]; j < (same && cb == ck ? i + 1 : K.first[ck] + K.cnt[ck]); ++j)
                  if (orb.schwarz[cb][(size_t)i] * orb.schwarz[ck][(size_t)j] < thresh) ++orb.int4c_stats[1];
            }
      const TileRows tr{dmu + R.c0, dnu + R.c0, R.rows}, ts{dmu + S.c0, dnu + S.c0, S.rows};
      for (int f = 0; f < nfrag; ++f)
        if (int rc = ao2mo_tile_accumulate(E, S.rows, tr, ts, same, dTA[(size_t)f], n[f], PR, PS, T, out[(size_t)f])) { dev_sync(); return rc; }
    }
  for (int f = 0; f < nfrag; ++f) QTRY(dev_int4c_add_transpose(npair_of(n[f]), out[(size_t)f]));      // G = A + A^T: the 4-fold packed block, symmetric to the bit
  QTRY(lap.close());
  return dev_sync();      // the lists of the cache and the work buffers were read by the launches
}

int int4c_tile(IntBasis& orb, const int32_t* pr, int64_t nr, const int32_t* ps, int64_t nsp, double thresh, double* out_host) {
  const char* who = "qemb_op_int4c_tile";
  if (!pr || !ps || nr <= 0 || nsp <= 0 || !out_host) { set_error(std::string(who) + ": bad arguments"); return QEMB_ERR_ARG; }
  if (!(thresh >= 0.0)) { set_error(std::string(who) + ": the screening threshold must be >= 0"); return QEMB_ERR_ARG; }
  QTRY(check_orbital(orb, who));
  const int64_t nsh = orb.nshell, np = npair_of(orb.nao);
  // the two sets: canonical shell pairs (I >= J), none twice; the same list on both sides, or no pair in common
  bool same = nr == nsp;
  for (int64_t k = 0; same && k < 2 * nr; ++k) same = pr[k] == ps[k];
  std::vector<char> inR((size_t)npair_of(nsh), 0), inS((size_t)npair_of(nsh), 0);
  for (int side = 0; side < 2; ++side) {
    const int32_t* p = side ? ps : pr;
    std::vector<char>& in = side ? inS : inR;
    for (int64_t k = 0; k < (side ? nsp : nr); ++k) {
      const int64_t I = p[2 * k], J = p[2 * k + 1];
      if (I < 0 || I >= nsh || J < 0 || J > I) { set_error(std::string(who) + ": a shell pair (I, J) needs nshell > I >= J >= 0"); return QEMB_ERR_ARG; }
      if (in[(size_t)(I * (I + 1) / 2 + J)]) { set_error(std::string(who) + ": a shell pair is listed twice"); return QEMB_ERR_ARG; }
      in[(size_t)(I * (I + 1) / 2 + J)] = 1;
      if (side && !same && inR[(size_t)(I * (I + 1) / 2 + J)]) { set_error(std::string(who) + ": the two sets must be the same list or have no shell pair in common"); return QEMB_ERR_ARG; }
    }
  }
  QTRY(ensure_cache(orb));
  const PairPlan& full = orb.jk_cache->plan;
  // class and position in its class list of every canonical shell pair, in the order of plan_of
  std::vector<int> cls((size_t)npair_of(nsh)); std::vector<int64_t> idx((size_t)npair_of(nsh));
  {
    int64_t seen[kNPairClass] = {0, 0, 0, 0, 0, 0};
    for (int64_t I = 0, k = 0; I < nsh; ++I)
      for (int64_t J = 0; J <= I; ++J, ++k) {
        const int la = orb.shells[(size_t)I].l, lb = orb.shells[(size_t)J].l;
        cls[(size_t)k] = int4c::pair_class(std::max(la, lb), std::min(la, lb)); idx[(size_t)k] = seen[cls[(size_t)k]]++;
      }
  }
  PairPlan sub[2];
  std::vector<double> q[2][kNPairClass];
  std::vector<int32_t> map[2];
  int64_t rows[2] = {0, 0};
  for (int side = 0; side < 2; ++side) {
    const int32_t* p = side ? ps : pr;
    map[side].assign((size_t)np, -1);
    for (int64_t k = 0; k < (side ? nsp : nr); ++k) {
      const int64_t I = p[2 * k], J = p[2 * k + 1], w = I * (I + 1) / 2 + J;
      const int c = cls[(size_t)w]; const size_t i = (size_t)idx[(size_t)w];
      sub[side].a[c].push_back(full.a[c][i]); sub[side].b[c].push_back(full.b[c][i]); sub[side].off[c].push_back(full.off[c][i]);
      q[side][c].push_back(orb.schwarz[c][i]);
      for_ao_pairs(orb.shells[(size_t)I], orb.shells[(size_t)J], I == J, [&](int64_t m, int64_t n) { map[side][(size_t)(m * (m + 1) / 2 + n)] = (int32_t)rows[side]++; });
    }
  }
  DevicePlan dl[2];
  DBuf maps, E;
  QTRY(maps.alloc(np + 2));
  int32_t* drow = reinterpret_cast<int32_t*>(maps.p);
  int32_t* dcol = drow + np;
  TileSide side[2];
  for (int k = 0; k < 2; ++k) {
    QTRY(dl[k].upload(sub[k])); QTRY(dl[k].upload_q(q[k]));
    QTRY(dev_h2d(k ? dcol : drow, map[k].data(), sizeof(int32_t) * np));
    for (int c = 0; c < kNPairClass; ++c) side[k].l[c] = dl[k].list(c, thresh > 0.0);
  }
  QTRY(E.alloc(rows[0] * rows[1]));
  if (int rc = fill_tile(orb, orb.jk_cache->dev.data, side[0], side[1], same, drow, dcol, rows[1], thresh, E)) { dev_sync(); return rc; }
  QTRY(dev_d2h(out_host, E, sizeof(double) * rows[0] * rows[1]));
  return dev_sync();
}

int int4c_block(const int l[4], const BfRecord* const rec[4], const double* c2s_host, double* out_host) {
  if (!rec[0] || !rec[1] || !rec[2] || !rec[3] || !c2s_host || !out_host) { set_error("qemb_op_int4c_class: null argument"); return QEMB_ERR_ARG; }
  for (int k = 0; k < 4; ++k)
    if (l[k] < 0 || l[k] > int4c::kMaxLOrb) {
      set_error("qemb_op_int4c_class: unsupported angular class (" + std::to_string(l[0]) + "," + std::to_string(l[1]) + "|" + std::to_string(l[2]) + "," + std::to_string(l[3]) + ")");
      return QEMB_ERR_UNSUPPORTED;
    }
  for (int k = 0; k < 10; ++k)
    if (c2s_host[k] != ((k == 0 || k == 1 || k == 5 || k == 9) ? 1.0 : 0.0)) {
      set_error("qemb_op_int4c_class: the Cartesian -> spherical matrices of l = 0 and l = 1 must be the identity (p functions in x, y, z order)");
      return QEMB_ERR_UNSUPPORTED;
    }
  std::vector<Shell> sh(4);
  for (int k = 0; k < 4; ++k) {
    if (rec[k]->nprim < 1 || rec[k]->nprim > int3c::kMaxPrim) { set_error("qemb_op_int4c_class: 1 to 8 primitives per contraction"); return QEMB_ERR_ARG; }
    sh[k] = Shell{};
    for (int d = 0; d < 3; ++d) sh[k].r[d] = rec[k]->ctr[d];
    sh[k].l = l[k]; sh[k].nprim = rec[k]->nprim; sh[k].ao0 = 0;
    for (int i = 0; i < rec[k]->nprim; ++i) { sh[k].ex[i] = rec[k]->ex[i]; sh[k].co[i] = rec[k]->co[i]; }
  }
  // canonical roles: inside each pair the larger l first, the pair of the higher class as the bra; the block is put back into the caller's order on the host
  int r[4] = {0, 1, 2, 3};
  if (l[0] < l[1]) std::swap(r[0], r[1]);
  if (l[2] < l[3]) std::swap(r[2], r[3]);
  const bool swap_bk = int4c::pair_class(l[r[2]], l[r[3]]) > int4c::pair_class(l[r[0]], l[r[1]]);
  if (swap_bk) { std::swap(r[0], r[2]); std::swap(r[1], r[3]); }
  PairPlan p;      // two pairs, (r0, r1) and (r2, r3): the roles are ordered already (l[r0] >= l[r1]), so PairPlan::add keeps them
  p.add(sh, r[0], r[1]); p.add(sh, r[2], r[3]);
  DBuf dsh, dc, dout;
  int ns[4];
  for (int k = 0; k < 4; ++k) ns[k] = 2 * l[r[k]] + 1;
  const int64_t nout = (int64_t)ns[0] * ns[1] * ns[2] * ns[3];
  QTRY(dsh.alloc(4 * (sizeof(Shell) / sizeof(double)))); QTRY(dc.alloc(int3c::kC2sLen)); QTRY(dout.alloc(nout));
  QTRY(dev_h2d(dsh, sh.data(), sizeof(Shell) * 4)); QTRY(dev_h2d(dc, c2s_host, sizeof(double) * int3c::kC2sLen));
  DevicePlan d;
  QTRY(d.build(p, reinterpret_cast<const Shell*>(dsh.p), dc));
  const int cb = int4c::pair_class(l[r[0]], l[r[1]]), ck = int4c::pair_class(l[r[2]], l[r[3]]);
  ClassArgs g{};
  g.sh = reinterpret_cast<const Shell*>(dsh.p); g.data = d.data; g.bra = d.list(cb, false); g.ket = d.list(ck, false);
  if (cb == ck) { g.bra.n = 1; g.ket.a += 1; g.ket.b += 1; g.ket.off += 1; g.ket.n = 1; }      // both pairs sit in one list: entry 0 the bra, entry 1 the ket
  g.same = 0; g.thresh = 0.0; g.out = int4c::kBlock; g.N = 0; g.dst = dout;
  if (int rc = dev_int4c_class(l[r[0]], l[r[1]], l[r[2]], l[r[3]], g)) { dev_sync(); return rc; }
  std::vector<double> h((size_t)nout);
  QTRY(dev_d2h(h.data(), dout, sizeof(double) * nout));
  // h[(i0, i1, i2, i3)] in canonical roles r -> out[(j0, j1, j2, j3)] in the caller's order: caller's shell r[k] carries index i_k
  int nc[4];
  for (int k = 0; k < 4; ++k) nc[k] = 2 * l[k] + 1;
  int i[4];
  for (i[0] = 0; i[0] < ns[0]; ++i[0]) for (i[1] = 0; i[1] < ns[1]; ++i[1]) for (i[2] = 0; i[2] < ns[2]; ++i[2]) for (i[3] = 0; i[3] < ns[3]; ++i[3]) {
    int j[4];
    for (int k = 0; k < 4; ++k) j[r[k]] = i[k];
    out_host[((j[0] * nc[1] + j[1]) * nc[2] + j[2]) * nc[3] + j[3]] = h[(size_t)(((i[0] * ns[1] + i[1]) * ns[2] + i[2]) * ns[3] + i[3])];
  }
  return 0;
}

}  // namespace qemb
