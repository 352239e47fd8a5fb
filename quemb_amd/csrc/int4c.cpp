// int4c.cpp -- driver of the four-centre AO integrals on the device (see int4c.h): shell pairs per pair class (PairPlan, with the table that says where every
// canonical shell pair sits), the pair stage (DevicePlan), and the four routes -- stored integrals, direct J / K, the direct AO -> fragment transform, the explicit
// tile -- as callers of ONE walk over the canonical class pairs (for_class_pairs: the launches, their quartet count and the tile orientation), ONE census of
// the screened quartets (census, given the screening predicate) and ONE memory guard (mem_guard).  The refusals shared with the DF driver are in int3c.h.
#include "int4c.h"
#include "ao2mo.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
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
  std::vector<int> cls;          // the pair table: class and position in its class list of every pair, in the order it was added (plan_of: I (I + 1) / 2 + J)
  std::vector<int64_t> idx;
  int64_t data_words = 0, n_pairs = 0;
  void add(const std::vector<Shell>& sh, int I, int J) {      // I >= J in the caller's order; role A: the larger l
    const bool sw = sh[I].l < sh[J].l;
    const int A = sw ? J : I, B = sw ? I : J, c = int4c::pair_class(sh[A].l, sh[B].l);
    cls.push_back(c); idx.push_back((int64_t)a[c].size());
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

// the plan on the device: index lists, pair stage written
struct DevicePlan {
  DBuf d32, d64, dq, data;
  size_t o_a[kNPairClass], o_b[kNPairClass], o_off[kNPairClass];
  int64_t n[kNPairClass];
  PairList list(int c, bool with_q, int64_t first = 0, int64_t cnt = -1) const {      // the class list, or its sub-range [first, first + cnt)
    PairList l{};
    l.a = reinterpret_cast<const int32_t*>(d32.p) + o_a[c] + first; l.b = reinterpret_cast<const int32_t*>(d32.p) + o_b[c] + first;
    l.off = reinterpret_cast<const int64_t*>(d64.p) + o_off[c] + first; l.q = with_q ? dq.p + o_off[c] + first : nullptr; l.n = cnt < 0 ? n[c] : cnt;
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

struct PairCache {
  PairPlan plan;
  DevicePlan dev;
};

int64_t int4c_work_bytes(const IntBasis& orb) { return plan_of(orb).bytes(); }

int64_t int4c_out_words(int64_t N, int sym) {
  const int64_t np = N * (N + 1) / 2;
  return sym == 8 ? np * (np + 1) / 2 : sym == 4 ? np * np : sym == 1 ? N * N * N * N : -1;
}

namespace {

// ---- the one walk over the canonical class pairs ----
// A side: per pair class a sub-range [first, first + cnt) of the class lists of a plan (the whole plan, a slab of it, or a list uploaded for one call).
struct Side {
  int64_t first[kNPairClass] = {0, 0, 0, 0, 0, 0}, cnt[kNPairClass] = {0, 0, 0, 0, 0, 0};
};
Side whole(const PairPlan& p) {
  Side s;
  for (int c = 0; c < kNPairClass; ++c) s.cnt[c] = (int64_t)p.a[c].size();
  return s;
}
// One launch of the walk: bra class cb >= ket class ck, the bra range [b0, b0 + bn) and the ket range [k0, k0 + kn) of their class lists.  swapped: the bra
// range is S's and the ket range R's (the pair of the higher class sits in the column set: computed as (S|R), stored transposed).  same: bra and ket are ONE
// range, only the quartets with bra index >= ket index exist.  store: how a tile whose rows are R and whose columns are S receives the launch.
struct Step {
  int cb, ck;
  int64_t b0, bn, k0, kn;
  bool swapped;
  int same, store;
  int64_t quartets() const { return same ? bn * (bn + 1) / 2 : bn * kn; }      // the canonical shell quartets of the launch
};
// Every canonical shell quartet with one pair in R and one in S -- `one`: R and S are the same set (S is not read); otherwise they have no pair in common --
// exactly once, in the orientation the class kernels need: f(step) per non-empty launch, stopping at the first error.
template <class F>
int for_class_pairs(const Side& R, const Side& S, bool one, F f) {
  for (int cb = 0; cb < kNPairClass; ++cb)
    for (int ck = 0; ck <= cb; ++ck)
      for (int pass = 0; pass < (one || cb == ck ? 1 : 2); ++pass) {
        const Side &B = pass ? S : R, &K = one ? R : pass ? R : S;
        if (!B.cnt[cb] || !K.cnt[ck]) continue;
        const Step s{cb, ck, B.first[cb], B.cnt[cb], K.first[ck], K.cnt[ck], pass == 1, one && cb == ck, one ? int4c::kTileBoth : pass ? int4c::kTileTransposed : int4c::kTileAsIs};
        QTRY(f(s));
      }
  return 0;
}
// The census of qemb_int4c_stats: the quartets of a step that screened(cb, i, ck, j) names -- the decision of the items repeated on the host over positions in
// the class lists of the whole plan, O(n_pairs^2): part of the call's time when thresh > 0.
template <class P>
int64_t census(const Step& s, P screened) {
  int64_t n = 0;
  for (int64_t i = s.b0; i < s.b0 + s.bn; ++i)
    for (int64_t j = s.k0; j < (s.same ? i + 1 : s.k0 + s.kn); ++j)
      if (screened(s.cb, i, s.ck, j)) ++n;
  return n;
}
auto schwarz_screened(const IntBasis& orb, double thresh) {
  return [&orb, thresh](int cb, int64_t i, int ck, int64_t j) { return orb.schwarz[cb][(size_t)i] * orb.schwarz[ck][(size_t)j] < thresh; };
}

// ---- the one memory guard ----
// what the four-centre calls may take: min(free device memory, orb.int4c_mem_limit)
struct Room { double free_b = 0.0, room = 0.0; };
int room_of(const IntBasis& orb, Room* r) {
  size_t free_b = 0, total_b = 0;
  QTRY(dev_mem_info(&free_b, &total_b));
  r->free_b = r->room = (double)free_b;
  if (orb.int4c_mem_limit >= 0 && (double)orb.int4c_mem_limit < r->room) r->room = (double)orb.int4c_mem_limit;
  return 0;
}
// Before anything is allocated: a call that takes `need` bytes in all, of which the basis holds `resident` on the device already (not asked of the free memory
// again), is refused when need exceeds the limit or the rest the free memory.  what: what takes the memory, for the message.
int mem_guard(const IntBasis& orb, double need, double resident, const char* who, const std::string& what) {
  Room r;
  QTRY(room_of(orb, &r));
  if (!((orb.int4c_mem_limit >= 0 && need > (double)orb.int4c_mem_limit) || need - resident > r.free_b)) return 0;
  auto bytes = [](double b) { const std::string t = std::to_string(b); return t.substr(0, t.find('.')) + " bytes"; };
  set_error(std::string(who) + ": with N = " + std::to_string(orb.nao) + ", " + what + " take " + bytes(need) + ", more than the " + bytes(r.room) + " of device memory they may take");
  return QEMB_ERR_ALLOC;
}

}  // namespace

int int4c_guard(const IntBasis& orb, int sym, bool with_output, const char* who) {
  if (int4c_out_words(orb.nao, sym) < 0) { set_error(std::string(who) + ": sym must be 1, 4 or 8, not " + std::to_string(sym)); return QEMB_ERR_ARG; }
  QTRY(check_orbital(orb, who));
  const double out_b = with_output ? 8.0 * (double)int4c_out_words(orb.nao, sym) : 0.0, work_b = (double)int4c_work_bytes(orb);
  return mem_guard(orb, out_b + work_b, 0.0, who, "the integrals (sym = " + std::to_string(sym) + ") and the pair stage");
}

int int4c_fill(IntBasis& orb, int sym, double thresh, double* out) {
  const char* who = "qemb_int4c2e";
  if (!out) { set_error(std::string(who) + ": null output"); return QEMB_ERR_ARG; }
  if (int4c_out_words(orb.nao, sym) < 0) { set_error(std::string(who) + ": sym must be 1, 4 or 8, not " + std::to_string(sym)); return QEMB_ERR_ARG; }
  QTRY(check_thresh(thresh, who));
  QTRY(check_orbital(orb, who));
  const PairPlan p = plan_of(orb);      // the call's own plan, released on return
  DevicePlan d;
  QTRY(d.build(p, orb.dev(), orb.dc2s));
  const bool screen = thresh > 0.0;
  if (screen) {
    int rc = schwarz_factors(orb, p, d);
    if (rc) { dev_sync(); return rc; }
    QTRY(d.upload_q(orb.schwarz));
  }
  orb.int4c_stats[0] = orb.int4c_stats[1] = 0;
  const Side all = whole(p);
  int rc = for_class_pairs(all, all, true, [&](const Step& s) {
    ClassArgs g{};
    g.sh = orb.dev(); g.data = d.data; g.bra = d.list(s.cb, screen); g.ket = d.list(s.ck, screen);
    g.same = s.same; g.thresh = thresh; g.out = sym; g.N = orb.nao; g.dst = out;
    QTRY(dev_int4c_class(kLa[s.cb], kLb[s.cb], kLa[s.ck], kLb[s.ck], g));
    orb.int4c_stats[0] += s.quartets();
    if (screen) orb.int4c_stats[1] += census(s, schwarz_screened(orb, thresh));
    return 0;
  });
  if (rc) { dev_sync(); return rc; }      // earlier launches still read the lists
  return dev_sync();      // the work buffers are released on return
}

namespace {
// The basis's resident pair stage, lists and Schwarz factors (IntBasis::pair_cache): written by the first call that needs them -- direct J / K, the AO ->
// fragment transform or the explicit tile -- and kept to the end of the basis
int ensure_pair_cache(IntBasis& orb) {
  if (orb.pair_cache) return 0;
  auto c = std::make_shared<PairCache>();
  c->plan = plan_of(orb);
  int rc = c->dev.build(c->plan, orb.dev(), orb.dc2s);
  if (!rc) rc = schwarz_factors(orb, c->plan, c->dev);
  if (!rc) rc = c->dev.upload_q(orb.schwarz);
  if (rc) { dev_sync(); return rc; }
  orb.pair_cache = c;
  return 0;
}
int64_t jk_small_bytes(const IntBasis& orb) { return 8 * (3 * (int64_t)orb.nao * orb.nao + (int64_t)orb.nshell * orb.nshell) + 4096; }      // D, J, K, the shell-block table
}  // namespace

int64_t int4c_jk_bytes(const IntBasis& orb) { return int4c_work_bytes(orb) + jk_small_bytes(orb); }

int int4c_jk_direct(IntBasis& orb, const double* dm, double thresh, double* J, double* K, int io_on_device) {
  const char* who = "qemb_int_jk_direct";
  if (!dm) { set_error(std::string(who) + ": null density"); return QEMB_ERR_ARG; }
  if (!J && !K) { set_error(std::string(who) + ": J and K are both null"); return QEMB_ERR_ARG; }
  QTRY(check_thresh(thresh, who));
  QTRY(check_orbital(orb, who));
  QTRY(mem_guard(orb, (double)int4c_jk_bytes(orb), orb.pair_cache ? (double)int4c_work_bytes(orb) : 0.0, who, "the pair stage, the lists and the N x N matrices"));
  QTRY(ensure_pair_cache(orb));
  const DevicePlan& d = orb.pair_cache->dev;
  const PairPlan& p = orb.pair_cache->plan;
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
  const Side all = whole(p);
  int rc = for_class_pairs(all, all, true, [&](const Step& s) {
    JkArgs g{};
    g.sh = orb.dev(); g.data = d.data; g.bra = d.list(s.cb, screen); g.ket = d.list(s.ck, screen);
    g.same = s.same; g.thresh = thresh; g.N = N; g.nshell = (int)nsh; g.dm = dD; g.dmax = screen ? btab.p : nullptr; g.J = dJ; g.K = dK;
    QTRY(dev_int4c_jk_class(kLa[s.cb], kLb[s.cb], kLa[s.ck], kLb[s.ck], g));
    orb.int4c_stats[0] += s.quartets();
    if (screen)
      orb.int4c_stats[1] += census(s, [&](int cb, int64_t i, int ck, int64_t j) {
        return int4c::jk_screened(thresh, orb.schwarz[cb][(size_t)i], orb.schwarz[ck][(size_t)j], tab.data(), (int)nsh, p.a[cb][(size_t)i], p.b[cb][(size_t)i],
                                  p.a[ck][(size_t)j], p.b[ck][(size_t)j]);
      });
    return 0;
  });
  if (rc) { dev_sync(); return rc; }
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
struct Slab : Side {
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

TileLayout tile_layout(const IntBasis& orb, const PairPlan& plan, int64_t tile_pairs, bool with_maps) {
  TileLayout t;
  if (with_maps) { const size_t np = (size_t)npair_of(orb.nao); t.pos.assign(np, -1); t.mu.assign(np, 0); t.nu.assign(np, 0); }
  int64_t c = 0;
  Slab cur;
  auto close = [&]() { if (cur.rows) { t.slabs.push_back(cur); t.max_rows = std::max(t.max_rows, cur.rows); } };
  size_t w = 0;      // the shell pair in the order of plan_of
  for (int I = 0; I < orb.nshell; ++I)
    for (int J = 0; J <= I; ++J, ++w) {
      const Shell &A = orb.shells[I], &B = orb.shells[J];
      const int64_t sz = n_ao_pairs(A, B, I == J);
      if (cur.rows && cur.rows + sz > tile_pairs) {      // the next slab opens where this one ends in every class list
        close();
        Slab next;
        for (int k = 0; k < kNPairClass; ++k) next.first[k] = cur.first[k] + cur.cnt[k];
        next.c0 = c;
        cur = next;
      }
      ++cur.cnt[plan.cls[w]];
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

// One tile: rows = the AO pairs of the shell pairs of R (a range of the lists of dR), columns = those of S in dS (R and S the same set, or disjoint).  Every
// canonical quartet with one pair in R and one in S is evaluated once (for_class_pairs) and lands at [row[.]][col[.]]: every element of the tile is written
// exactly once (a screened quartet as zeros).
int fill_tile(const IntBasis& orb, const double* data, const DevicePlan& dR, const Side& R, const DevicePlan& dS, const Side& S, bool same, const int32_t* row,
              const int32_t* col, int64_t ld, double thresh, double* dst) {
  return for_class_pairs(R, S, same, [&](const Step& s) {
    ClassArgs g{};
    g.sh = orb.dev(); g.data = data; g.thresh = thresh; g.out = int4c::kTile; g.N = orb.nao; g.dst = dst; g.row = row; g.col = col; g.ld = ld;
    g.bra = (s.swapped ? dS : dR).list(s.cb, thresh > 0.0, s.b0, s.bn); g.ket = (same || s.swapped ? dR : dS).list(s.ck, thresh > 0.0, s.k0, s.kn);
    g.same = s.same; g.store = s.store;
    return dev_int4c_class(kLa[s.cb], kLb[s.cb], kLa[s.ck], kLb[s.ck], g);
  });
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
int64_t direct_fixed_bytes(const PairPlan& plan, int64_t N, const DirectSizes& z) { return plan.bytes() + 12 * npair_of(N) + 8 * (z.sum_npq2 + z.sum_ta) + 4096; }
int64_t direct_tile_bytes(int64_t rows, const DirectSizes& z) { return 8 * (rows * rows + 3 * rows * z.npq_max); }
// the default tile: the tile and its operands take at most half of what the fixed part leaves, at most 8192 AO pairs (a 512 MB tile: the products are long
// enough for the GEMM's best rate, and a larger tile saves nothing but launches)
int64_t default_tile_pairs(const IntBasis& orb, const PairPlan& plan, const DirectSizes& z) {
  Room r;
  room_of(orb, &r);      // no figure: no room, the smallest tile
  const double avail = 0.5 * (r.room - (double)direct_fixed_bytes(plan, orb.nao, z)) / 8.0, m = 1.5 * (double)z.npq_max;
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
  const PairPlan plan = plan_of(orb);
  if (tile_pairs <= 0) tile_pairs = default_tile_pairs(orb, plan, z);
  *bytes = direct_fixed_bytes(plan, orb.nao, z) + direct_tile_bytes(tile_layout(orb, plan, tile_pairs, false).max_rows, z);
  return 0;
}

int int4c_ao2mo_direct(IntBasis& orb, int nfrag, const double* const* TA_host, const int* n, int64_t tile_pairs, double thresh, std::vector<DBuf>& out) {
  const char* who = "qemb_ao2mo_direct";
  if (!TA_host) { set_error(std::string(who) + ": null coefficients"); return QEMB_ERR_ARG; }
  QTRY(check_thresh(thresh, who));
  QTRY(check_orbital(orb, who));
  DirectSizes z;
  QTRY(direct_sizes(orb, nfrag, n, who, &z));
  for (int f = 0; f < nfrag; ++f)
    if (!TA_host[f]) { set_error(std::string(who) + ": null coefficients of fragment " + std::to_string(f)); return QEMB_ERR_ARG; }
  const int64_t N = orb.nao;
  TileLayout lay;
  {      // layout and guard from the plan on the host, before anything is allocated
    const PairPlan plan = plan_of(orb);
    if (tile_pairs <= 0) tile_pairs = default_tile_pairs(orb, plan, z);
    lay = tile_layout(orb, plan, tile_pairs, true);
    QTRY(mem_guard(orb, (double)(direct_fixed_bytes(plan, N, z) + direct_tile_bytes(lay.max_rows, z)), orb.pair_cache ? (double)plan.bytes() : 0.0, who,
                   std::to_string(nfrag) + " fragments and tiles of " + std::to_string(lay.max_rows) + " AO pairs"));
  }
  QTRY(ensure_pair_cache(orb));
  const DevicePlan& d = orb.pair_cache->dev;
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
      const bool skip = screen && R.qmax * S.qmax < thresh;      // every quartet of the tile is below the threshold: the tile counts as zeros
      int64_t nq = 0, nscr = 0;
      for_class_pairs(R, S, same, [&](const Step& st) {
        nq += st.quartets();
        if (screen && !skip) nscr += census(st, schwarz_screened(orb, thresh));
        return 0;
      });
      orb.int4c_stats[0] += nq;
      orb.int4c_stats[1] += skip ? nq : nscr;
      ++orb.int4c_tiles[skip ? 1 : 0];
      if (skip) continue;
      if (int rc = fill_tile(orb, d.data, d, R, d, S, same, dpos, dpos, S.rows, thresh, E)) { dev_sync(); return rc; }
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
  QTRY(check_thresh(thresh, who));
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
  QTRY(ensure_pair_cache(orb));
  const PairPlan& full = orb.pair_cache->plan;
  PairPlan sub[2];      // the listed shell pairs in list order, looked up in the pair table of the plan
  std::vector<double> q[2][kNPairClass];
  std::vector<int32_t> map[2];
  int64_t rows[2] = {0, 0};
  for (int side = 0; side < 2; ++side) {
    const int32_t* p = side ? ps : pr;
    map[side].assign((size_t)np, -1);
    for (int64_t k = 0; k < (side ? nsp : nr); ++k) {
      const int64_t I = p[2 * k], J = p[2 * k + 1], w = I * (I + 1) / 2 + J;
      const int c = full.cls[(size_t)w]; const size_t i = (size_t)full.idx[(size_t)w];
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
  for (int k = 0; k < 2; ++k) {
    QTRY(dl[k].upload(sub[k])); QTRY(dl[k].upload_q(q[k]));
    QTRY(dev_h2d(k ? dcol : drow, map[k].data(), sizeof(int32_t) * np));
  }
  QTRY(E.alloc(rows[0] * rows[1]));
  if (int rc = fill_tile(orb, orb.pair_cache->dev.data, dl[0], whole(sub[0]), dl[1], whole(sub[1]), same, drow, dcol, rows[1], thresh, E)) { dev_sync(); return rc; }
  QTRY(dev_d2h(out_host, E, sizeof(double) * rows[0] * rows[1]));
  return dev_sync();
}

// ---- pivoted Cholesky decomposition of the 4-fold packed tensor: blocked, at shell-pair granularity (int4c.h) ----
namespace {

constexpr int64_t kCdDefaultPanel = 128;

inline int32_t* i32(double* p) { return reinterpret_cast<int32_t*>(p); }

// the plan rows of the decomposition: every AO pair once, shell pair after shell pair in the order of plan_of (ONE slab of the tile layout), and per shell pair
// its first row and its number of rows
struct CdRows {
  TileLayout lay;
  std::vector<int32_t> row0, cnt;
  int64_t max_sp = 0;
};
CdRows cd_rows(const IntBasis& orb, const PairPlan& plan, bool with_maps) {
  CdRows r;
  r.lay = tile_layout(orb, plan, npair_of(orb.nao), with_maps);
  int64_t c = 0;
  for (int I = 0; I < orb.nshell; ++I)
    for (int J = 0; J <= I; ++J) {
      const int64_t sz = n_ao_pairs(orb.shells[I], orb.shells[J], I == J);
      r.row0.push_back((int32_t)c); r.cnt.push_back((int32_t)sz);
      c += sz; r.max_sp = std::max(r.max_sp, sz);
    }
  return r;
}
// what a decomposition holds beside the factor: pair stage and lists (with the kDiag buffers), the diagonal, four int32 tables of npair entries, one panel, the
// factor's columns at the panel's rows, the panel's own factor and its small arrays, the shell-pair tables and maxima
int64_t cd_fixed_bytes(const PairPlan& plan, int64_t np, int64_t cap) {
  return plan.bytes() + 8 * np + 16 * np + 8 * np * cap + 8 * cap * cap + 24 * cap + 32 * plan.n_pairs + 8192;
}
int64_t cd_rank_bytes(int64_t np, int64_t cap) { return 8 * (np + cap); }      // per vector: its row of the factor and of the gathered columns
struct CdSizes { int64_t np, cap, panel_pairs, max_rank, bytes; };
int cd_sizes(const IntBasis& orb, const PairPlan& plan, int64_t max_sp, int64_t panel_pairs, int64_t max_rank, CdSizes* z) {
  z->np = npair_of(orb.nao);
  z->panel_pairs = panel_pairs > 0 ? panel_pairs : kCdDefaultPanel;
  z->cap = std::min(z->np, std::max(z->panel_pairs, max_sp));
  if (max_rank <= 0) {      // what the memory allows, at most npair
    Room r;
    room_of(orb, &r);      // no figure: no room, one vector
    const double left = r.room - (double)cd_fixed_bytes(plan, z->np, z->cap);
    max_rank = left > 0.0 ? (int64_t)std::min((double)z->np, left / (double)cd_rank_bytes(z->np, z->cap)) : 0;
    max_rank = std::max<int64_t>(1, max_rank);
  }
  z->max_rank = std::min(max_rank, z->np);
  z->bytes = cd_fixed_bytes(plan, z->np, z->cap) + z->max_rank * cd_rank_bytes(z->np, z->cap);
  return 0;
}
int cd_check_args(const IntBasis& orb, double tol, double span, const char* who) {
  if (!(tol > 0.0) || !std::isfinite(tol)) { set_error(std::string(who) + ": the tolerance must be positive"); return QEMB_ERR_ARG; }
  if (!(span > 0.0 && span <= 1.0)) { set_error(std::string(who) + ": the span factor must lie in (0, 1]"); return QEMB_ERR_ARG; }
  return check_orbital(orb, who);
}

// the factor on the device in plan-row order, with the table that leads back to the canonical pair index
struct CdFactor {
  DBuf L, tables;
  int64_t rank = 0, np = 0;
  const int32_t* pos = nullptr;      // device: canonical AO pair index -> plan row
};

int cd_decompose(IntBasis& orb, double tol, double span, int64_t panel_pairs, int64_t max_rank, const char* who, CdFactor* out) {
  QTRY(cd_check_args(orb, tol, span, who));
  CdRows rows;
  CdSizes z;
  {      // sizes and guard from the plan on the host, before anything is allocated
    const PairPlan plan = plan_of(orb);
    rows = cd_rows(orb, plan, true);
    QTRY(cd_sizes(orb, plan, rows.max_sp, panel_pairs, max_rank, &z));
    QTRY(mem_guard(orb, (double)z.bytes, orb.pair_cache ? (double)plan.bytes() : 0.0, who,
                   "the pair stage, the diagonal, a panel of " + std::to_string(z.cap) + " AO pairs and a factor of up to " + std::to_string(z.max_rank) + " vectors"));
  }
  QTRY(ensure_pair_cache(orb));
  const DevicePlan& d = orb.pair_cache->dev;
  const PairPlan& full = orb.pair_cache->plan;
  const int64_t np = z.np, nsp = full.n_pairs, cap = z.cap, nb = (nsp + 255) / 256;
  // int32 tables: pos, col (per canonical pair index), gidx (per plan row), row0, cnt (per shell pair), srow, piv (per panel column), the panel's rank
  DBuf &tables = out->tables, dD, red, E, LS, T, work, diag;
  QTRY(tables.alloc((3 * np + 2 * nsp + 2 * cap + 2) / 2 + 1));
  int32_t *dpos = i32(tables.p), *dcol = dpos + np, *dgidx = dcol + np, *drow0 = dgidx + np, *dcnt = drow0 + nsp, *dsrow = dcnt + nsp, *dpiv = dsrow + cap, *drank = dpiv + cap;
  QTRY(dD.alloc(np)); QTRY(red.alloc(1 + nsp + nb)); QTRY(E.alloc(np * cap)); QTRY(T.alloc(cap * cap)); QTRY(work.alloc(cap));
  double *dmax_d = red.p, *spmax_d = red.p + 1, *part_d = red.p + 1 + nsp;
  QTRY(dev_h2d(dpos, rows.lay.pos.data(), sizeof(int32_t) * np));
  QTRY(dev_h2d(drow0, rows.row0.data(), sizeof(int32_t) * nsp)); QTRY(dev_h2d(dcnt, rows.cnt.data(), sizeof(int32_t) * nsp));
  {      // 1. the diagonal: the launches of schwarz_factors, every (ab|ab) kept -- gathered from the class buffers into plan-row order
    int64_t base[kNPairClass], words = 0;
    for (int c = 0; c < kNPairClass; ++c) { base[c] = words; words += d.n[c] * (2 * kLa[c] + 1) * (2 * kLb[c] + 1); }
    QTRY(diag.alloc(words));
    for (int c = 0; c < kNPairClass; ++c) {
      if (!d.n[c]) continue;
      ClassArgs g{};
      g.sh = orb.dev(); g.data = d.data; g.bra = g.ket = d.list(c, false); g.same = 1; g.thresh = 0.0; g.out = int4c::kDiag; g.N = orb.nao; g.dst = diag.p + base[c];
      if (int rc = dev_int4c_class(kLa[c], kLb[c], kLa[c], kLb[c], g)) { dev_sync(); return rc; }
    }
    std::vector<int32_t> gidx((size_t)np);
    size_t w = 0;
    for (int I = 0; I < orb.nshell; ++I)
      for (int J = 0; J <= I; ++J, ++w) {
        const Shell &A = orb.shells[I], &B = orb.shells[J];
        const bool sw = A.l < B.l;      // role A of the pair stage: the larger l (PairPlan::add)
        const int c = full.cls[w], nsB = 2 * kLb[c] + 1, ncd = (2 * kLa[c] + 1) * nsB;
        int64_t row = rows.row0[w];
        for_ao_pairs(A, B, I == J, [&](int64_t m, int64_t n) {
          const int a = (int)(m - A.ao0), b = (int)(n - B.ao0);
          gidx[(size_t)row++] = (int32_t)(base[c] + full.idx[w] * ncd + (sw ? b * nsB + a : a * nsB + b));
        });
      }
    if (words > 0x7fffffffLL) { set_error(std::string(who) + ": too many shell pairs"); return QEMB_ERR_ARG; }
    QTRY(dev_h2d(dgidx, gidx.data(), sizeof(int32_t) * np));
    if (int rc = dev_cd_gather_cols(1, np, diag, words, dgidx, dD, np)) { dev_sync(); return rc; }
    if (int rc = dev_cd_diag_update(np, 0, nullptr, 0, nullptr, nullptr, dD, nsp, drow0, dcnt, spmax_d, part_d, dmax_d)) { dev_sync(); return rc; }
  }
  DBuf& L = out->L;
  int64_t capL = std::min(z.max_rank, std::max<int64_t>(4 * cap, 64)), M = 0, panels = 0, cols = 0;
  QTRY(L.alloc(capL * np));
  std::vector<double> hred((size_t)(1 + nsp));
  std::vector<int32_t> colmap((size_t)np), srow;
  std::vector<int64_t> cand;
  std::vector<char> inS((size_t)nsp);
  double dmax = 0.0;
  for (;;) {
    QTRY(dev_d2h(hred.data(), red, sizeof(double) * (1 + nsp)));      // waits for everything issued so far
    dmax = hred[0];
    if (!(dmax > tol)) break;      // 2. the stop test
    if (M >= z.max_rank) {
      orb.cd_stats[0] = M; orb.cd_stats[1] = panels; orb.cd_stats[2] = cols; orb.cd_dmax = dmax;
      char buf[64];
      std::snprintf(buf, sizeof buf, "%.3e", dmax);
      set_error(std::string(who) + ": with N = " + std::to_string(orb.nao) + ", the factor reached rank " + std::to_string(M) + " = max_rank with the largest residual diagonal still " + buf +
                ", above the tolerance");
      return QEMB_ERR_NOCONV;
    }
    // 3. the panel: whole shell pairs above the threshold, largest first
    const double thr = std::max(span * dmax, tol);
    cand.clear();
    for (int64_t w = 0; w < nsp; ++w)
      if (hred[(size_t)(1 + w)] > thr) cand.push_back(w);
    std::stable_sort(cand.begin(), cand.end(), [&](int64_t a, int64_t b) { return hred[(size_t)(1 + a)] > hred[(size_t)(1 + b)]; });      // stable: ties by the lower index
    std::fill(inS.begin(), inS.end(), 0);
    std::fill(colmap.begin(), colmap.end(), -1);
    srow.clear();
    PairPlan sub[2];      // [0]: every shell pair outside the panel, [1]: the panel's, looked up in the pair table of the plan
    auto add_to = [&](PairPlan& s, int64_t w) {
      const int c = full.cls[(size_t)w]; const size_t i = (size_t)full.idx[(size_t)w];
      s.a[c].push_back(full.a[c][i]); s.b[c].push_back(full.b[c][i]); s.off[c].push_back(full.off[c][i]);
    };
    for (int64_t w : cand) {
      if (!srow.empty() && (int64_t)srow.size() + rows.cnt[(size_t)w] > z.panel_pairs) break;
      inS[(size_t)w] = 1;
      add_to(sub[1], w);
      for (int e = 0; e < rows.cnt[(size_t)w]; ++e) {
        const int64_t row = rows.row0[(size_t)w] + e, m = rows.lay.mu[(size_t)row], n = rows.lay.nu[(size_t)row];
        colmap[(size_t)(m * (m + 1) / 2 + n)] = (int32_t)srow.size();
        srow.push_back((int32_t)row);
      }
    }
    for (int64_t w = 0; w < nsp; ++w)
      if (!inS[(size_t)w]) add_to(sub[0], w);
    const int64_t nS = (int64_t)srow.size();
    DevicePlan dl[2];
    for (int k = 0; k < 2; ++k) QTRY(dl[k].upload(sub[k]));
    QTRY(dev_h2d(dcol, colmap.data(), sizeof(int32_t) * np)); QTRY(dev_h2d(dsrow, srow.data(), sizeof(int32_t) * nS));
    // 4. E[:, S] = (all ij | kl in S), unscreened: (pairs outside S) x S and S x S into one buffer
    int rc = fill_tile(orb, d.data, dl[0], whole(sub[0]), dl[1], whole(sub[1]), false, dpos, dcol, nS, 0.0, E);
    if (!rc) rc = fill_tile(orb, d.data, dl[1], whole(sub[1]), dl[1], whole(sub[1]), true, dpos, dcol, nS, 0.0, E);
    // 5. E -= L^T L[:, S]
    if (!rc && M > 0) {
      rc = LS.alloc(M * nS);
      if (!rc) rc = dev_cd_gather_cols(M, nS, L, np, dsrow, LS, nS);
      if (!rc) rc = gemm(np, nS, M, -1.0, L, np, false, LS, nS, false, 1.0, E, nS);
    }
    // 6. the panel's own block
    if (!rc) rc = dev_cd_panel_factor(E, nS, dsrow, (int)nS, thr, dD, T, dpiv, drank, work);
    int32_t r32 = 0;
    if (!rc) rc = dev_d2h(&r32, drank, sizeof(int32_t));
    if (rc) { dev_sync(); return rc; }      // the launches read the lists of dl
    if (r32 <= 0) { set_error(std::string(who) + ": a panel above the threshold gave no pivot"); return QEMB_ERR_NUMERIC; }
    const int64_t r = std::min<int64_t>(r32, z.max_rank - M);      // at max_rank the first pivots of the panel are kept; the stop test above then fails the call
    if (M + r > capL) {
      const int64_t ncap = std::min(z.max_rank, std::max(2 * capL, M + r));
      DBuf bigger;
      QTRY(bigger.alloc(ncap * np));
      if (M > 0) QTRY(dev_d2d(bigger, L, sizeof(double) * M * np));
      QTRY(dev_sync());
      L = std::move(bigger); capL = ncap;
    }
    // 7. the new vectors at every AO pair, 8. the diagonal
    rc = dev_cd_new_rows(np, (int)nS, (int)r, E, nS, T, dpiv, L.p + M * np, np);
    if (!rc) rc = dev_cd_diag_update(np, (int)r, L.p + M * np, np, dpiv, dsrow, dD, nsp, drow0, dcnt, spmax_d, part_d, dmax_d);
    if (rc) { dev_sync(); return rc; }
    M += r; ++panels; cols += nS;
  }
  orb.cd_stats[0] = M; orb.cd_stats[1] = panels; orb.cd_stats[2] = cols; orb.cd_dmax = dmax;
  out->rank = M; out->np = np; out->pos = dpos;
  return 0;
}

}  // namespace

int int4c_cholesky_bytes(const IntBasis& orb, int64_t panel_pairs, int64_t max_rank, int64_t* bytes) {
  const char* who = "qemb_int_cholesky_bytes";
  if (!bytes) { set_error(std::string(who) + ": bad arguments"); return QEMB_ERR_ARG; }
  QTRY(check_orbital(orb, who));
  const PairPlan plan = plan_of(orb);
  CdSizes z;
  QTRY(cd_sizes(orb, plan, cd_rows(orb, plan, false).max_sp, panel_pairs, max_rank, &z));
  *bytes = z.bytes;
  return 0;
}

int int4c_cholesky(IntBasis& orb, double tol, double span, int64_t panel_pairs, int64_t max_rank, double* out_host, int64_t* rank) {
  const char* who = "qemb_int_cholesky";
  if (!rank) { set_error(std::string(who) + ": bad arguments"); return QEMB_ERR_ARG; }
  CdFactor f;
  QTRY(cd_decompose(orb, tol, span, panel_pairs, max_rank, who, &f));
  *rank = f.rank;
  if (!out_host || f.rank == 0) return dev_sync();
  DBuf P;      // 9. canonical packed order: the columns of the factor gathered by the table of plan rows
  QTRY(P.alloc(f.rank * f.np));
  if (int rc = dev_cd_gather_cols(f.rank, f.np, f.L, f.np, f.pos, P, f.np)) { dev_sync(); return rc; }
  QTRY(dev_d2h(out_host, P, sizeof(double) * f.rank * f.np));
  return dev_sync();
}

int int4c_cholesky_to_df(IntBasis& orb, double tol, double span, int64_t panel_pairs, int64_t max_rank, DfContext& df) {
  const char* who = "qemb_df_set_ints_from_cholesky";
  CdFactor f;
  QTRY(cd_decompose(orb, tol, span, panel_pairs, max_rank, who, &f));
  if (f.rank == 0) { set_error(std::string(who) + ": every integral is below the tolerance, the factor is empty"); return QEMB_ERR_NUMERIC; }
  const int64_t N = orb.nao;
  QTRY(mem_guard(orb, 8.0 * (double)f.rank * (double)(N * N + f.np), 8.0 * (double)f.rank * (double)f.np, who,
                 "the factor of " + std::to_string(f.rank) + " vectors and its [rank][N][N] image"));
  QTRY(df.begin_ints_identity((int)N, (int)f.rank));
  if (int rc = dev_cd_unpack(f.rank, N, f.L, f.np, f.pos, df.Lpq)) { dev_sync(); return rc; }      // 9. straight into the context, every element once
  return dev_sync();
}

int int4c_block(const int l[4], const BfRecord* const rec[4], const double* c2s_host, double* out_host) {
  if (!rec[0] || !rec[1] || !rec[2] || !rec[3] || !c2s_host || !out_host) { set_error("qemb_op_int4c_class: null argument"); return QEMB_ERR_ARG; }
  for (int k = 0; k < 4; ++k)
    if (l[k] < 0 || l[k] > int4c::kMaxLOrb) {
      set_error("qemb_op_int4c_class: unsupported angular class (" + std::to_string(l[0]) + "," + std::to_string(l[1]) + "|" + std::to_string(l[2]) + "," + std::to_string(l[3]) + ")");
      return QEMB_ERR_UNSUPPORTED;
    }
  QTRY(check_c2s(c2s_host, "qemb_op_int4c_class"));
  std::vector<Shell> sh(4);
  for (int k = 0; k < 4; ++k) QTRY(shell_of(*rec[k], l[k], 0, "qemb_op_int4c_class", &sh[k]));
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
