// int4c.cpp -- driver of the four-centre AO integrals on the device (see int4c.h): shell pairs per pair class, the pair stage, one launch per canonical class.
#include "int4c.h"
#include <algorithm>
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
  int build(const PairPlan& p, const Shell* dsh, const double* dc2s) {
    std::vector<int32_t> i32; std::vector<int64_t> i64;
    for (int c = 0; c < kNPairClass; ++c) {
      n[c] = (int64_t)p.a[c].size();
      o_a[c] = i32.size(); i32.insert(i32.end(), p.a[c].begin(), p.a[c].end());
      o_b[c] = i32.size(); i32.insert(i32.end(), p.b[c].begin(), p.b[c].end());
      o_off[c] = i64.size(); i64.insert(i64.end(), p.off[c].begin(), p.off[c].end());
    }
    QTRY(d32.alloc((int64_t)i32.size() / 2 + 1)); QTRY(d64.alloc((int64_t)i64.size() + 1)); QTRY(data.alloc(p.data_words));
    if (!i32.empty()) QTRY(dev_h2d(d32, i32.data(), sizeof(int32_t) * i32.size()));
    if (!i64.empty()) QTRY(dev_h2d(d64, i64.data(), sizeof(int64_t) * i64.size()));
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
  if (!orb.jk_cache) {      // first call on this basis: lists, pair stage, Schwarz factors -- kept
    auto c = std::make_shared<Int4cCache>();
    c->plan = plan_of(orb);
    int rc = c->dev.build(c->plan, orb.dev(), orb.dc2s);
    if (!rc) rc = schwarz_factors(orb, c->plan, c->dev);
    if (!rc) {
      std::vector<double> q;
      for (int k = 0; k < kNPairClass; ++k) q.insert(q.end(), orb.schwarz[k].begin(), orb.schwarz[k].end());
      rc = c->dev.dq.alloc((int64_t)q.size() + 1);
      if (!rc && !q.empty()) rc = dev_h2d(c->dev.dq, q.data(), sizeof(double) * q.size());
    }
    if (rc) { dev_sync(); return rc; }
    orb.jk_cache = c;
  }
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
