// int3c.cpp -- driver of the DF integrals on the device (see int3c.h): shells from the uploaded records, work lists per angular class, one launch per class;
// the one-electron integrals of the same basis (int1e_fill);
// and the refusals and the record -> shell copy it shares with the four-centre driver (int4c.cpp).
#include "int3c.h"
#include "int1e_core.h"
#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <utility>

namespace qemb {

using int3c::ClassArgs;
using int3c::Shell;

// ---- the refusals and the record -> shell copy that the DF and the four-centre drivers share (int3c.h) ----
int check_c2s(const double* c2s_host, const char* who) {
  for (int k = 0; k < 10; ++k)
    if (c2s_host[k] != ((k == 0 || k == 1 || k == 5 || k == 9) ? 1.0 : 0.0)) {
      set_error(std::string(who) + ": the Cartesian -> spherical matrices of l = 0 and l = 1 must be the identity (p functions in x, y, z order)");
      return QEMB_ERR_UNSUPPORTED;
    }
  return 0;
}

int check_orbital(const IntBasis& orb, const char* who) {
  for (int i = 0; i < orb.nshell; ++i)
    if (orb.shells[i].l > 2) {
      set_error(std::string(who) + ": orbital shell " + std::to_string(i) + " has l = " + std::to_string(orb.shells[i].l) + "; orbital shells beyond d are not supported");
      return QEMB_ERR_UNSUPPORTED;
    }
  return 0;
}

int check_thresh(double thresh, const char* who) {
  if (thresh >= 0.0) return 0;      // a NaN is refused too
  set_error(std::string(who) + ": the screening threshold must be >= 0");
  return QEMB_ERR_ARG;
}

int shell_of(const BfRecord& r, int l, int ao0, const std::string& who, Shell* s) {
  if (r.nprim < 1 || r.nprim > int3c::kMaxPrim) { set_error(who + ": 1 to 8 primitives per contraction"); return QEMB_ERR_ARG; }
  *s = Shell{};
  for (int d = 0; d < 3; ++d) s->r[d] = r.ctr[d];
  s->l = l; s->nprim = r.nprim; s->ao0 = ao0;
  for (int i = 0; i < r.nprim; ++i) { s->ex[i] = r.ex[i]; s->co[i] = r.co[i]; }
  return 0;
}

int IntBasis::create(int n_bf, const BfRecord* rec, const double* c2s_host) {
  if (n_bf <= 0 || !rec || !c2s_host) { set_error("qemb_int_basis_create: bad arguments"); return QEMB_ERR_ARG; }
  shells.clear(); nao = 0;
  int f = 0;
  while (f < n_bf) {
    const BfRecord& r0 = rec[f];
    const int l = r0.lmn[0] + r0.lmn[1] + r0.lmn[2];
    const std::string where = "qemb_int_basis_create: function " + std::to_string(f);
    if (l < 0 || l > int3c::kMaxL || r0.lmn[0] != l) { set_error(where + " does not start a shell of l <= 4 (components in libcint order, x^l first)"); return QEMB_ERR_UNSUPPORTED; }
    Shell s;
    QTRY(shell_of(r0, l, nao, where, &s));
    const int nc = int3c::ncart(l);
    if (f + nc > n_bf) { set_error(where + ": the shell is incomplete"); return QEMB_ERR_ARG; }
    int k = 0;
    for (int lx = l; lx >= 0; --lx)
      for (int ly = l - lx; ly >= 0; --ly, ++k) {
        const BfRecord& r = rec[f + k];
        const bool same = r.lmn[0] == lx && r.lmn[1] == ly && r.lmn[2] == l - lx - ly && r.nprim == r0.nprim && !std::memcmp(r.ctr, r0.ctr, sizeof(r.ctr)) &&
                          !std::memcmp(r.ex, r0.ex, sizeof(double) * r0.nprim) && !std::memcmp(r.co, r0.co, sizeof(double) * r0.nprim);
        if (!same) { set_error(where + ": component " + std::to_string(k) + " of the shell differs in order, centre, exponents or coefficients"); return QEMB_ERR_UNSUPPORTED; }
      }
    shells.push_back(s);
    nao += 2 * l + 1;
    f += nc;
  }
  nshell = (int)shells.size();
  QTRY(check_c2s(c2s_host, "qemb_int_basis_create"));
  static_assert(sizeof(Shell) % sizeof(double) == 0, "Shell is a whole number of doubles");
  std::vector<Shell> up(shells);
  Shell unit{};      // index nshell on the device: the unit s function of (P|Q) = (P 1|Q); its centre does not enter (exponent 0)
  unit.nprim = 1; unit.ex[0] = 0.0; unit.co[0] = 1.0;
  up.push_back(unit);
  QTRY(dshells.alloc((int64_t)up.size() * (sizeof(Shell) / sizeof(double))));
  QTRY(dev_h2d(dshells, up.data(), sizeof(Shell) * up.size()));
  QTRY(dc2s.alloc(int3c::kC2sLen));
  return dev_h2d(dc2s, c2s_host, sizeof(double) * int3c::kC2sLen);
}

namespace {

// index lists of every class in one device buffer
struct IndexPool {
  std::vector<int32_t> i32;
  std::vector<int64_t> i64;
  DBuf d32, d64;
  int upload() {
    QTRY(d32.alloc((int64_t)(i32.size() + 2) / 2 + 1)); QTRY(d64.alloc((int64_t)i64.size() + 1));
    if (!i32.empty()) QTRY(dev_h2d(d32, i32.data(), sizeof(int32_t) * i32.size()));
    if (!i64.empty()) QTRY(dev_h2d(d64, i64.data(), sizeof(int64_t) * i64.size()));
    return 0;
  }
  const int32_t* p32(size_t off) const { return reinterpret_cast<const int32_t*>(d32.p) + off; }
  const int64_t* p64(size_t off) const { return reinterpret_cast<const int64_t*>(d64.p) + off; }
};

struct PairClass {
  std::vector<int32_t> pa, pb;
  std::vector<int64_t> ent_ptr, ent_row;
  std::vector<int32_t> ent_ab;
  size_t o_pa = 0, o_pb = 0, o_ptr = 0, o_row = 0, o_ab = 0;
};

// auxiliary shells by l: offsets into pool.i32
void aux_lists(const IntBasis& aux, IndexPool& pool, size_t off[int3c::kMaxL + 1], int64_t cnt[int3c::kMaxL + 1]) {
  for (int l = 0; l <= int3c::kMaxL; ++l) {
    off[l] = pool.i32.size(); cnt[l] = 0;
    for (int s = 0; s < aux.nshell; ++s)
      if (aux.shells[s].l == l) { pool.i32.push_back(s); ++cnt[l]; }
  }
}

}  // namespace

int int3c_fill(const IntBasis& orb, const IntBasis& aux, int layout, const int64_t* pairs, int64_t n_pairs, double* out) {
  if (layout < INT_LAYOUT_PQL || layout > INT_LAYOUT_PAIRS) { set_error("qemb_int3c2e: unknown layout " + std::to_string(layout) + " (0 pqL, 1 Lpq, 2 packed, 3 pair list)"); return QEMB_ERR_ARG; }
  if (!out || (layout == INT_LAYOUT_PAIRS) != (pairs != nullptr) || (pairs && n_pairs < 0)) { set_error("qemb_int3c2e: a pair list goes with layout 3 and only with it"); return QEMB_ERR_ARG; }
  QTRY(check_orbital(orb, "qemb_int3c2e"));
  std::map<int, PairClass> cls;      // key la * 8 + lb
  auto role = [&](int I, int J, int& A, int& B) { const bool sw = orb.shells[I].l < orb.shells[J].l; A = sw ? J : I; B = sw ? I : J; return sw; };
  if (layout != INT_LAYOUT_PAIRS) {
    for (int I = 0; I < orb.nshell; ++I)      // rows of the output in increasing order inside a class
      for (int J = 0; J <= I; ++J) {
        int A, B; role(I, J, A, B);
        PairClass& c = cls[orb.shells[A].l * 8 + orb.shells[B].l];
        c.pa.push_back(A); c.pb.push_back(B);
      }
  } else {
    std::vector<int> sh_of(orb.nao);
    for (int s = 0; s < orb.nshell; ++s)
      for (int k = 0; k < 2 * orb.shells[s].l + 1; ++k) sh_of[orb.shells[s].ao0 + k] = s;
    struct Ent { int a, b; int64_t row; };
    std::map<std::pair<int, int>, std::vector<Ent>> by_pair;
    for (int64_t k = 0; k < n_pairs; ++k) {
      const int64_t p = pairs[2 * k], q = pairs[2 * k + 1];
      if (p < 0 || p >= orb.nao || q < 0 || q >= orb.nao) { set_error("qemb_int3c2e: pair " + std::to_string(k) + " is out of range"); return QEMB_ERR_ARG; }
      int I = sh_of[p], J = sh_of[q], a = (int)p - orb.shells[I].ao0, b = (int)q - orb.shells[J].ao0;
      if (I < J) { std::swap(I, J); std::swap(a, b); }
      int A, B;
      if (role(I, J, A, B)) std::swap(a, b);
      if (A == B && a < b) std::swap(a, b);
      by_pair[{A, B}].push_back({a, b, k});
    }
    for (auto& kv : by_pair) {
      PairClass& c = cls[orb.shells[kv.first.first].l * 8 + orb.shells[kv.first.second].l];
      if (c.ent_ptr.empty()) c.ent_ptr.push_back(0);
      c.pa.push_back(kv.first.first); c.pb.push_back(kv.first.second);
      for (const Ent& e : kv.second) { c.ent_ab.push_back(e.a); c.ent_ab.push_back(e.b); c.ent_row.push_back(e.row); }
      c.ent_ptr.push_back((int64_t)c.ent_row.size());
    }
  }
  IndexPool pool;
  size_t aoff[int3c::kMaxL + 1]; int64_t acnt[int3c::kMaxL + 1];
  aux_lists(aux, pool, aoff, acnt);
  for (auto& kv : cls) {
    PairClass& c = kv.second;
    c.o_pa = pool.i32.size(); pool.i32.insert(pool.i32.end(), c.pa.begin(), c.pa.end());
    c.o_pb = pool.i32.size(); pool.i32.insert(pool.i32.end(), c.pb.begin(), c.pb.end());
    c.o_ab = pool.i32.size(); pool.i32.insert(pool.i32.end(), c.ent_ab.begin(), c.ent_ab.end());
    c.o_ptr = pool.i64.size(); pool.i64.insert(pool.i64.end(), c.ent_ptr.begin(), c.ent_ptr.end());
    c.o_row = pool.i64.size(); pool.i64.insert(pool.i64.end(), c.ent_row.begin(), c.ent_row.end());
  }
  QTRY(pool.upload());
  for (auto& kv : cls) {
    const PairClass& c = kv.second;
    for (int lp = 0; lp <= int3c::kMaxL; ++lp) {
      if (!acnt[lp]) continue;
      ClassArgs g{};
      g.orb = orb.dev(); g.aux = aux.dev();
      g.pa = pool.p32(c.o_pa); g.pb = pool.p32(c.o_pb); g.ps = pool.p32(aoff[lp]);
      g.npair = (int64_t)c.pa.size(); g.naux_sh = acnt[lp];
      g.c2s = orb.dc2s; g.out = out; g.layout = layout; g.swapped = 0;
      g.N = orb.nao; g.naux = aux.nao;
      if (layout == INT_LAYOUT_PAIRS) { g.ent_ptr = pool.p64(c.o_ptr); g.ent_ab = pool.p32(c.o_ab); g.ent_row = pool.p64(c.o_row); }
      if (int rc = dev_int3c_class(kv.first / 8, kv.first % 8, lp, g)) { dev_sync(); return rc; }      // earlier launches still read the index lists
    }
  }
  return dev_sync();      // the index lists are released on return
}

int int2c_fill(const IntBasis& aux, double* out) {
  if (!out) { set_error("qemb_int2c2e: null output"); return QEMB_ERR_ARG; }
  IndexPool pool;
  size_t aoff[int3c::kMaxL + 1]; int64_t acnt[int3c::kMaxL + 1];
  aux_lists(aux, pool, aoff, acnt);
  QTRY(pool.upload());
  for (int la = 0; la <= int3c::kMaxL; ++la)
    for (int lp = 0; lp <= int3c::kMaxL; ++lp) {
      if (!acnt[la] || !acnt[lp]) continue;
      ClassArgs g{};
      g.orb = aux.dev(); g.aux = aux.dev();
      g.pa = pool.p32(aoff[la]); g.pb = nullptr; g.ps = pool.p32(aoff[lp]);
      g.npair = acnt[la]; g.naux_sh = acnt[lp];
      g.c2s = aux.dc2s; g.out = out; g.layout = int3c::kMetric;
      g.N = aux.nao; g.naux = aux.nao; g.unit = aux.nshell;
      if (int rc = dev_int3c_class(la, 0, lp, g)) { dev_sync(); return rc; }
    }
  return dev_sync();
}

// S, T, V and the dipole matrices of the basis: shell pairs I >= J grouped by pair class, one launch per class (one wavefront per shell pair), the matrices
// assembled on the device and copied out.  A null output is not computed.  host: the int1e::kKinds matrices in the order of int1e::Kind.
static int int1e_run(const IntBasis& orb, int natm, const double* xyz_host, const double* Z_host, const double* origin, double* const* host, const char* who) {
  QTRY(check_orbital(orb, who));
  bool any = false;
  for (int k = 0; k < int1e::kKinds; ++k) any = any || host[k];
  if (!any) return QEMB_OK;
  std::map<int, PairClass> cls;      // key la * 8 + lb
  for (int I = 0; I < orb.nshell; ++I)
    for (int J = 0; J <= I; ++J) {
      const bool sw = orb.shells[I].l < orb.shells[J].l;
      PairClass& c = cls[orb.shells[sw ? J : I].l * 8 + orb.shells[sw ? I : J].l];
      c.pa.push_back(sw ? J : I); c.pb.push_back(sw ? I : J);
    }
  IndexPool pool;
  for (auto& kv : cls) {
    PairClass& c = kv.second;
    c.o_pa = pool.i32.size(); pool.i32.insert(pool.i32.end(), c.pa.begin(), c.pa.end());
    c.o_pb = pool.i32.size(); pool.i32.insert(pool.i32.end(), c.pb.begin(), c.pb.end());
  }
  QTRY(pool.upload());
  const int64_t n2 = (int64_t)orb.nao * orb.nao;
  DBuf nuc, out[int1e::kKinds];
  if (host[int1e::kNuclear] && natm > 0) {
    QTRY(nuc.alloc(4 * (int64_t)natm));
    QTRY(dev_h2d(nuc, xyz_host, sizeof(double) * 3 * natm));
    QTRY(dev_h2d(nuc.p + 3 * natm, Z_host, sizeof(double) * natm));
  }
  int1e::Args g{};
  g.sh = orb.dev(); g.c2s = orb.dc2s; g.natm = natm; g.xyz = nuc.p; g.Z = nuc.p ? nuc.p + 3 * natm : nullptr; g.N = orb.nao;
  for (int d = 0; d < 3; ++d) g.origin[d] = origin ? origin[d] : 0.0;
  for (int k = 0; k < int1e::kKinds; ++k)
    if (host[k]) { QTRY(out[k].alloc(n2)); g.out[k] = out[k]; }
  for (auto& kv : cls) {
    const PairClass& c = kv.second;
    g.pa = pool.p32(c.o_pa); g.pb = pool.p32(c.o_pb); g.npair = (int64_t)c.pa.size();
    if (int rc = dev_int1e_class(kv.first / 8, kv.first % 8, g)) { dev_sync(); return rc; }      // earlier launches still read the index lists
  }
  for (int k = 0; k < int1e::kKinds; ++k)
    if (host[k]) QTRY(dev_d2h(host[k], out[k], sizeof(double) * n2));
  return dev_sync();      // the index lists are released on return
}

int int1e_fill(const IntBasis& orb, int natm, const double* xyz_host, const double* Z_host, double* S_host, double* T_host, double* V_host) {
  if (natm < 0 || (V_host && natm > 0 && (!xyz_host || !Z_host))) { set_error("qemb_int1e: the nuclear attraction needs natm >= 0 centres and charges"); return QEMB_ERR_ARG; }
  double* const host[int1e::kKinds] = {S_host, T_host, V_host, nullptr, nullptr, nullptr};
  return int1e_run(orb, natm, xyz_host, Z_host, nullptr, host, "qemb_int1e");
}

// <a|r - origin|b>: out_host[3][N][N]
int int1e_dipole_fill(const IntBasis& orb, const double* origin, double* out_host) {
  if (!origin || !out_host) { set_error("qemb_int1e_dipole: origin and out are needed"); return QEMB_ERR_ARG; }
  const int64_t n2 = (int64_t)orb.nao * orb.nao;
  double* const host[int1e::kKinds] = {nullptr, nullptr, nullptr, out_host, out_host + n2, out_host + 2 * n2};
  return int1e_run(orb, 0, nullptr, nullptr, origin, host, "qemb_int1e_dipole");
}

int int3c_block(int la, int lb, int lp, const BfRecord* A, const BfRecord* B, const BfRecord* P, const double* c2s_host, double* out_host) {
  if (!A || !B || !P || !c2s_host || !out_host) { set_error("qemb_op_int3c_class: null argument"); return QEMB_ERR_ARG; }
  if (la < 0 || la > 2 || lb < 0 || lb > 2 || lp < 0 || lp > int3c::kMaxL) {
    set_error("qemb_op_int3c_class: unsupported angular class (" + std::to_string(la) + "," + std::to_string(lb) + "|" + std::to_string(lp) + ")");
    return QEMB_ERR_UNSUPPORTED;
  }
  QTRY(check_c2s(c2s_host, "qemb_op_int3c_class"));
  const BfRecord* rec[3] = {A, B, P};
  const int ls[3] = {la, lb, lp};
  Shell sh[3];
  for (int k = 0; k < 3; ++k) QTRY(shell_of(*rec[k], ls[k], 0, "qemb_op_int3c_class", &sh[k]));
  const int64_t nout = (int64_t)(2 * la + 1) * (2 * lb + 1) * (2 * lp + 1);
  DBuf dsh, dc, dout, didx;
  const int32_t idx[4] = {la >= lb ? 0 : 1, la >= lb ? 1 : 0, 2, 0};      // role A, role B, the auxiliary shell
  QTRY(dsh.alloc(3 * (sizeof(Shell) / sizeof(double)))); QTRY(dc.alloc(int3c::kC2sLen)); QTRY(dout.alloc(nout)); QTRY(didx.alloc(2));
  QTRY(dev_h2d(dsh, sh, sizeof(sh))); QTRY(dev_h2d(dc, c2s_host, sizeof(double) * int3c::kC2sLen)); QTRY(dev_h2d(didx, idx, sizeof(idx)));
  ClassArgs g{};
  const Shell* ds = reinterpret_cast<const Shell*>(dsh.p);
  const int32_t* di = reinterpret_cast<const int32_t*>(didx.p);
  g.orb = ds; g.aux = ds; g.pa = di; g.pb = di + 1; g.ps = di + 2;
  g.npair = 1; g.naux_sh = 1; g.c2s = dc; g.out = dout; g.layout = int3c::kBlock; g.swapped = la < lb;
  g.N = 0; g.naux = 2 * lp + 1;
  QTRY(dev_int3c_class(std::max(la, lb), std::min(la, lb), lp, g));
  return dev_d2h(out_host, dout, sizeof(double) * nout);
}

}  // namespace qemb
