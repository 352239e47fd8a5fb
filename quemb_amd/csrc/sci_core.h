// sci_core.h -- the arithmetic of the selected CI on 64-bit occupation words, written once for the kernels of sci_ops.hip (one item per thread or wave) and
// their scalar restatement for the mock device layer (sci_ops_hostcheck.cpp: the items in a loop).
//
// A determinant is the key (a, b): one uint64 per spin, bit p set = fragment MO p occupied, n <= 64.  Alpha creators stand to the left of the beta ones, the
// creators of one spin in ascending order; keys order by (a, b) as integers -- the order and signs of the full space of fci.cpp.  The phase of a+_a a_i on one
// string is the parity of the occupied orbitals strictly between i and a; an excitation of one spin passes the other spin's creators in pairs and picks up no
// sign.  sci_hij is the Slater-Condon rule on two keys, h [n][n] and V [n^2][n^2] = (pq|rs) in the fragment-MO basis:
//   diagonal       sum_i (na_i + nb_i) h_ii + 1/2 sum_ij [(na_i na_j + nb_i nb_j)(J_ij - K_ij) + 2 na_i nb_j J_ij]
//   single i -> a  +- [h_ai + sum_{j in the same spin} ((ai|jj) - (aj|ji)) + sum_{j in the other spin} (ai|jj)]          (j over the occupied orbitals of the ket)
//   same spin      +- [(ai|bj) - (aj|bi)],  i < j, a < b, the phase of i -> a on the ket times that of j -> b on what it leaves
//   opposite spin  +- (ai|bj), the product of the two single phases
// No shift by the word width anywhere: masks of the orbitals below p are (1 << p) - 1 with p <= 63.
#pragma once
#include <cmath>
#include <cstdint>
#include "dev_ops.h"

#if defined(__HIPCC__)
#define QEMB_SCI_HD __host__ __device__ __forceinline__
#else
#define QEMB_SCI_HD inline
#endif

namespace qemb {

QEMB_SCI_HD int sci_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(x);
#else
  return __builtin_popcountll(x);
#endif
}
QEMB_SCI_HD int sci_ctz(uint64_t x) {      // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((unsigned long long)x) - 1;
#else
  return __builtin_ctzll(x);
#endif
}
QEMB_SCI_HD uint64_t sci_bit(int p) { return (uint64_t)1 << p; }
// parity of the occupied orbitals of s strictly between i and a (i != a)
QEMB_SCI_HD int sci_between(uint64_t s, int i, int a) {
  const int lo = i < a ? i : a, hi = i < a ? a : i;
  const uint64_t below_hi = sci_bit(hi) - 1, upto_lo = (sci_bit(lo) - 1) | sci_bit(lo);
  return sci_popc(s & below_hi & ~upto_lo) & 1;
}
QEMB_SCI_HD bool sci_key_less(uint64_t a1, uint64_t b1, uint64_t a2, uint64_t b2) { return a1 < a2 || (a1 == a2 && b1 < b2); }
// excitation degree of two keys (pairs of orbitals that differ), > 2: not connected
QEMB_SCI_HD int sci_degree(uint64_t a1, uint64_t b1, uint64_t a2, uint64_t b2) { return (sci_popc(a1 ^ a2) + sci_popc(b1 ^ b2)) >> 1; }

QEMB_SCI_HD double sci_diag(int n, const double* h, const double* V, uint64_t a, uint64_t b) {
  const int64_t n2 = (int64_t)n * n;
  double e = 0.0;
  for (uint64_t x = a | b; x; x &= x - 1) {
    const int i = sci_ctz(x);
    const int ai = (int)((a >> i) & 1), bi = (int)((b >> i) & 1);
    double t = 0.0;
    for (uint64_t y = a | b; y; y &= y - 1) {
      const int j = sci_ctz(y);
      const int aj = (int)((a >> j) & 1), bj = (int)((b >> j) & 1);
      const double Jij = V[(int64_t)(i * n + i) * n2 + j * n + j], Kij = V[(int64_t)(i * n + j) * n2 + j * n + i];
      t += (ai * aj + bi * bj) * (Jij - Kij) + (ai * bj + bi * aj) * Jij;
    }
    e += (ai + bi) * h[i * n + i] + 0.5 * t;
  }
  return e;
}
// <a+ i s, other|H|s, other>: s the string that is excited, other the string of the other spin
QEMB_SCI_HD double sci_single(int n, const double* h, const double* V, uint64_t s, uint64_t other, int i, int a) {
  const int64_t n2 = (int64_t)n * n;
  const double* Vai = V + (int64_t)(a * n + i) * n2;
  double x = h[a * n + i];
  for (uint64_t y = s; y; y &= y - 1) { const int j = sci_ctz(y); x += Vai[j * n + j] - V[(int64_t)(a * n + j) * n2 + j * n + i]; }
  for (uint64_t y = other; y; y &= y - 1) { const int j = sci_ctz(y); x += Vai[j * n + j]; }
  return sci_between(s, i, a) ? -x : x;
}
// what an off-diagonal element is made of: the spin-orbital pairs i -> a (and j -> b) that lead from the ket (a2, b2) to the bra (a1, b1), and the phase
struct SciExc { int degree, i, a, j, b, spin1, spin2, neg; };      // spin: 0 alpha, 1 beta; degree 0: the same key
QEMB_SCI_HD SciExc sci_excitation(uint64_t a1, uint64_t b1, uint64_t a2, uint64_t b2) {
  SciExc e = {0, 0, 0, 0, 0, 0, 0, 0};
  const int na = sci_popc(a1 ^ a2) >> 1, nb = sci_popc(b1 ^ b2) >> 1;
  e.degree = na + nb;
  if (e.degree == 0 || e.degree > 2) return e;
  if (e.degree == 1) {
    const uint64_t s = na ? a2 : b2, t = na ? a1 : b1;
    e.spin1 = na ? 0 : 1; e.i = sci_ctz(s & ~t); e.a = sci_ctz(t & ~s); e.neg = sci_between(s, e.i, e.a);
  } else if (na == 1) {
    e.spin1 = 0; e.spin2 = 1;
    e.i = sci_ctz(a2 & ~a1); e.a = sci_ctz(a1 & ~a2); e.j = sci_ctz(b2 & ~b1); e.b = sci_ctz(b1 & ~b2);
    e.neg = sci_between(a2, e.i, e.a) ^ sci_between(b2, e.j, e.b);
  } else {
    const uint64_t s = na ? a2 : b2, t = na ? a1 : b1;
    e.spin1 = e.spin2 = na ? 0 : 1;
    uint64_t holes = s & ~t, parts = t & ~s;
    e.i = sci_ctz(holes); holes &= holes - 1; e.j = sci_ctz(holes);
    e.a = sci_ctz(parts); parts &= parts - 1; e.b = sci_ctz(parts);
    e.neg = sci_between(s, e.i, e.a) ^ sci_between(s ^ sci_bit(e.i) ^ sci_bit(e.a), e.j, e.b);
  }
  return e;
}
// <(a1, b1)|H|(a2, b2)>
QEMB_SCI_HD double sci_hij(int n, const double* h, const double* V, uint64_t a1, uint64_t b1, uint64_t a2, uint64_t b2) {
  const SciExc e = sci_excitation(a1, b1, a2, b2);
  const int64_t n2 = (int64_t)n * n;
  if (e.degree > 2) return 0.0;
  if (e.degree == 0) return sci_diag(n, h, V, a2, b2);
  if (e.degree == 1) return e.spin1 == 0 ? sci_single(n, h, V, a2, b2, e.i, e.a) : sci_single(n, h, V, b2, a2, e.i, e.a);
  double x = V[(int64_t)(e.a * n + e.i) * n2 + e.b * n + e.j];
  if (e.spin1 == e.spin2) x -= V[(int64_t)(e.a * n + e.j) * n2 + e.b * n + e.i];
  return e.neg ? -x : x;
}

// ---- the screen: every single and double excitation of one determinant, as a flat index e in [0, total)
// occ / vir lists of the two strings (ascending); counts in SciLists
struct SciLists { unsigned char occ[2][64], vir[2][64]; int no[2], nv[2]; };
QEMB_SCI_HD void sci_lists(int n, uint64_t a, uint64_t b, SciLists* L) {
  for (int sp = 0; sp < 2; ++sp) {
    const uint64_t s = sp ? b : a;
    int no = 0, nv = 0;
    for (int p = 0; p < n; ++p) { if ((s >> p) & 1) L->occ[sp][no++] = (unsigned char)p; else L->vir[sp][nv++] = (unsigned char)p; }
    L->no[sp] = no; L->nv[sp] = nv;
  }
}
QEMB_SCI_HD long long sci_pairs(int m) { return (long long)m * (m - 1) / 2; }
// pair number p of C(m, 2) -> x < y, p = y (y - 1) / 2 + x
QEMB_SCI_HD void sci_unpair(long long p, int* x, int* y) {
  long long yy = (long long)((1.0 + sqrt(1.0 + 8.0 * (double)p)) * 0.5);
  while (yy * (yy - 1) / 2 > p) --yy;
  while ((yy + 1) * yy / 2 <= p) ++yy;
  *y = (int)yy; *x = (int)(p - yy * (yy - 1) / 2);
}
// the excitations of one determinant: [alpha singles | beta singles | alpha doubles | beta doubles | alpha x beta]; without `doubles` the first two only
QEMB_SCI_HD long long sci_excitation_count(const SciLists& L, bool doubles) {
  const long long sa = (long long)L.no[0] * L.nv[0], sb = (long long)L.no[1] * L.nv[1];
  long long t = sa + sb;
  if (doubles) t += sci_pairs(L.no[0]) * sci_pairs(L.nv[0]) + sci_pairs(L.no[1]) * sci_pairs(L.nv[1]) + sa * sb;
  return t;
}
// excitation e of the determinant (a, b): the key it leads to
QEMB_SCI_HD void sci_excite(const SciLists& L, uint64_t a, uint64_t b, long long e, uint64_t* na, uint64_t* nb) {
  const long long sa = (long long)L.no[0] * L.nv[0], sb = (long long)L.no[1] * L.nv[1];
  *na = a; *nb = b;
  if (e < sa) { *na = a ^ sci_bit(L.occ[0][e / L.nv[0]]) ^ sci_bit(L.vir[0][e % L.nv[0]]); return; }
  e -= sa;
  if (e < sb) { *nb = b ^ sci_bit(L.occ[1][e / L.nv[1]]) ^ sci_bit(L.vir[1][e % L.nv[1]]); return; }
  e -= sb;
  for (int sp = 0; sp < 2; ++sp) {
    const long long pv = sci_pairs(L.nv[sp]), cnt = sci_pairs(L.no[sp]) * pv;
    if (e < cnt) {
      int i, j, p, q;
      sci_unpair(e / pv, &i, &j); sci_unpair(e % pv, &p, &q);
      const uint64_t m = sci_bit(L.occ[sp][i]) ^ sci_bit(L.occ[sp][j]) ^ sci_bit(L.vir[sp][p]) ^ sci_bit(L.vir[sp][q]);
      if (sp == 0) *na = a ^ m; else *nb = b ^ m;
      return;
    }
    e -= cnt;
  }
  const long long ea = e / sb, eb = e % sb;
  *na = a ^ sci_bit(L.occ[0][ea / L.nv[0]]) ^ sci_bit(L.vir[0][ea % L.nv[0]]);
  *nb = b ^ sci_bit(L.occ[1][eb / L.nv[1]]) ^ sci_bit(L.vir[1][eb % L.nv[1]]);
}
// lane `lane` of `nlanes` walks e = lane, lane + nlanes, ...; emit(na, nb) for every excitation with |H c| >= eps.  Returns how many passed.
template <class Emit>
QEMB_SCI_HD int sci_screen_lane(int n, const double* h, const double* V, const SciLists& L, uint64_t a, uint64_t b, double c, double eps, double dbl_bound,
                                int lane, int nlanes, Emit emit) {
  if (c == 0.0) return 0;
  const long long total = sci_excitation_count(L, fabs(c) * dbl_bound >= eps);
  int cnt = 0;
  for (long long e = lane; e < total; e += nlanes) {
    uint64_t na, nb;
    sci_excite(L, a, b, e, &na, &nb);
    if (fabs(sci_hij(n, h, V, na, nb, a, b) * c) >= eps) { emit(cnt, na, nb); ++cnt; }
  }
  return cnt;
}

// ---- the second-order correction: the determinant (a, b) outside the sorted space against its members.  Lane `lane` of `nlanes` takes the runs of equal alpha
// s = lane, lane + nlanes, ... (seg[s] .. seg[s + 1], as sci_build forms them): a run whose alpha is more than two excitations away is skipped whole, then the
// betas of the run are compared.  Returns the lane's part of S_a = sum_i H_ai c_i over the products with |H_ai c_i| >= eps, each tested on its own -- the
// expression the screen tests, bra and ket in the same places, so the two passes decide alike.  A double excitation of a member with |c_i| dbl_bound < eps
// cannot pass (the screen's own shortcut) and is not evaluated.
QEMB_SCI_HD double sci_pt2_lane(int n, const double* h, const double* V, const uint64_t* keys, const double* c, long long nseg, const long long* seg, uint64_t a, uint64_t b,
                                double eps, double dbl_bound, int lane, int nlanes) {
  double sum = 0.0;
  for (long long s = lane; s < nseg; s += nlanes) {
    const long long k0 = seg[s], k1 = seg[s + 1];
    const uint64_t as = keys[2 * k0];
    const int da = sci_popc(a ^ as) >> 1;
    if (da > 2) continue;
    for (long long k = k0; k < k1; ++k) {
      const uint64_t bs = keys[2 * k + 1];
      const int d = da + (sci_popc(b ^ bs) >> 1);
      if (d > 2 || d == 0) continue;
      const double ck = c[k];
      if (ck == 0.0 || (d == 2 && !(fabs(ck) * dbl_bound >= eps))) continue;
      const double x = sci_hij(n, h, V, a, b, as, bs) * ck;
      if (fabs(x) >= eps) sum += x;
    }
  }
  return sum;
}
// the Epstein-Nesbet term of one determinant; the denominator is not guarded
QEMB_SCI_HD double sci_pt2_term(double S, double e_var, double haa) { return S * S / (e_var - haa); }
// a key of the screen's output that lies outside the alpha-word range [lo, hi] becomes the pad key of the sort, which flag_new drops
QEMB_SCI_HD void sci_put_in_range(uint64_t* o, uint64_t a, uint64_t b, uint64_t lo, uint64_t hi) {
  const bool in = a >= lo && a <= hi;
  o[0] = in ? a : ~(uint64_t)0; o[1] = in ? b : ~(uint64_t)0;
}

// position of the first key of A[0..nA) that is not less than (a, b); keys are interleaved (A[2k], A[2k+1])
QEMB_SCI_HD long long sci_lower_bound(const uint64_t* A, long long nA, uint64_t a, uint64_t b) {
  long long lo = 0, hi = nA;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (sci_key_less(A[2 * mid], A[2 * mid + 1], a, b)) lo = mid + 1; else hi = mid;
  }
  return lo;
}
QEMB_SCI_HD bool sci_contains(const uint64_t* A, long long nA, uint64_t a, uint64_t b) {
  const long long k = sci_lower_bound(A, nA, a, b);
  return k < nA && A[2 * k] == a && A[2 * k + 1] == b;
}

}  // namespace qemb
