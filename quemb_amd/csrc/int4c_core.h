// int4c_core.h -- one (shell pair | shell pair) block of the four-centre AO Coulomb integrals (mu nu|lambda sigma), McMurchie-Davidson, as inline arithmetic
// that the gfx950 kernels (int4c_ops.hip) and the scalar restatement of the mock device layer (int4c_ops_hostcheck.cpp: loops) both instantiate.  The Boys
// function, the Hermite E coefficients, the R table, the shell record and the Cartesian -> spherical tables are those of int3c_core.h; mathematics,
// normalisation and component order are those of the host source csrc_host/gto_ints.c behind Mole.eri_s1:
//   (ab|cd) = sum_prim ca cb cc cd K_ab K_cd 2 pi^5/2 / (p q sqrt(p + q)) sum_{tuv} E^{ab}_{tuv} sum_{t'u'v'} (-1)^{t'+u'+v'} E^{cd}_{t'u'v'} R_{t+t',u+u',v+v'}(pq/(p+q), P - Q)
// Two stages, so that no thread carries a Cartesian block (a (dd|dd) one has 1296 elements):
//   pair_item     per (shell pair, primitive pair): p, P and the Hermite expansion of every REAL-SPHERICAL product a b of the pair,
//                   Ebar^{ab}_{tuv} = ca cb K_ab sum_{ia ib} c2s_A[ia,a] c2s_B[ib,b] Ex[t] Ey[u] Ez[v]      (nsph(la) nsph(lb) nherm(la + lb) numbers, 875 for dd)
//                 -- the Cartesian -> spherical step is done here, once per pair, on the coefficients;
//   quartet_item  per (shell quartet, ket component pair c d): over the primitive quartets one R table, G_{tuv} = pref sum (-1)^{..} Ebar^{cd}_{t'u'v'} R_{t+t',..}
//                 (at most 35 numbers) and acc[a b] += sum_{tuv} Ebar^{ab}_{tuv} G_{tuv} for the nsph(la) nsph(lb) <= 25 bra products; then every element
//                 of the output that belongs to (a b|c d) is stored once, from that one value.
// The stored forms include a TILE of the 4-fold packed tensor (kTile: rows and columns are two sets of AO pairs), the operand of the integral-direct
// AO -> fragment transform; pairprod_item and addt_item are the two element-wise passes of that transform (int4c.cpp: ao2mo_direct).
#pragma once
#include "int3c_core.h"

namespace qemb {
namespace int4c {

using int3c::Shell;
using int3c::kMaxPrim;
using int3c::ncart;
using int3c::nsph;
using int3c::nherm;
using int3c::c2s_off;
using int3c::hidx;

constexpr int kMaxLOrb = 2;                                                   // orbital shells s, p, d
constexpr int kNPairClass = (kMaxLOrb + 1) * (kMaxLOrb + 2) / 2;              // ss ps pp ds dp dd
constexpr int kPrimPairs = kMaxPrim * kMaxPrim;
constexpr int pair_class(int la, int lb) { return la * (la + 1) / 2 + lb; }   // la >= lb
constexpr int pair_stride(int la, int lb) { return 4 + nsph(la) * nsph(lb) * nherm(la + lb); }      // doubles per primitive pair: p, P[3], Ebar

// the shell pairs of one pair class (role A: the shell of larger l; a == b: a pair inside one shell), in increasing order of the pair index I (I + 1) / 2 + J
struct PairList {
  const int32_t* a;
  const int32_t* b;
  const int64_t* off;          // first double of the pair in `data`; primitive pair (ia, ib) at off + (ia * nprim_b + ib) * pair_stride
  const double* q;             // Schwarz factor sqrt(max_ab (ab|ab)) of the pair, or null (no screening)
  int64_t n;
};

struct PairArgs {
  const Shell* sh;
  PairList pairs;
  const double* c2s;
  double* data;
};

// Cartesian exponents of component i of a shell in libcint order
QEMB_I3_HD void cart_lmn(int l, int i, int& x, int& y, int& z) {
  int k = 0;
  x = l; y = 0; z = 0;
  for (int cx = l; cx >= 0; --cx)
    for (int cy = l - cx; cy >= 0; --cy, ++k)
      if (k == i) { x = cx; y = cy; z = l - cx - cy; }
}

template <int LA, int LB>
QEMB_I3_HD void pair_item(const PairArgs& g, int64_t item) {
  constexpr int LAB = LA + LB, NT = LAB + 1, nh = nherm(LAB), nsA = nsph(LA), nsB = nsph(LB), ncA = ncart(LA), ncB = ncart(LB);
  const int64_t k = item / kPrimPairs;
  const int ip = (int)(item % kPrimPairs);
  const Shell& A = g.sh[g.pairs.a[k]];
  const Shell& B = g.sh[g.pairs.b[k]];
  if (ip >= A.nprim * B.nprim) return;
  const int pa = ip / B.nprim, pb = ip % B.nprim;
  const double a = A.ex[pa], b = B.ex[pb], p = a + b, h = 0.5 / p;
  const double AB[3] = {A.r[0] - B.r[0], A.r[1] - B.r[1], A.r[2] - B.r[2]};
  const double cf = A.co[pa] * B.co[pb] * exp(-(a * b / p) * (AB[0] * AB[0] + AB[1] * AB[1] + AB[2] * AB[2]));
  double Ex[(LA + 1) * (LB + 1) * NT], Ey[(LA + 1) * (LB + 1) * NT], Ez[(LA + 1) * (LB + 1) * NT];
  int3c::hermite_e<LA, LB>(h, -(b / p) * AB[0], (a / p) * AB[0], Ex);
  int3c::hermite_e<LA, LB>(h, -(b / p) * AB[1], (a / p) * AB[1], Ey);
  int3c::hermite_e<LA, LB>(h, -(b / p) * AB[2], (a / p) * AB[2], Ez);
  double* o = g.data + g.pairs.off[k] + (int64_t)ip * pair_stride(LA, LB);
  o[0] = p;
  for (int d = 0; d < 3; ++d) o[1 + d] = (a * A.r[d] + b * B.r[d]) / p;
  const double* MA = g.c2s + c2s_off(LA);
  const double* MB = g.c2s + c2s_off(LB);
  for (int sa = 0; sa < nsA; ++sa)
    for (int sb = 0; sb < nsB; ++sb) {
      double* e = o + 4 + (sa * nsB + sb) * nh;
      for (int t = 0; t <= LAB; ++t)
        for (int u = 0; u <= LAB - t; ++u)
          for (int v = 0; v <= LAB - t - u; ++v) {
            double s = 0.0;
            for (int ia = 0; ia < ncA; ++ia) {
              const double wa = LA >= 2 ? MA[ia * nsA + sa] : (ia == sa ? 1.0 : 0.0);      // s, p: the identity (IntBasis::create checks the table)
              if (wa == 0.0) continue;
              int ax, ay, az;
              cart_lmn(LA, ia, ax, ay, az);
              for (int ib = 0; ib < ncB; ++ib) {
                const double wb = LB >= 2 ? MB[ib * nsB + sb] : (ib == sb ? 1.0 : 0.0);
                if (wb == 0.0) continue;
                int bx, by, bz;
                cart_lmn(LB, ib, bx, by, bz);
                if (t > ax + bx || u > ay + by || v > az + bz) continue;
                s += wa * wb * Ex[(ax * (LB + 1) + bx) * NT + t] * Ey[(ay * (LB + 1) + by) * NT + u] * Ez[(az * (LB + 1) + bz) * NT + v];
              }
            }
            e[hidx(t, u, v)] = cf * s;
          }
    }
}

// ---- one launch: the shell quartets of one angular class (la >= lb | lc >= ld), bra pair class >= ket pair class ---------------------------------
enum Out { kBlock = 0, kS1 = 1, kDiag = 2, kS4 = 4, kS8 = 8, kTile = 16 };
enum TileStore { kTileAsIs = 0, kTileTransposed = 1, kTileBoth = 2 };

struct ClassArgs {
  const Shell* sh;
  const double* data;          // what pair_item wrote
  PairList bra, ket;
  int same;                    // bra and ket are the same list (equal pair classes): only the quartets with bra index >= ket index are computed
  double thresh;               // > 0 with bra.q / ket.q: a quartet with q_bra q_ket < thresh is stored as zeros
  int out;                     // kS8: 1-D npair (npair + 1) / 2; kS4: [npair][npair]; kS1: [N]^4; kBlock: one block [a][b][c][d];
                               // kDiag: dst[k * nsph(lc) nsph(ld) + c d] = (c d|c d) of pair k (bra == ket list, the source of the Schwarz factors)
                               // kTile: dst[row[ij] * ld + col[kl]] -- a tile of the kS4 tensor whose rows / columns are the AO pairs of two sets of shell pairs
  int64_t N;
  double* dst;
  // kTile only.  row / col: AO pair index -> compact tile row / column (defined for the AO pairs of the bra / ket lists' shell pairs; for kTileTransposed the
  // other way round).  store: kTileAsIs (ij|kl) -> [row[ij]][col[kl]]; kTileTransposed -> [row[kl]][col[ij]] (the class kernels need bra class >= ket class: a
  // quartet whose bra pair belongs to the column set is computed in that orientation and stored transposed); kTileBoth: both, once where ij = kl (rows = columns)
  const int32_t* row;
  const int32_t* col;
  int64_t ld;
  int store;
};

template <int LC, int LD>
inline int64_t class_items(const ClassArgs& g) {
  return (g.out == kDiag ? g.bra.n : g.bra.n * g.ket.n) * (nsph(LC) * nsph(LD));
}

// The primitive loops of one item: acc[ab] += (a b|c d) for the bra products ab0 <= ab < ab1 and the ket product cd, over every primitive quartet of the two
// pairs (boff / koff: their first doubles in `data`).  Shared by the stored forms (quartet_item) and the digest form (quartet_jk_item).
template <int LA, int LB, int LC, int LD>
QEMB_I3_HD void quartet_acc(const Shell& A, const Shell& B, const Shell& C, const Shell& D, const double* data, int64_t boff, int64_t koff, int cd, int ab0, int ab1,
                            double* acc) {
  constexpr int LAB = LA + LB, LCD = LC + LD, L = LAB + LCD, nhAB = nherm(LAB), nhCD = nherm(LCD);
  constexpr double kPref = 34.98683665524972497;      // 2 pi^(5/2)
  const int npab = A.nprim * B.nprim, npcd = C.nprim * D.nprim;
  double R[nherm(L)], G[nhAB];
  for (int ib = 0; ib < npab; ++ib) {
    const double* eb = data + boff + (int64_t)ib * pair_stride(LA, LB);
    const double p = eb[0];
    for (int ik = 0; ik < npcd; ++ik) {
      const double* ek = data + koff + (int64_t)ik * pair_stride(LC, LD);
      const double q = ek[0];
      const double PQ[3] = {eb[1] - ek[1], eb[2] - ek[2], eb[3] - ek[3]};
      int3c::rtable<L>(p * q / (p + q), PQ, R);
      const double pref = kPref / (p * q * sqrt(p + q));
      const double* ecd = ek + 4 + cd * nhCD;
      for (int t = 0; t <= LAB; ++t)
        for (int u = 0; u <= LAB - t; ++u)
          for (int v = 0; v <= LAB - t - u; ++v) {
            double s = 0.0;
            for (int t2 = 0; t2 <= LCD; ++t2)
              for (int u2 = 0; u2 <= LCD - t2; ++u2)
                for (int v2 = 0; v2 <= LCD - t2 - u2; ++v2) {
                  const double term = ecd[hidx(t2, u2, v2)] * R[hidx(t + t2, u + u2, v + v2)];
                  s += ((t2 + u2 + v2) & 1) ? -term : term;
                }
            G[hidx(t, u, v)] = pref * s;
          }
      for (int ab = ab0; ab < ab1; ++ab) {
        const double* e = eb + 4 + ab * nhAB;
        double s = 0.0;
        for (int hh = 0; hh < nhAB; ++hh) s += e[hh] * G[hh];
        acc[ab] += s;
      }
    }
  }
}

// Every element of `dst` that belongs to the item is written exactly once, by plain stores, all images of an integral from one value: the same bits run to run.
template <int LA, int LB, int LC, int LD>
QEMB_I3_HD void quartet_item(const ClassArgs& g, int64_t item) {
  constexpr int nsA = nsph(LA), nsB = nsph(LB), nsC = nsph(LC), nsD = nsph(LD), nab = nsA * nsB, ncd = nsC * nsD;
  const int cd = (int)(item % ncd);
  const int64_t qi = item / ncd;
  const int64_t kb = g.out == kDiag ? qi : qi / g.ket.n, kk = g.out == kDiag ? qi : qi % g.ket.n;
  if (g.same && kk > kb) return;
  const int c = cd / nsD, d = cd % nsD;
  const bool sameAB = g.bra.a[kb] == g.bra.b[kb], sameCD = g.ket.a[kk] == g.ket.b[kk], diag = g.same && kb == kk;
  if (sameCD && d > c && g.out != kDiag && g.out != kBlock) return;      // a pair inside one shell: mu >= nu only, the other order is its image
  const Shell& A = g.sh[g.bra.a[kb]];
  const Shell& B = g.sh[g.bra.b[kb]];
  const Shell& C = g.sh[g.ket.a[kk]];
  const Shell& D = g.sh[g.ket.b[kk]];
  double acc[nab];
  for (int k = 0; k < nab; ++k) acc[k] = 0.0;
  const bool screened = g.thresh > 0.0 && g.bra.q && g.ket.q && g.bra.q[kb] * g.ket.q[kk] < g.thresh;
  const int abd = (c % nsA) * nsB + (d % nsB);                                      // kDiag (LA == LC, LB == LD): the one bra product the item stores, (c d|c d)
  const int ab0 = g.out == kDiag ? abd : 0, ab1 = g.out == kDiag ? abd + 1 : nab;
  if (!screened) quartet_acc<LA, LB, LC, LD>(A, B, C, D, g.data, g.bra.off[kb], g.ket.off[kk], cd, ab0, ab1, acc);
  if (g.out == kDiag) {      // LA == LC, LB == LD
    g.dst[kb * ncd + cd] = acc[abd];
    return;
  }
  const int64_t N = g.N, np = N * (N + 1) / 2;
  const int64_t la = C.ao0 + c, si = D.ao0 + d;
  const int64_t kl = la >= si ? la * (la + 1) / 2 + si : si * (si + 1) / 2 + la;
  for (int a = 0; a < nsA; ++a)
    for (int b = 0; b < nsB; ++b) {
      const double v = acc[a * nsB + b];
      if (g.out == kBlock) { g.dst[((a * nsB + b) * nsC + c) * nsD + d] = v; continue; }
      if (sameAB && b > a) continue;
      const int64_t mu = A.ao0 + a, nu = B.ao0 + b;
      const int64_t ij = mu >= nu ? mu * (mu + 1) / 2 + nu : nu * (nu + 1) / 2 + mu;
      if (diag && kl > ij) continue;      // (ab|cd) and (cd|ab) of one shell pair: the one with ij >= kl is computed
      if (g.out == kS8) {
        const int64_t hi = ij >= kl ? ij : kl, lo = ij >= kl ? kl : ij;
        g.dst[hi * (hi + 1) / 2 + lo] = v;
      } else if (g.out == kS4) {
        g.dst[ij * np + kl] = v;
        if (ij != kl) g.dst[kl * np + ij] = v;
      } else if (g.out == kTile) {
        if (g.store != kTileTransposed) g.dst[g.row[ij] * g.ld + g.col[kl]] = v;
        if (g.store == kTileTransposed || (g.store == kTileBoth && ij != kl)) g.dst[g.row[kl] * g.ld + g.col[ij]] = v;
      } else {      // kS1: the 8 images (fewer where indices coincide), each stored once
        double* o = g.dst;
        o[((mu * N + nu) * N + la) * N + si] = v;
        if (mu != nu) o[((nu * N + mu) * N + la) * N + si] = v;
        if (la != si) {
          o[((mu * N + nu) * N + si) * N + la] = v;
          if (mu != nu) o[((nu * N + mu) * N + si) * N + la] = v;
        }
        if (ij != kl) {
          o[((la * N + si) * N + mu) * N + nu] = v;
          if (mu != nu) o[((la * N + si) * N + nu) * N + mu] = v;
          if (la != si) {
            o[((si * N + la) * N + mu) * N + nu] = v;
            if (mu != nu) o[((si * N + la) * N + nu) * N + mu] = v;
          }
        }
      }
    }
}

// ---- the element-wise passes of the integral-direct AO -> fragment transform ----------------------------------------------------------------------------
// P[r][pq] = TA[mu,p] TA[nu,q] + TA[nu,p] TA[mu,q] (mu != nu), TA[mu,p] TA[mu,q] (mu = nu) for the AO pair (mu[r], nu[r]) of tile row r and the packed fragment
// pair pq = p (p + 1) / 2 + q, p >= q: one item per element, consecutive items along pq (the stores of a wavefront are one contiguous run).
struct PairProdArgs {
  const double* TA;            // [N][n]
  int64_t n, npq, rows;
  const int32_t* mu;           // [rows], mu >= nu
  const int32_t* nu;
  double* P;                   // [rows][npq]
};

QEMB_I3_HD void pairprod_item(const PairProdArgs& g, int64_t r, int64_t pq) {
  int64_t p = (int64_t)((sqrtf(8.0f * (float)pq + 1.0f) - 1.0f) * 0.5f);      // single precision is 2^-7 of a unit off at pq = 2^31: the two loops settle it
  while (p * (p + 1) / 2 > pq) --p;
  while ((p + 1) * (p + 2) / 2 <= pq) ++p;
  const int64_t q = pq - p * (p + 1) / 2;
  const double* tm = g.TA + (int64_t)g.mu[r] * g.n;
  const double* tn = g.TA + (int64_t)g.nu[r] * g.n;
  g.P[r * g.npq + pq] = g.mu[r] == g.nu[r] ? tm[p] * tm[q] : tm[p] * tn[q] + tn[p] * tm[q];
}

// A = A + A^T in place (m x m): the item of (i, j), i >= j, owns both elements
QEMB_I3_HD void addt_item(double* A, int64_t m, int64_t i, int64_t j) {
  if (j > i) return;
  const double s = A[i * m + j] + A[j * m + i];
  A[i * m + j] = s;
  A[j * m + i] = s;
}

// ---- the digest form: J and K from the quartets, no integral stored (qemb_int_jk_direct) -----------------------------------------------------------
// One item is the item of quartet_item: (shell quartet, ket component pair c d), the same primitive loops (quartet_acc) and the same filters (sameAB / sameCD /
// diag), so every unique integral v = (mu nu|la si) -- one per orbit of the 8 index permutations -- is met exactly once.  Its orbit contributes to
//   J[p,q] = sum_rs (pq|rs) D[r,s]        K[p,r] = sum_qs (pq|rs) D[q,s]
// the sum over its DISTINCT images.  The 8 permutations (mu <-> nu, la <-> si, bra <-> ket) form a group; the images of v are the cosets of its stabiliser,
// whose order is 2^(number of coincidences among mu = nu, la = si, (mu nu) = (la si)) -- mu = si with nu = la cannot hold unless all four are equal.  So
// applying ALL 8 permutations with the scaled value
//   v' = v  *  (mu = nu ? 1/2 : 1)  *  (la = si ? 1/2 : 1)  *  (ij = kl ? 1/2 : 1)
// counts every distinct image once.  With D symmetric the 8 terms are
//   J_full[mu,nu] += 2 v' D[la,si]    J_full[nu,mu] += 2 v' D[la,si]    J_full[la,si] += 2 v' D[mu,nu]    J_full[si,la] += 2 v' D[mu,nu]
//   K = T + T^T,   T[mu,la] += v' D[nu,si]    T[nu,la] += v' D[mu,si]    T[mu,si] += v' D[nu,la]    T[nu,si] += v' D[mu,la]
// Only the lower triangle L (p >= r) is accumulated and mirrored afterwards (dev_mirror_lower), so J and K are symmetric to the bit:
//   J:  L[max(mu,nu), min] += (mu = nu ? 4 : 2) v' D[la,si],   L[max(la,si), min] += (la = si ? 4 : 2) v' D[mu,nu]
//       -- with the factors of v' that is  w_kl v D[la,si]  and  w_ij v D[mu,nu]  (w = 2 off the diagonal of the pair, 1 on it), halved each when ij = kl,
//       where both land on one element
//   K:  a term x for T[p,r] becomes  L[max(p,r), min] += (p = r ? 2 : 1) x        (K[p,p] = 2 T[p,p];  K[p,r] = T[p,r] + T[r,p])
// e.g. mu = nu = la = si: v' = v / 8, J: 2 adds of 4 v' D = v D; K: 4 terms of 2 v' D = v D.
// Inside the item everything that shares a destination is summed first: J[la,si] gets one add (sum over a b), the K rows (mu, la), (mu, si) one add per a
// (summed over b), (nu, la), (nu, si) one per b (summed over a): nab + 1 + 2 (nsA + nsB) adds per item, through QEMB_JK_ADD -- an FP64 atomic add on the
// device (the sums then depend on arrival order: not bit-reproducible from run to run), a plain += in the scalar restatement.
#ifndef QEMB_JK_ADD
#if defined(__HIP_DEVICE_COMPILE__)
#define QEMB_JK_ADD(p, x) unsafeAtomicAdd((p), (x))
#else
#define QEMB_JK_ADD(p, x) (*(p) += (x))
#endif
#endif

struct JkArgs {
  const Shell* sh;
  const double* data;          // what pair_item wrote
  PairList bra, ket;
  int same;                    // as ClassArgs
  double thresh;               // > 0 with bra.q / ket.q: a quartet with q_bra q_ket < thresh, or q_bra q_ket dmax < thresh, is skipped
  int64_t N;
  int nshell;
  const double* dm;            // [N][N], symmetric
  const double* dmax;          // [nshell][nshell] max |D| per shell block (dmax_item), or null: the bound is not weighted
  double* J;                   // [N][N] lower triangle accumulated (zeroed by the caller, mirrored afterwards); null: not formed
  double* K;                   // likewise
};

template <int LC, int LD>
inline int64_t jk_items(const JkArgs& g) { return g.bra.n * g.ket.n * (nsph(LC) * nsph(LD)); }

// max |D| over the block of shells (I, J): one item per ordered shell pair
QEMB_I3_HD void dmax_item(const Shell* sh, int nshell, int64_t N, const double* dm, double* out, int64_t item) {
  const Shell& A = sh[item / nshell];
  const Shell& B = sh[item % nshell];
  double m = 0.0;
  for (int a = 0; a < 2 * A.l + 1; ++a)
    for (int b = 0; b < 2 * B.l + 1; ++b) m = fmax(m, fabs(dm[(A.ao0 + a) * N + B.ao0 + b]));
  out[item] = m;
}

// the screening decision of one quartet (shells ia, ib | ic, id with Schwarz factors qb, qk): shared by the items and by the census of the driver
QEMB_I3_HD bool jk_screened(double thresh, double qb, double qk, const double* dmax, int nshell, int ia, int ib, int ic, int id) {
  if (!(thresh > 0.0)) return false;
  const double qq = qb * qk;
  if (qq < thresh) return true;
  if (!dmax) return false;
  double m = fmax(dmax[ic * nshell + id], dmax[ia * nshell + ib]);
  m = fmax(m, fmax(dmax[ib * nshell + id], dmax[ib * nshell + ic]));
  m = fmax(m, fmax(dmax[ia * nshell + id], dmax[ia * nshell + ic]));
  return qq * m < thresh;
}

QEMB_I3_HD void jk_add_lower(double* M, int64_t N, int64_t p, int64_t r, double x) {
  if (x == 0.0) return;
  QEMB_JK_ADD(M + (p >= r ? p * N + r : r * N + p), p == r ? 2.0 * x : x);
}

template <int LA, int LB, int LC, int LD>
QEMB_I3_HD void quartet_jk_item(const JkArgs& g, int64_t item) {
  constexpr int nsA = nsph(LA), nsB = nsph(LB), nsD = nsph(LD), nab = nsA * nsB, ncd = nsph(LC) * nsD;
  const int cd = (int)(item % ncd);
  const int64_t qi = item / ncd;
  const int64_t kb = qi / g.ket.n, kk = qi % g.ket.n;
  if (g.same && kk > kb) return;
  const int c = cd / nsD, d = cd % nsD;
  const int ia = g.bra.a[kb], ib = g.bra.b[kb], ic = g.ket.a[kk], id = g.ket.b[kk];
  const bool sameAB = ia == ib, sameCD = ic == id, diag = g.same && kb == kk;
  if (sameCD && d > c) return;
  if (g.bra.q && g.ket.q && jk_screened(g.thresh, g.bra.q[kb], g.ket.q[kk], g.dmax, g.nshell, ia, ib, ic, id)) return;
  const Shell& A = g.sh[ia];
  const Shell& B = g.sh[ib];
  const Shell& C = g.sh[ic];
  const Shell& D = g.sh[id];
  double acc[nab];
  for (int k = 0; k < nab; ++k) acc[k] = 0.0;
  quartet_acc<LA, LB, LC, LD>(A, B, C, D, g.data, g.bra.off[kb], g.ket.off[kk], cd, 0, nab, acc);
  const int64_t N = g.N;
  const int64_t la = C.ao0 + c, si = D.ao0 + d;
  const int64_t kl = la >= si ? la * (la + 1) / 2 + si : si * (si + 1) / 2 + la;
  const double* Dl = g.dm + la * N;
  const double* Ds = g.dm + si * N;
  const double fcd = la == si ? 0.5 : 1.0, dls = Dl[si];
  double jcd = 0.0, kbl[nsB], kbs[nsB];
  for (int b = 0; b < nsB; ++b) kbl[b] = kbs[b] = 0.0;
  for (int a = 0; a < nsA; ++a) {
    const int64_t mu = A.ao0 + a;
    double kal = 0.0, kas = 0.0;
    for (int b = 0; b < nsB; ++b) {
      if (sameAB && b > a) continue;
      const int64_t nu = B.ao0 + b;
      const int64_t ij = mu >= nu ? mu * (mu + 1) / 2 + nu : nu * (nu + 1) / 2 + mu;
      if (diag && kl > ij) continue;
      const double v = acc[a * nsB + b] * (fcd * (mu == nu ? 0.5 : 1.0) * (ij == kl ? 0.5 : 1.0));      // v'
      if (g.J) {
        jk_add_lower(g.J, N, mu, nu, 2.0 * v * dls);
        jcd += v * g.dm[mu * N + nu];
      }
      if (g.K) {
        kal += v * Ds[nu];          // T[mu,la] += v' D[nu,si]
        kas += v * Dl[nu];          // T[mu,si] += v' D[nu,la]
        kbl[b] += v * Ds[mu];       // T[nu,la] += v' D[mu,si]
        kbs[b] += v * Dl[mu];       // T[nu,si] += v' D[mu,la]
      }
    }
    if (g.K) {
      jk_add_lower(g.K, N, mu, la, kal);
      jk_add_lower(g.K, N, mu, si, kas);
    }
  }
  if (g.J) jk_add_lower(g.J, N, la, si, 2.0 * jcd);
  if (g.K)
    for (int b = 0; b < nsB; ++b) {
      jk_add_lower(g.K, N, B.ao0 + b, la, kbl[b]);
      jk_add_lower(g.K, N, B.ao0 + b, si, kbs[b]);
    }
}

}  // namespace int4c

// argument checks shared by the device layer and its scalar restatement
inline int int4c_check_pairs(int la, int lb, const int4c::PairArgs& g) {
  if (la < 0 || la > int4c::kMaxLOrb || lb < 0 || lb > la) {
    set_error("dev_int4c_pairs: unsupported pair class (" + std::to_string(la) + "," + std::to_string(lb) + ")");
    return QEMB_ERR_UNSUPPORTED;
  }
  if (g.pairs.n < 0 || !g.sh || !g.pairs.a || !g.pairs.b || !g.pairs.off || !g.c2s || !g.data) { set_error("dev_int4c_pairs: bad arguments"); return QEMB_ERR_ARG; }
  return 0;
}
inline int int4c_check_class(int la, int lb, int lc, int ld, const int4c::ClassArgs& g) {
  using namespace int4c;
  if (la < 0 || la > kMaxLOrb || lb < 0 || lb > la || lc < 0 || lc > kMaxLOrb || ld < 0 || ld > lc || pair_class(lc, ld) > pair_class(la, lb)) {
    set_error("dev_int4c_class: not a canonical angular class (" + std::to_string(la) + "," + std::to_string(lb) + "|" + std::to_string(lc) + "," + std::to_string(ld) + ")");
    return QEMB_ERR_UNSUPPORTED;
  }
  if (g.out != kBlock && g.out != kS1 && g.out != kDiag && g.out != kS4 && g.out != kS8 && g.out != kTile) { set_error("dev_int4c_class: unknown output form " + std::to_string(g.out)); return QEMB_ERR_ARG; }
  const bool same_class = la == lc && lb == ld;
  if ((g.same && !same_class) || (g.out == kDiag && !g.same)) { set_error("dev_int4c_class: one list on both sides needs equal pair classes"); return QEMB_ERR_ARG; }
  if (g.bra.n < 0 || g.ket.n < 0 || !g.sh || !g.data || !g.dst || !g.bra.a || !g.bra.b || !g.bra.off || !g.ket.a || !g.ket.b || !g.ket.off ||
      (g.out != kBlock && g.out != kDiag && g.N <= 0)) { set_error("dev_int4c_class: bad arguments"); return QEMB_ERR_ARG; }
  if (g.out == kTile && (!g.row || !g.col || g.ld <= 0 || g.store < kTileAsIs || g.store > kTileBoth || (g.same && g.store != kTileBoth))) {
    set_error("dev_int4c_class: a tile needs its row and column maps, a leading dimension and a store mode (both triangles when bra and ket are one list)");
    return QEMB_ERR_ARG;
  }
  return 0;
}
inline int int4c_check_pairprod(const int4c::PairProdArgs& g) {
  if (!g.TA || !g.mu || !g.nu || !g.P || g.n <= 0 || g.npq != g.n * (g.n + 1) / 2 || g.rows < 0 || g.npq > 0x7fffffffLL) { set_error("dev_int4c_pairprod: bad arguments"); return QEMB_ERR_ARG; }
  return 0;
}
inline int int4c_check_jk(int la, int lb, int lc, int ld, const int4c::JkArgs& g) {
  using namespace int4c;
  if (la < 0 || la > kMaxLOrb || lb < 0 || lb > la || lc < 0 || lc > kMaxLOrb || ld < 0 || ld > lc || pair_class(lc, ld) > pair_class(la, lb)) {
    set_error("dev_int4c_jk_class: not a canonical angular class (" + std::to_string(la) + "," + std::to_string(lb) + "|" + std::to_string(lc) + "," + std::to_string(ld) + ")");
    return QEMB_ERR_UNSUPPORTED;
  }
  if (g.same && !(la == lc && lb == ld)) { set_error("dev_int4c_jk_class: one list on both sides needs equal pair classes"); return QEMB_ERR_ARG; }
  if (g.bra.n < 0 || g.ket.n < 0 || !g.sh || !g.data || !g.dm || (!g.J && !g.K) || !g.bra.a || !g.bra.b || !g.bra.off || !g.ket.a || !g.ket.b || !g.ket.off || g.N <= 0 ||
      g.nshell <= 0) { set_error("dev_int4c_jk_class: bad arguments"); return QEMB_ERR_ARG; }
  return 0;
}

}  // namespace qemb
