// int3c_core.h -- one (shell pair | auxiliary shell) block of the 3-centre Coulomb integrals (mu nu|P), McMurchie-Davidson, as inline arithmetic that
// the gfx950 kernels (int3c_ops.hip: one thread per block) and the scalar restatement of the mock device layer (int3c_ops_hostcheck.cpp: a loop) both
// instantiate.  Same mathematics, normalisation and component order as the host source csrc_host/gto_ints.c behind integrals.aux_e2:
//   (ab|c) = sum_prim ca cb cc K_ab 2 pi^5/2 / (p q sqrt(p + q)) sum_{tuv} E^{ab}_{tuv} sum_{t'u'v'} (-1)^{t'+u'+v'} E^{c}_{t'u'v'} R_{t+t',u+u',v+v'}(alpha, P - C)
// (of the auxiliary expansion only the top term t' + u' + v' = l_P is carried: the others vanish in the solid-harmonic contraction, see block_cart)
// with Cartesian components in libcint order (xx xy xz yy yz zz ...), then the Cartesian -> real-spherical matrix of integrals.cart2sph on each centre.
// (P|Q) is the same block with a unit s function (exponent 0) as the second orbital shell -- what gto_eri_2c does.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include "dev_ops.h"

#if defined(__HIPCC__)
#define QEMB_I3_HD __host__ __device__ __forceinline__
#else
#define QEMB_I3_HD inline
#endif

namespace qemb {
namespace int3c {

constexpr int kMaxPrim = 8;      // integrals.MAXPRIM
constexpr int kMaxL = 4;         // auxiliary shells up to g; orbital shells up to d
constexpr int kC2sLen = 245;     // sum_l ncart(l) (2l + 1), l = 0..4

struct Shell {                   // one contracted shell; co carries primitive and contraction normalisation (the record of its first Cartesian component)
  double r[3];
  int l, nprim, ao0, pad;        // ao0: first (spherical) function of the shell
  double ex[kMaxPrim], co[kMaxPrim];
};

constexpr int ncart(int l) { return (l + 1) * (l + 2) / 2; }
constexpr int nsph(int l) { return 2 * l + 1; }
constexpr int nherm(int L) { return (L + 1) * (L + 2) * (L + 3) / 6; }
constexpr int c2s_off(int l) { return l == 0 ? 0 : c2s_off(l - 1) + ncart(l - 1) * nsph(l - 1); }
// Hermite index (t,u,v): grouped by order N = t + u + v, inside an order by s = u + v, then v
QEMB_I3_HD int hidx(int t, int u, int v) {
  const int s = u + v, N = t + s;
  return N * (N + 1) * (N + 2) / 6 + s * (s + 1) / 2 + v;
}

// Boys function F_0..F_nmax(x).  x < 35: the series of F_nmax (every term positive, so no cancellation; at most ~130 terms at x = 35) and downward
// recursion; x >= 35: F_0 = sqrt(pi / x) erf(sqrt x) / 2 -- the asymptotic form, erf = 1 to the last bit there -- and upward recursion, which is stable for
// x > m.  The switch at 35 and both branches are those of the host source, so the two sources differ by rounding only.
QEMB_I3_HD void boys(int nmax, double x, double* F) {
  const double et = exp(-x);
  if (x < 35.0) {
    double term = 1.0 / (2 * nmax + 1), sum = term;
    for (int i = 1; i < 200; ++i) {
      term *= 2.0 * x / (2 * nmax + 2 * i + 1);
      sum += term;
      if (term < 1e-17 * sum) break;
    }
    F[nmax] = et * sum;
    for (int m = nmax; m > 0; --m) F[m - 1] = (2.0 * x * F[m] + et) / (2 * m - 1);
  } else {
    F[0] = 0.5 * sqrt(3.14159265358979323846 / x) * erf(sqrt(x));
    for (int m = 0; m < nmax; ++m) F[m + 1] = ((2 * m + 1) * F[m] - et) / (2.0 * x);
  }
}

// R^0_{tuv}(alpha, X) for t + u + v <= L in ONE table: level n of the auxiliary index overwrites level n + 1 from the highest order down, so an entry
// of order N is formed from entries of order N - 1 and N - 2 that still hold level n + 1.
template <int L>
QEMB_I3_HD void rtable(double alpha, const double X[3], double* R) {
  double F[L + 1], pw[L + 1];
  boys(L, alpha * (X[0] * X[0] + X[1] * X[1] + X[2] * X[2]), F);
  pw[0] = 1.0;
  for (int n = 1; n <= L; ++n) pw[n] = pw[n - 1] * (-2.0 * alpha);
  for (int n = L; n >= 0; --n) {
    for (int N = L - n; N >= 1; --N)
      for (int t = 0; t <= N; ++t)
        for (int u = 0; u <= N - t; ++u) {
          const int v = N - t - u;
          double val;
          if (t > 0) {
            val = X[0] * R[hidx(t - 1, u, v)];
            if (t > 1) val += (t - 1) * R[hidx(t - 2, u, v)];
          } else if (u > 0) {
            val = X[1] * R[hidx(t, u - 1, v)];
            if (u > 1) val += (u - 1) * R[hidx(t, u - 2, v)];
          } else {
            val = X[2] * R[hidx(t, u, v - 1)];
            if (v > 1) val += (v - 1) * R[hidx(t, u, v - 2)];
          }
          R[hidx(t, u, v)] = val;
        }
    R[0] = pw[n] * F[n];
  }
}

// Hermite expansion coefficients of one Cartesian direction without the Gaussian-product factor (it is applied once, as K_ab):
// E[(i * (LB + 1) + j) * (LA + LB + 1) + t], XPA = P - A, XPB = P - B, h = 1 / (2 p)
template <int LA, int LB>
QEMB_I3_HD void hermite_e(double h, double XPA, double XPB, double* E) {
  constexpr int NT = LA + LB + 1;
  for (int k = 0; k < (LA + 1) * (LB + 1) * NT; ++k) E[k] = 0.0;
  E[0] = 1.0;
  auto at = [&](int i, int j, int t) -> double { return (t < 0 || t > i + j) ? 0.0 : E[(i * (LB + 1) + j) * NT + t]; };
  for (int i = 1; i <= LA; ++i)
    for (int t = 0; t <= i; ++t) E[(i * (LB + 1)) * NT + t] = h * at(i - 1, 0, t - 1) + XPA * at(i - 1, 0, t) + (t + 1) * at(i - 1, 0, t + 1);
  for (int i = 0; i <= LA; ++i)
    for (int j = 1; j <= LB; ++j)
      for (int t = 0; t <= i + j; ++t)
        E[(i * (LB + 1) + j) * NT + t] = h * at(i, j - 1, t - 1) + XPB * at(i, j - 1, t) + (t + 1) * at(i, j - 1, t + 1);
}

// The Cartesian block acc[(ia * ncart(LB) + ib) * ncart(LP) + ic] of the shells A, B (orbital pair) and C (auxiliary), summed over primitive triples.
// harmonic_a (the metric: B is the unit s function, so A alone is a solid-harmonic Gaussian after block_to_sph): the top Hermite term of role A only, as for C.
template <int LA, int LB, int LP>
QEMB_I3_HD void block_cart(const Shell& A, const Shell& B, const Shell& Cs, double* acc, bool harmonic_a = false) {
  constexpr int LAB = LA + LB, L = LAB + LP, NTA = LAB + 1, ncB = ncart(LB), ncP = ncart(LP);
  constexpr double kPref = 34.98683665524972497;      // 2 pi^(5/2)
  for (int k = 0; k < ncart(LA) * ncB * ncP; ++k) acc[k] = 0.0;
  const double AB[3] = {A.r[0] - B.r[0], A.r[1] - B.r[1], A.r[2] - B.r[2]};
  const double ab2 = AB[0] * AB[0] + AB[1] * AB[1] + AB[2] * AB[2];
  double Ex[(LA + 1) * (LB + 1) * NTA], Ey[(LA + 1) * (LB + 1) * NTA], Ez[(LA + 1) * (LB + 1) * NTA];
  double Ec[(LP + 1) * (LP + 1)], R[nherm(L)], G[nherm(LAB)];
  for (int pc = 0; pc < Cs.nprim; ++pc) {
    const double q = Cs.ex[pc];
    hermite_e<LP, 0>(0.5 / q, 0.0, 0.0, Ec);      // Ec[i * (LP + 1) + t]: the auxiliary function times a unit s function on its own centre
    for (int pa = 0; pa < A.nprim; ++pa)
      for (int pb = 0; pb < B.nprim; ++pb) {
        const double a = A.ex[pa], b = B.ex[pb], p = a + b, h = 0.5 / p;
        const double Kab = exp(-(a * b / p) * ab2);
        double PC[3];
        for (int d = 0; d < 3; ++d) PC[d] = (a * A.r[d] + b * B.r[d]) / p - Cs.r[d];
        hermite_e<LA, LB>(h, -(b / p) * AB[0], (a / p) * AB[0], Ex);
        hermite_e<LA, LB>(h, -(b / p) * AB[1], (a / p) * AB[1], Ey);
        hermite_e<LA, LB>(h, -(b / p) * AB[2], (a / p) * AB[2], Ez);
        rtable<L>(p * q / (p + q), PC, R);
        const double pref = A.co[pa] * B.co[pb] * Cs.co[pc] * Kab * kPref / (p * q * sqrt(p + q));
        int ic = 0;
        for (int cx = LP; cx >= 0; --cx)
          for (int cy = LP - cx; cy >= 0; --cy, ++ic) {
            const int cz = LP - cx - cy;
            // G_{tuv} = pref sum_{t'u'v'} (-1)^{t'+u'+v'} E^c R_{t+t',u+u',v+v'}: the auxiliary component folded into the Hermite integrals
            for (int t = 0; t <= LAB; ++t)
              for (int u = 0; u <= LAB - t; ++u)
                for (int v = 0; v <= LAB - t - u; ++v) {
                  // only the top Hermite term t' = cx, u' = cy, v' = cz: block_to_sph contracts the component with a harmonic polynomial, and
                  // S_lm(r) exp(-q r^2) = (2q)^-l S_lm(d/dC) exp(-q r^2), so the lower terms sum to zero there.  Carrying them would subtract Cartesian
                  // integrals that keep the R^-1 ... R^-l parts from one another: 1e-10 of a far (g|g) block as rounding.  (s, p: the only term anyway.)
                  const double g = Ec[cx * (LP + 1) + cx] * Ec[cy * (LP + 1) + cy] * Ec[cz * (LP + 1) + cz] * R[hidx(t + cx, u + cy, v + cz)];
                  G[hidx(t, u, v)] = (LP & 1) ? -pref * g : pref * g;      // t' + u' + v' = LP
                }
            int ia = 0;
            for (int ax = LA; ax >= 0; --ax)
              for (int ay = LA - ax; ay >= 0; --ay, ++ia) {
                const int az = LA - ax - ay;
                int ib = 0;
                for (int bx = LB; bx >= 0; --bx)
                  for (int by = LB - bx; by >= 0; --by, ++ib) {
                    const int bz = LB - bx - by;
                    const double* ex = Ex + (ax * (LB + 1) + bx) * NTA;
                    const double* ey = Ey + (ay * (LB + 1) + by) * NTA;
                    const double* ez = Ez + (az * (LB + 1) + bz) * NTA;
                    double s = 0.0;
                    for (int t = harmonic_a ? ax : 0; t <= ax + bx; ++t)
                      for (int u = harmonic_a ? ay : 0; u <= ay + by; ++u) {
                        const double e2 = ex[t] * ey[u];
                        for (int v = harmonic_a ? az : 0; v <= az + bz; ++v) s += e2 * ez[v] * G[hidx(t, u, v)];
                      }
                    acc[(ia * ncB + ib) * ncP + ic] += s;
                  }
              }
          }
      }
  }
}

// Cartesian -> real spherical on the three centres, in place: afterwards the value of (a, b, m) is acc[(a * ncart(LB) + b) * ncart(LP) + m] for
// a < 2 LA + 1, b < 2 LB + 1, m < 2 LP + 1 (the strides stay Cartesian).  c2s: the matrices of integrals.cart2sph, l = 0..4, each ncart x (2l + 1) row-major.
template <int LA, int LB, int LP>
QEMB_I3_HD void block_to_sph(double* acc, const double* c2s) {
  constexpr int ncA = ncart(LA), ncB = ncart(LB), ncP = ncart(LP);
  if (LP >= 2) {
    const double* M = c2s + c2s_off(LP);
    for (int r = 0; r < ncA * ncB; ++r) {
      double tmp[nsph(LP)];
      for (int m = 0; m < nsph(LP); ++m) {
        double s = 0.0;
        for (int ic = 0; ic < ncP; ++ic) s += acc[r * ncP + ic] * M[ic * nsph(LP) + m];
        tmp[m] = s;
      }
      for (int m = 0; m < nsph(LP); ++m) acc[r * ncP + m] = tmp[m];
    }
  }
  if (LB >= 2) {
    const double* M = c2s + c2s_off(LB);
    for (int ia = 0; ia < ncA; ++ia)
      for (int m = 0; m < nsph(LP); ++m) {
        double tmp[nsph(LB)];
        for (int jb = 0; jb < nsph(LB); ++jb) {
          double s = 0.0;
          for (int ib = 0; ib < ncB; ++ib) s += acc[(ia * ncB + ib) * ncP + m] * M[ib * nsph(LB) + jb];
          tmp[jb] = s;
        }
        for (int jb = 0; jb < nsph(LB); ++jb) acc[(ia * ncB + jb) * ncP + m] = tmp[jb];
      }
  }
  if (LA >= 2) {
    const double* M = c2s + c2s_off(LA);
    for (int ib = 0; ib < nsph(LB); ++ib)
      for (int m = 0; m < nsph(LP); ++m) {
        double tmp[nsph(LA)];
        for (int ja = 0; ja < nsph(LA); ++ja) {
          double s = 0.0;
          for (int ia = 0; ia < ncA; ++ia) s += acc[(ia * ncB + ib) * ncP + m] * M[ia * nsph(LA) + ja];
          tmp[ja] = s;
        }
        for (int ja = 0; ja < nsph(LA); ++ja) acc[(ja * ncB + ib) * ncP + m] = tmp[ja];
      }
  }
}

// ---- one launch: the blocks of one angular class -------------------------------------------------------------------------------------------
enum Layout { kPqL = 0, kLpq = 1, kPacked = 2, kPairs = 3, kBlock = 4, kMetric = 5 };

struct ClassArgs {
  const Shell* orb;            // orbital shells (kMetric: the auxiliary shells)
  const Shell* aux;
  const int32_t* pa;           // per shell pair of the class: the shell in role A (l = LA >= LB) and in role B; pa == pb: a block inside one shell
  const int32_t* pb;
  const int32_t* ps;           // auxiliary shells of the class (l = LP)
  int64_t npair, naux_sh;
  const double* c2s;
  double* out;
  int layout;
  int swapped;                 // kBlock: the caller's first shell plays role B
  int unit;                    // kMetric: index in `orb` of a unit s function (one primitive, exponent 0, coefficient 1), role B of (P|Q)
  int64_t N, naux;             // functions of the orbital / auxiliary basis
  const int64_t* ent_ptr;      // kPairs: per shell pair of the class, entries [ent_ptr[k], ent_ptr[k + 1])
  const int32_t* ent_ab;       //   (a, b) inside the block, a >= b when pa == pb
  const int64_t* ent_row;      //   row of `out` (n_pairs x naux)
};

// Every element of `out` that belongs to the item is written exactly once, by plain stores: the same bits run to run.
template <int LA, int LB, int LP>
QEMB_I3_HD void class_item(const ClassArgs& g, int64_t item) {
  constexpr int ncB = ncart(LB), ncP = ncart(LP), nsA = nsph(LA), nsB = nsph(LB), nsP = nsph(LP);
  // neighbouring items write neighbouring addresses: the auxiliary shell runs fastest where the auxiliary index is contiguous in `out`
  const bool aux_fast = g.layout == kPqL || g.layout == kPairs || g.layout == kMetric;
  const int64_t k = aux_fast ? item / g.naux_sh : item % g.npair;
  const int64_t s = aux_fast ? item % g.naux_sh : item / g.npair;
  double acc[ncart(LA) * ncB * ncP];
  const Shell& C = g.aux[g.ps[s]];      // the shells are read in place: a private copy indexed by the primitive loops would live in scratch
  const int64_t P0 = C.ao0;
  if (g.layout == kMetric) {      // (P|Q): role A = the auxiliary shell pa[k], role B = a unit s function, any centre (its exponent is 0)
    if (g.ps[s] > g.pa[k]) return;      // the lower triangle of shell pairs is computed, the upper one is its copy
    const Shell& A = g.orb[g.pa[k]];
    const Shell& U = g.orb[g.unit];
    block_cart<LA, LB, LP>(A, U, C, acc, true);
    block_to_sph<LA, LB, LP>(acc, g.c2s);
    const bool same = g.pa[k] == g.ps[s];
    for (int a = 0; a < nsA; ++a)
      for (int m = 0; m < nsP; ++m) {
        if (same && m > a) continue;
        const double v = acc[a * ncB * ncP + m];
        const int64_t mu = A.ao0 + a, nu = P0 + m;
        g.out[mu * g.naux + nu] = v;
        if (mu != nu) g.out[nu * g.naux + mu] = v;
      }
    return;
  }
  const Shell& A = g.orb[g.pa[k]];
  const Shell& B = g.orb[g.pb[k]];
  block_cart<LA, LB, LP>(A, B, C, acc);
  block_to_sph<LA, LB, LP>(acc, g.c2s);
  const bool same = g.pa[k] == g.pb[k];
  if (g.layout == kPairs) {
    for (int64_t e = g.ent_ptr[k]; e < g.ent_ptr[k + 1]; ++e) {
      const int a = g.ent_ab[2 * e], b = g.ent_ab[2 * e + 1];
      double* row = g.out + g.ent_row[e] * g.naux + P0;
      for (int m = 0; m < nsP; ++m) row[m] = acc[(a * ncB + b) * ncP + m];
    }
    return;
  }
  const int64_t N = g.N, np = N * (N + 1) / 2;
  for (int a = 0; a < nsA; ++a)
    for (int b = 0; b < nsB; ++b) {
      if (same && b > a) continue;      // a block inside one shell: the lower triangle is computed, the upper one is its copy
      const int64_t mu = A.ao0 + a, nu = B.ao0 + b;
      for (int m = 0; m < nsP; ++m) {
        const double v = acc[(a * ncB + b) * ncP + m];
        const int64_t P = P0 + m;
        switch (g.layout) {
          case kPqL:
            g.out[(mu * N + nu) * g.naux + P] = v;
            if (mu != nu) g.out[(nu * N + mu) * g.naux + P] = v;
            break;
          case kLpq:
            g.out[(P * N + mu) * N + nu] = v;
            if (mu != nu) g.out[(P * N + nu) * N + mu] = v;
            break;
          case kPacked:
            g.out[P * np + (mu > nu ? mu * (mu + 1) / 2 + nu : nu * (nu + 1) / 2 + mu)] = v;
            break;
          default:      // kBlock: one explicit block in the caller's shell order
            g.out[((g.swapped ? b * nsA + a : a * nsB + b)) * nsP + m] = v;
            break;
        }
      }
    }
}

}  // namespace int3c

// argument checks shared by the device layer and its scalar restatement
inline int int3c_check_boys(int m_max, int64_t n, const void* x, const void* out) {
  if (m_max < 0 || m_max > 2 * int3c::kMaxL + 4 || n < 0 || (n > 0 && (!x || !out))) { set_error("dev_boys: need 0 <= m_max <= 12 and non-null arrays"); return QEMB_ERR_ARG; }
  return 0;
}
inline int int3c_check_class(int la, int lb, int lp, const int3c::ClassArgs& g) {
  using namespace int3c;
  const bool metric = g.layout == kMetric;
  if (la < 0 || lb < 0 || lb > la || lp < 0 || lp > kMaxL || la > (metric ? kMaxL : 2) || (metric && lb != 0)) {
    set_error("dev_int3c_class: unsupported angular class (" + std::to_string(la) + "," + std::to_string(lb) + "|" + std::to_string(lp) + ")");
    return QEMB_ERR_UNSUPPORTED;
  }
  if (g.layout < kPqL || g.layout > kMetric) { set_error("dev_int3c_class: unknown layout " + std::to_string(g.layout)); return QEMB_ERR_ARG; }
  if (g.npair < 0 || g.naux_sh < 0 || !g.orb || !g.aux || !g.pa || (!metric && !g.pb) || (metric && g.unit < 0) || !g.ps || !g.c2s || !g.out || g.naux <= 0 || (!metric && g.layout != kBlock && g.N <= 0) ||
      (g.layout == kPairs && (!g.ent_ptr || !g.ent_ab || !g.ent_row))) { set_error("dev_int3c_class: bad arguments"); return QEMB_ERR_ARG; }
  return 0;
}

}  // namespace qemb
