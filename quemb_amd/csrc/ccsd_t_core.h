// ccsd_t_core.h -- the arithmetic of the perturbative triples correction E_(T) at one (i,j,k; a,b,c), written once for the assembly kernel of ccsd_t_ops.hip
// (one workgroup per (a,b,c)) and its scalar restatement for the mock device layer (ccsd_t_ops_hostcheck.cpp: the elements in a loop).
//
// Closed shell, Fock = diag(mo_energy), chemists' notation; i j k m occupied, a b c f virtual:
//   g[i,j,k,a,b,c] = sum_f (ia|fb) t2[k,j,c,f] - sum_m (ia|mj) t2[m,k,b,c]
//   W = the sum of g over the six simultaneous permutations of the pairs (i,a), (j,b), (k,c)
//   V = W + t1[i,a] (jb|kc) + t1[j,b] (ia|kc) + t1[k,c] (ia|jb)
//   E_(T) = 1/3 sum_{ijk,abc} W r3(V) / D,   r3(X)_ijk = 4 X_ijk + X_jki + X_kij - 2 X_kji - 2 X_ikj - 2 X_jik,   D = e_i + e_j + e_k - e_a - e_b - e_c
// The summand, summed over ijk, is invariant under the permutations of (a,b,c): only a >= b >= c is evaluated, with the number of distinct arrangements as
// the weight (6, 3 with two equal).  At a = b = c both W and V are invariant under every permutation of ijk and r3 of such a tensor is (4 + 1 + 1 - 2 - 2 - 2) = 0
// times it: those elements are identically zero and are not evaluated.  Hence no triples, and no launch, with fewer than two occupied or two virtual orbitals.
// r3 is evaluated as 2 (X_ijk - X_kji) + 2 (X_ijk - X_ikj) + (X_jki - X_jik) + (X_kij - X_jik): differences of nearby numbers, exactly 0 at i = j = k.
//
// Both parts of g come from the driver's products (ccsd_t.cpp): for a tile triple and each of the six arrangements (X,Y,Z) of its tiles a buffer
//   G_XYZ[x][y][p][z][r][q] = sum_f (p x|f y) t2[r,q,z,f] - sum_m t2[m,p,y,x] (r z|m q)      (x in X, y in Y, z in Z; p, r, q occupied)
// one product over K = v + o.  The first sum is the particle part of g[p,q,r,x,y,z]; the second is the hole part of g[r,q,p,z,y,x], the same three pairs
// (p,x), (q,y), (r,z) with the first and the third exchanged -- rows and columns of a product have to split as (x,y,p | z,r,q), and only this arrangement of
// the hole term does.  W adds the six arrangements of the pairs, so every particle part and every hole part is met once.
#pragma once
#include <cmath>
#include <cstdint>
#include "dev_ops.h"

#if defined(__HIPCC__)
#define QEMB_T_HD __host__ __device__ __forceinline__
#else
#define QEMB_T_HD inline
#endif

namespace qemb {

// What one launch of the assembly step works on: a tile triple A >= B >= C of the virtual orbitals (first indices a0, b0, c0, extents ta, tb, tc).
struct CcsdTArgs {
  int o, v;
  int a0, b0, c0, ta, tb, tc;
  const double* g[6];      // G_ABC, G_ACB, G_BAC, G_BCA, G_CAB, G_CBA (equal tiles: the same buffer under several names)
  const double *t1, *ovov, *eo, *ev;
  double* partial;         // [ta][tb][tc]: weight / 3 * sum_ijk W r3(V) / D of the element, 0 where it is not evaluated (ccsd_t_evaluated)
  double* scratch;         // occupied counts beyond the LDS form: 2 o^3 doubles per workgroup (W, then V)
};

// The LDS form of the assembly kernel: V, 8 o^3 bytes, within 64 KiB -- two workgroups of a CU's 160 KiB --, and at most kCcsdTPerThread elements of W in
// the registers of each of 1024 threads: o <= kCcsdTLdsMaxOcc = 20.  Beyond it: the global form.
constexpr int64_t kCcsdTLdsBytes = 64 * 1024;
constexpr int kCcsdTPerThread = 8;
constexpr int kCcsdTLdsMaxOcc = 20;
inline int64_t ccsd_t_lds_bytes(int64_t o) { return 8 * o * o * o; }
inline bool ccsd_t_lds_form(int64_t o) { return o <= kCcsdTLdsMaxOcc; }
static_assert(8 * 20 * 20 * 20 <= kCcsdTLdsBytes && 20 * 20 * 20 <= kCcsdTPerThread * 1024, "kCcsdTLdsMaxOcc must fit the LDS budget and the registers");
static_assert(8 * 21 * 21 * 21 > kCcsdTLdsBytes, "kCcsdTLdsMaxOcc is the largest count that fits");
inline int64_t ccsd_t_scratch_elems(int64_t o, int64_t tile) { return ccsd_t_lds_form(o) ? 0 : 2 * o * o * o * tile * tile * tile; }
inline const char* ccsd_t_args_error(const CcsdTArgs& A) {
  if (A.o < 1 || A.o > 1024 || A.v < 1) return "dev_ccsd_t_assemble: need 1 <= o <= 1024 and v >= 1";
  if (A.ta < 1 || A.tb < 1 || A.tc < 1 || A.a0 < 0 || A.b0 < 0 || A.c0 < 0 || A.a0 + A.ta > A.v || A.b0 + A.tb > A.v || A.c0 + A.tc > A.v) return "dev_ccsd_t_assemble: a tile outside the virtual orbitals";
  if ((int64_t)A.ta * A.tb * A.tc > 0x7fffffffLL) return "dev_ccsd_t_assemble: too many elements in one tile triple";
  for (int k = 0; k < 6; ++k) if (!A.g[k]) return "dev_ccsd_t_assemble: a product buffer is missing";
  if (!A.t1 || !A.ovov || !A.eo || !A.ev || !A.partial) return "dev_ccsd_t_assemble: bad arguments";
  if (!ccsd_t_lds_form(A.o) && !A.scratch) return "dev_ccsd_t_assemble: this occupied count needs the global scratch";
  return nullptr;
}

// the elements a launch evaluates, and the number of distinct arrangements of their (a,b,c)
QEMB_T_HD bool ccsd_t_evaluated(int a, int b, int c) { return a >= b && b >= c && a != c; }
QEMB_T_HD double ccsd_t_weight(int a, int b, int c) { return (a == b || b == c) ? 3.0 : 6.0; }

// W and V of one element; la, lb, lc: the virtual indices inside their tiles
QEMB_T_HD void ccsd_t_element(const CcsdTArgs& A, int la, int lb, int lc, int i, int j, int k, double* W_out, double* V_out) {
  const long long o = A.o, v = A.v, ta = A.ta, tb = A.tb, tc = A.tc;
  const long long a = A.a0 + la, b = A.b0 + lb, c = A.c0 + lc;
  // G[x][y][p][z][r][q] with the extents [.][ty][o][tz][o][o]: the six arrangements of the pairs (i,a), (j,b), (k,c)
  double w = A.g[0][((((la * tb + lb) * o + i) * tc + lc) * o + k) * o + j];      // (i,a) (j,b) (k,c)
  w += A.g[1][((((la * tc + lc) * o + i) * tb + lb) * o + j) * o + k];            // (i,a) (k,c) (j,b)
  w += A.g[2][((((lb * ta + la) * o + j) * tc + lc) * o + k) * o + i];            // (j,b) (i,a) (k,c)
  w += A.g[3][((((lb * tc + lc) * o + j) * ta + la) * o + i) * o + k];            // (j,b) (k,c) (i,a)
  w += A.g[4][((((lc * ta + la) * o + k) * tb + lb) * o + j) * o + i];            // (k,c) (i,a) (j,b)
  w += A.g[5][((((lc * tb + lb) * o + k) * ta + la) * o + i) * o + j];            // (k,c) (j,b) (i,a)
  const long long ov = o * v;
  double x = w;
  x = std::fma(A.t1[i * v + a], A.ovov[(j * v + b) * ov + k * v + c], x);
  x = std::fma(A.t1[j * v + b], A.ovov[(i * v + a) * ov + k * v + c], x);
  x = std::fma(A.t1[k * v + c], A.ovov[(i * v + a) * ov + j * v + b], x);
  *W_out = w;
  *V_out = x;
}

// r3 of V at (i,j,k); Vs: [i][j][k]
QEMB_T_HD double ccsd_t_r3(const double* Vs, int o, int i, int j, int k) {
  const int oo = o * o;
  const double x = Vs[i * oo + j * o + k], jik = Vs[j * oo + i * o + k];
  return 2.0 * ((x - Vs[k * oo + j * o + i]) + (x - Vs[i * oo + k * o + j])) + ((Vs[j * oo + k * o + i] - jik) + (Vs[k * oo + i * o + j] - jik));
}

}  // namespace qemb
