// int1e_core.h -- the one-electron integrals of a contracted shell pair: overlap S, kinetic energy T and nuclear attraction V = sum_C -Z_C <a|1/r_C|b>, as inline
// arithmetic that the gfx950 kernel (int1e_ops.hip: one wavefront per shell pair) and the scalar restatement of the mock device layer (int1e_ops_hostcheck.cpp:
// a loop over the same 64 "lanes") both instantiate.  Same mathematics, normalisation and component order as the host source csrc_host/gto_ints.c behind
// Mole.one_electron(); it sits on boys / rtable / hermite_e of int3c_core.h the way int4c_core.h does.
//   S_ab = sum_prim ca cb K_ab sx sy sz,  s_ij the 1-D overlaps by the Obara-Saika recursion from s_00 = sqrt(pi / p)
//   T_ab = sum_prim ca cb K_ab (tx sy sz + sx ty sz + sx sy tz),  t_ij = -2 b^2 s_{i,j+2} + b (2j + 1) s_ij - j (j - 1) / 2 s_{i,j-2}
//   <a|x - o_x|b> = sum_prim ca cb K_ab (s_{i,j+1} + (B_x - o_x) s_ij) sy sz  (x - o_x = (x - B_x) + (B_x - o_x)), likewise y and z: the 1-D overlaps S forms, one order up
//   V_ab = sum_C -Z_C sum_prim ca cb K_ab 2 pi / p sum_{tuv} E^x_t E^y_u E^z_v R_tuv(p, P - C)
// The work of a shell pair is dealt to kLanes lanes: lane w takes the items w, w + kLanes, .. of the list (primitive pair) for S and T and (primitive pair, atom), the
// atom fastest, for V, and keeps a private Cartesian block of at most 36 doubles.  The kLanes partial blocks are added up by a binary tree in a fixed order
// (lane w += lane w + off, off = 32, 16, .. 1), then the Cartesian -> spherical matrices are applied and every element is stored once: the same bits on every run.
#pragma once
#include "int3c_core.h"

namespace qemb {
namespace int1e {

using int3c::Shell;
using int3c::ncart;
using int3c::nsph;
using int3c::nherm;
using int3c::hidx;

constexpr int kLanes = 64;                 // one gfx950 wavefront
constexpr int kMaxBlock = 36;              // ncart(2)^2
enum Kind { kOverlap = 0, kKinetic = 1, kNuclear = 2, kDipoleX = 3, kDipoleY = 4, kDipoleZ = 5, kKinds = 6 };

struct Args {
  const Shell* sh;             // the shells of the basis (device)
  const int32_t* pa;           // per shell pair of the class: the shell in role A (l = LA >= LB) and in role B; pa == pb: a block inside one shell
  const int32_t* pb;
  int64_t npair;
  const double* c2s;
  int natm;
  const double* xyz;           // 3 natm: the nuclei (Bohr)
  const double* Z;             // natm: their charges
  double* out[kKinds];         // S, T, V, then <a|x - o_x|b>, <a|y - o_y|b>, <a|z - o_z|b> (N x N each; a null matrix is not computed)
  double origin[3];            // o of the dipole integrals (Bohr)
  int64_t N;
};

// 1-D overlaps without the Gaussian-product factor: s[i * (LB + 1) + j], i <= LA, j <= LB, h = 1 / (2p), XPA = P - A, XPB = P - B
template <int LA, int LB>
QEMB_I3_HD void overlap_1d(double h, double XPA, double XPB, double s00, double* s) {
  constexpr int W = LB + 1;
  s[0] = s00;
  for (int i = 0; i < LA; ++i) s[(i + 1) * W] = XPA * s[i * W] + (i > 0 ? h * i * s[(i - 1) * W] : 0.0);
  for (int j = 0; j < LB; ++j)
    for (int i = 0; i <= LA; ++i) {
      double v = XPB * s[i * W + j];
      if (i > 0) v += h * i * s[(i - 1) * W + j];
      if (j > 0) v += h * j * s[i * W + j - 1];
      s[i * W + j + 1] = v;
    }
}

// lane's share of the Cartesian block acc[ia * ncart(LB) + ib] of S (KIND = kOverlap), T (kKinetic) or a dipole component (kDipoleX ..): the primitive pairs lane,
// lane + nlanes, ..
template <int LA, int LB, int KIND>
QEMB_I3_HD void st_partial(const Shell& A, const Shell& B, const double* origin, int lane, int nlanes, double* acc) {
  constexpr int ncB = ncart(LB), W = LB + 3;
  for (int k = 0; k < ncart(LA) * ncB; ++k) acc[k] = 0.0;
  const double AB[3] = {A.r[0] - B.r[0], A.r[1] - B.r[1], A.r[2] - B.r[2]};
  const double ab2 = AB[0] * AB[0] + AB[1] * AB[1] + AB[2] * AB[2];
  double s[3][(LA + 1) * W], t[3][(LA + 1) * (LB + 1)];
  for (int item = lane; item < A.nprim * B.nprim; item += nlanes) {
    const int ia_ = item / B.nprim, ib_ = item % B.nprim;
    const double a = A.ex[ia_], b = B.ex[ib_], p = a + b, h = 0.5 / p;
    const double pref = A.co[ia_] * B.co[ib_] * exp(-(a * b / p) * ab2);
    const double s00 = sqrt(3.14159265358979323846 / p);
    for (int d = 0; d < 3; ++d) {
      overlap_1d<LA, LB + 2>(h, -(b / p) * AB[d], (a / p) * AB[d], s00, s[d]);
      if (KIND == kKinetic)
        for (int i = 0; i <= LA; ++i)
          for (int j = 0; j <= LB; ++j) {
            double v = -2.0 * b * b * s[d][i * W + j + 2] + b * (2 * j + 1) * s[d][i * W + j];
            if (j >= 2) v -= 0.5 * j * (j - 1) * s[d][i * W + j - 2];
            t[d][i * (LB + 1) + j] = v;
          }
    }
    int ia = 0;
    for (int ax = LA; ax >= 0; --ax)
      for (int ay = LA - ax; ay >= 0; --ay, ++ia) {
        const int az = LA - ax - ay;
        int ib = 0;
        for (int bx = LB; bx >= 0; --bx)
          for (int by = LB - bx; by >= 0; --by, ++ib) {
            const int bz = LB - bx - by;
            const double sx = s[0][ax * W + bx], sy = s[1][ay * W + by], sz = s[2][az * W + bz];
            double v;
            if (KIND == kKinetic) v = t[0][ax * (LB + 1) + bx] * sy * sz + sx * t[1][ay * (LB + 1) + by] * sz + sx * sy * t[2][az * (LB + 1) + bz];
            else if (KIND == kDipoleX) v = (s[0][ax * W + bx + 1] + (B.r[0] - origin[0]) * sx) * sy * sz;
            else if (KIND == kDipoleY) v = sx * (s[1][ay * W + by + 1] + (B.r[1] - origin[1]) * sy) * sz;
            else if (KIND == kDipoleZ) v = sx * sy * (s[2][az * W + bz + 1] + (B.r[2] - origin[2]) * sz);
            else v = sx * sy * sz;
            acc[ia * ncB + ib] += pref * v;
          }
      }
  }
}

// lane's share of the Cartesian block of V: the items (primitive pair, atom) lane, lane + nlanes, .. with the atom fastest, so that consecutive items of a lane
// that share the primitive pair share its Hermite expansion
template <int LA, int LB>
QEMB_I3_HD void v_partial(const Shell& A, const Shell& B, int natm, const double* xyz, const double* Z, int lane, int nlanes, double* acc) {
  constexpr int L = LA + LB, NT = L + 1, ncB = ncart(LB), nE = (LA + 1) * (LB + 1) * NT;
  for (int k = 0; k < ncart(LA) * ncB; ++k) acc[k] = 0.0;
  const double AB[3] = {A.r[0] - B.r[0], A.r[1] - B.r[1], A.r[2] - B.r[2]};
  const double ab2 = AB[0] * AB[0] + AB[1] * AB[1] + AB[2] * AB[2];
  double Ex[nE], Ey[nE], Ez[nE], R[nherm(L)], P[3] = {0.0, 0.0, 0.0};
  double p = 1.0, pref = 0.0;
  int last = -1;
  const int64_t nitem = (int64_t)A.nprim * B.nprim * natm;
  for (int64_t item = lane; item < nitem; item += nlanes) {
    const int pp = (int)(item / natm), c = (int)(item % natm);
    if (pp != last) {
      last = pp;
      const int ia_ = pp / B.nprim, ib_ = pp % B.nprim;
      const double a = A.ex[ia_], b = B.ex[ib_];
      p = a + b;
      for (int d = 0; d < 3; ++d) P[d] = (a * A.r[d] + b * B.r[d]) / p;
      int3c::hermite_e<LA, LB>(0.5 / p, -(b / p) * AB[0], (a / p) * AB[0], Ex);
      int3c::hermite_e<LA, LB>(0.5 / p, -(b / p) * AB[1], (a / p) * AB[1], Ey);
      int3c::hermite_e<LA, LB>(0.5 / p, -(b / p) * AB[2], (a / p) * AB[2], Ez);
      pref = A.co[ia_] * B.co[ib_] * exp(-(a * b / p) * ab2) * (2.0 * 3.14159265358979323846 / p);
    }
    const double PC[3] = {P[0] - xyz[3 * c], P[1] - xyz[3 * c + 1], P[2] - xyz[3 * c + 2]};
    int3c::rtable<L>(p, PC, R);
    const double w = -Z[c] * pref;
    int ia = 0;
    for (int ax = LA; ax >= 0; --ax)
      for (int ay = LA - ax; ay >= 0; --ay, ++ia) {
        const int az = LA - ax - ay;
        int ib = 0;
        for (int bx = LB; bx >= 0; --bx)
          for (int by = LB - bx; by >= 0; --by, ++ib) {
            const int bz = LB - bx - by;
            const double* ex = Ex + (ax * (LB + 1) + bx) * NT;
            const double* ey = Ey + (ay * (LB + 1) + by) * NT;
            const double* ez = Ez + (az * (LB + 1) + bz) * NT;
            double s = 0.0;
            for (int t = 0; t <= ax + bx; ++t)
              for (int u = 0; u <= ay + by; ++u) {
                const double e2 = ex[t] * ey[u];
                for (int v = 0; v <= az + bz; ++v) s += e2 * ez[v] * R[hidx(t, u, v)];
              }
            acc[ia * ncB + ib] += w * s;
          }
      }
  }
}

template <int LA, int LB>
QEMB_I3_HD void partial(int kind, const Args& g, int64_t k, int lane, int nlanes, double* acc) {
  const Shell& A = g.sh[g.pa[k]];
  const Shell& B = g.sh[g.pb[k]];
  if (kind == kOverlap) st_partial<LA, LB, kOverlap>(A, B, g.origin, lane, nlanes, acc);
  else if (kind == kKinetic) st_partial<LA, LB, kKinetic>(A, B, g.origin, lane, nlanes, acc);
  else if (kind == kDipoleX) st_partial<LA, LB, kDipoleX>(A, B, g.origin, lane, nlanes, acc);
  else if (kind == kDipoleY) st_partial<LA, LB, kDipoleY>(A, B, g.origin, lane, nlanes, acc);
  else if (kind == kDipoleZ) st_partial<LA, LB, kDipoleZ>(A, B, g.origin, lane, nlanes, acc);
  else v_partial<LA, LB>(A, B, g.natm, g.xyz, g.Z, lane, nlanes, acc);
}

// The summed Cartesian block of pair k -> real-spherical, stored with its mirror image: out[mu][nu] = out[nu][mu].  Inside one shell the lower triangle of the
// block is stored and mirrored.  Every element of the matrix belongs to one shell pair and is written once, so the matrix is symmetric to the bit.
template <int LA, int LB>
QEMB_I3_HD void store_block(const Args& g, int64_t k, double* out, double* acc) {
  constexpr int ncB = ncart(LB);
  int3c::block_to_sph<LA, LB, 0>(acc, g.c2s);
  const Shell& A = g.sh[g.pa[k]];
  const Shell& B = g.sh[g.pb[k]];
  const bool same = g.pa[k] == g.pb[k];
  for (int a = 0; a < nsph(LA); ++a)
    for (int b = 0; b < nsph(LB); ++b) {
      if (same && b > a) continue;
      const int64_t mu = A.ao0 + a, nu = B.ao0 + b;
      const double v = acc[a * ncB + b];
      out[mu * g.N + nu] = v;
      if (mu != nu) out[nu * g.N + mu] = v;
    }
}

}  // namespace int1e

// argument check shared by the device layer and its scalar restatement
inline int int1e_check_class(int la, int lb, const int1e::Args& g) {
  if (la < 0 || la > 2 || lb < 0 || lb > la) { set_error("dev_int1e_class: unsupported pair class (" + std::to_string(la) + "," + std::to_string(lb) + ")"); return QEMB_ERR_UNSUPPORTED; }
  if (g.npair < 0 || g.npair > 0x7fffffffLL || !g.sh || !g.pa || !g.pb || !g.c2s || g.N <= 0 || g.natm < 0 || (g.out[int1e::kNuclear] && g.natm > 0 && (!g.xyz || !g.Z))) {
    set_error("dev_int1e_class: bad arguments"); return QEMB_ERR_ARG;
  }
  return 0;
}

}  // namespace qemb
