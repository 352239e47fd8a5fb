// loc_core.h -- the arithmetic of orbital localisation by joint diagonalisation (Boys, Pipek-Mezey, Edmiston-Ruedenberg on a 3-index factor), written once for
// the kernels of loc_ops.hip (one item per thread) and their scalar restatement for the mock device layer (loc_ops_hostcheck.cpp: the items in a loop).
//
// The problem: a stack Q[K][m][m] of symmetric matrices; find the orthogonal U that maximises f = sum_k sum_i (U^T Q^k U)_ii^2.  One plane rotation of the orbitals
// p' = c p + s q, q' = -s p + c q changes f by a function of theta alone: with a_k = Q^k_pq and d_k = (Q^k_pp - Q^k_qq) / 2 the new half difference is
// d'_k = cos(2 theta) d_k + sin(2 theta) a_k, the sum Q^k_pp + Q^k_qq is kept, so f(theta) = const + cos(4 theta) (sum d^2 - sum a^2) + sin(4 theta) (2 sum a d)
// and the maximum is at 4 theta = atan2(2 sum a d, sum d^2 - sum a^2), theta in (-pi/4, pi/4].  The atan2 form also leaves a pairwise saddle (sum a d = 0 with
// sum d^2 < sum a^2) by a turn of pi/4, which a small-angle formula would not.  A sweep is the m - 1 rounds of the circle-method tournament (rr_pair: the order of the
// Jacobi eigensolvers of linalg_f64.hip, a bye when m is odd); the rotations of a round are disjoint.
//
// THE VARIANTS AND THEIR LIMITS, stated here only:
//   in LDS   one workgroup of kThreads keeps the stack and U in LDS for the whole solve -- every sweep, one launch.  (K + 1) m^2 <= kLdsStackDoubles (56 KiB, which
//            with the 7 KiB of reduction scratch stays under the 64 KiB a workgroup may take and leaves a CU's 160 KiB room for a second workgroup).  With K >= 1
//            that is m <= kLdsMaxM = 59, so the m / 2 <= 30 pairs of a round times kLdsParts partial sums are one thread each.  Boys on a bath (K = 3): m <= 42.
//   rounds   everything else.  Two launches per round, one workgroup per slab of kSlab matrices: the partial sums of the slab, then -- every workgroup adds the
//            partials of all slabs in the same order and so holds the same angles -- the rotation of the slab's matrices, rows and then columns (U is matrix K of
//            the stack, columns only).  No workgroup waits on another inside a kernel; what a round needs from all of them is there when its launch begins.
// Every sum has one fixed order and no atomics: two calls give the same bits.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include "dev_ops.h"

#if defined(__HIPCC__)
#define QEMB_LOC_HD __host__ __device__ __forceinline__
#else
#define QEMB_LOC_HD inline
#endif

namespace qemb {
namespace loc {

constexpr int kThreads = 256;
constexpr int kLdsStackDoubles = 7168;      // (K + 1) m^2 doubles of the stack and U: 56 KiB
constexpr int kLdsMaxM = 59;                // what the stack limit leaves at K = 1 (a consequence, not a second limit): sizes the per-pair scratch
static_assert(2 * kLdsMaxM * kLdsMaxM <= kLdsStackDoubles && 2 * (kLdsMaxM + 1) * (kLdsMaxM + 1) > kLdsStackDoubles, "kLdsMaxM follows from kLdsStackDoubles");
constexpr int kLdsParts = 8;                // partial sums per pair in the one-workgroup variant: part s takes k = s, s + 8, ...
constexpr int kSlab = 16;                   // matrices per workgroup in the launch-per-round variant: slab b takes k = 16 b .. 16 b + 15
constexpr int kMaxM = 512;                  // rounds variant: the cosines, sines and indices of the m / 2 pairs of a round sit in 5 KiB of LDS.  A matrix is one workgroup's
                                            // work (m^3 per sweep on one CU: 0.5 s at m = 512 and K = 1); beyond that the rounds would have to be split over workgroups
inline bool in_lds(int64_t K, int64_t m) { return K >= 1 && (K + 1) * m * m <= kLdsStackDoubles; }
inline int64_t slabs(int64_t nmat) { return (nmat + kSlab - 1) / kSlab; }
// doubles of workspace: the four results of the one-workgroup variant; 3 partial sums per pair and slab, the sweep's largest |theta|, f and ||Q||^2 per slab
inline int64_t work_doubles(int64_t K, int64_t m) { return in_lds(K, m) ? 4 : 3 * slabs(K) * ((m + 1) / 2) + 1 + 2 * slabs(K); }
// the footprint of a call: the stack, U and the identity it starts from, and the workspace
inline double footprint_bytes(int64_t K, int64_t m) { return 8.0 * ((double)K * (double)m * (double)m + 2.0 * (double)m * (double)m + (double)work_doubles(K, m)); }
// a pair whose sums are this small against ||Q||^2 = sum_k ||Q^k||_F^2 holds rounding noise only (|a|, |d| below 1e-14 of the stack's norm): its angle would be
// the argument of noise, of any size, and no sweep would ever count as converged.  It is left alone; the gain forgone is below 2e-28 ||Q||^2.
constexpr double kNoiseFloor = 1.0e-28;

// round-robin pairing (circle method): np players (even), round r in [0, np - 1), slot j in [0, np / 2); p < q
QEMB_LOC_HD void rr_pair(int np, int r, int j, int& p, int& q) {
  const int n1 = np - 1;
  if (j == 0) { p = n1; q = r; }
  else { p = (r + j) % n1; q = (r - j + n1) % n1; }
  if (p > q) { const int t = p; p = q; q = t; }
}

// one matrix's terms of a pair's three sums
QEMB_LOC_HD void pair_terms(const double* Qk, int m, int p, int q, double& saa, double& sdd, double& sad) {
  const double a = Qk[(int64_t)p * m + q];
  const double d = 0.5 * (Qk[(int64_t)p * m + p] - Qk[(int64_t)q * m + q]);
  saa += a * a; sdd += d * d; sad += a * d;
}
// the angle of a pair from its sums (norm2 = ||Q||^2), theta in (-pi/4, pi/4]
QEMB_LOC_HD double pair_angle(double saa, double sdd, double sad, double norm2) {
  const double y = 2.0 * sad, x = sdd - saa;
  if (hypot(y, x) <= kNoiseFloor * norm2) return 0.0;
  return 0.25 * atan2(y, x);
}
// rows p and q of one matrix at column x; columns p and q at row x
QEMB_LOC_HD void rotate_rows(double* Qk, int m, int p, int q, int x, double c, double s) {
  const double u = Qk[(int64_t)p * m + x], v = Qk[(int64_t)q * m + x];
  Qk[(int64_t)p * m + x] = c * u + s * v;
  Qk[(int64_t)q * m + x] = c * v - s * u;
}
QEMB_LOC_HD void rotate_cols(double* Qk, int m, int p, int q, int x, double c, double s) {
  const double u = Qk[(int64_t)x * m + p], v = Qk[(int64_t)x * m + q];
  Qk[(int64_t)x * m + p] = c * u + s * v;
  Qk[(int64_t)x * m + q] = c * v - s * u;
}
// sum_i Q_ii^2 and sum_ij Q_ij^2 over the rows i0, i0 + stride, .. of one matrix, in index order (matrix_sums: all rows)
QEMB_LOC_HD void matrix_sums_rows(const double* Qk, int m, int i0, int stride, double& f, double& n2) {
  double a = 0.0, b = 0.0;
  for (int i = i0; i < m; i += stride) {
    for (int j = 0; j < m; ++j) { const double v = Qk[(int64_t)i * m + j]; b += v * v; }
    const double v = Qk[(int64_t)i * m + i];
    a += v * v;
  }
  f += a; n2 += b;
}
QEMB_LOC_HD void matrix_sums(const double* Qk, int m, double& f, double& n2) { matrix_sums_rows(Qk, m, 0, 1, f, n2); }

// who: the entry point, for the messages.  m beyond the launch-per-round variant's limit is a size the kernels do not serve: QEMB_ERR_UNSUPPORTED naming the limit
inline int check_joint_diag(const char* who, int64_t K, int64_t m, bool have_Q, bool have_U, double stop_angle, int max_sweeps) {
  if (K < 0 || m < 0 || K > 0x7fffffffLL || (m > 0 && !have_U) || (K > 0 && m > 0 && !have_Q) || !(stop_angle >= 0.0) || max_sweeps < 0) {
    set_error(std::string(who) + ": bad arguments (K = " + std::to_string(K) + ", m = " + std::to_string(m) + ")");
    return QEMB_ERR_ARG;
  }
  if (m > kMaxM) {
    set_error(std::string(who) + ": m = " + std::to_string(m) + " orbitals, but the sweeps serve m <= " + std::to_string(kMaxM) + " (K = " + std::to_string(K) + ")");
    return QEMB_ERR_UNSUPPORTED;
  }
  return 0;
}

}  // namespace loc
}  // namespace qemb
