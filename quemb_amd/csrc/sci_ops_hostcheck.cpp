// sci_ops_hostcheck.cpp -- scalar restatement of the device operations of the selected CI for the mock device layer of tests/hostcheck.
// Everything below is compiled only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and sci_ops.hip provides the operations.
// The screen walks the lanes of sci_core.h one after another (the same output positions as the kernel); the sort is std::sort, the merge a two-finger merge,
// the matrix the kernel's walk over the runs of equal alpha (the tests hold the pattern to an all-pairs popcount in numpy), the product and the RDMs plain loops over the rows; the second-order rows and their sum keep the kernel's lanes and trees (the same order of additions).
#ifdef QEMB_HOSTCHECK
#include <algorithm>
#include <utility>
#include <vector>
#include "cumulant_core.h"
#include "sci_core.h"

namespace qemb {

static int screen(const char* who, int n, const double* h, const double* V, int64_t nd, const uint64_t* keys, const double* c, double eps, double dbl_bound,
                  int32_t* counts, const int64_t* offsets, uint64_t* out, uint64_t lo, uint64_t hi) {
  if (n <= 0 || n > kSciMaxOrb || !h || !V || !keys || !c || nd <= 0 || !(eps > 0.0) || (!counts && !(offsets && out))) { set_error(std::string(who) + ": bad arguments"); return QEMB_ERR_ARG; }
  for (int64_t d = 0; d < nd; ++d) {
    SciLists L;
    sci_lists(n, keys[2 * d], keys[2 * d + 1], &L);
    for (int lane = 0; lane < kSciScreenLanes; ++lane) {
      const int64_t slot = d * kSciScreenLanes + lane;
      if (counts) counts[slot] = sci_screen_lane(n, h, V, L, keys[2 * d], keys[2 * d + 1], c[d], eps, dbl_bound, lane, kSciScreenLanes, [](int, uint64_t, uint64_t) {});
      else {
        uint64_t* o = out + 4 * offsets[slot];
        sci_screen_lane(n, h, V, L, keys[2 * d], keys[2 * d + 1], c[d], eps, dbl_bound, lane, kSciScreenLanes,
                        [o, lo, hi](int k, uint64_t na, uint64_t nb) { sci_put_in_range(o + 4 * k, na, nb, lo, hi); sci_put_in_range(o + 4 * k + 2, nb, na, lo, hi); });
      }
    }
  }
  return 0;
}
int dev_sci_screen_count(int n, const double* h, const double* V, int64_t nd, const uint64_t* keys, const double* c, double eps, double dbl_bound, int32_t* counts) {
  if (!counts) { set_error("dev_sci_screen_count: bad arguments"); return QEMB_ERR_ARG; }
  return screen("dev_sci_screen_count", n, h, V, nd, keys, c, eps, dbl_bound, counts, nullptr, nullptr, 0, ~(uint64_t)0);
}
int dev_sci_screen_emit(int n, const double* h, const double* V, int64_t nd, const uint64_t* keys, const double* c, double eps, double dbl_bound, const int64_t* offsets, uint64_t* out,
                        uint64_t alpha_lo, uint64_t alpha_hi) {
  if (!offsets || !out) { set_error("dev_sci_screen_emit: bad arguments"); return QEMB_ERR_ARG; }
  return screen("dev_sci_screen_emit", n, h, V, nd, keys, c, eps, dbl_bound, nullptr, offsets, out, alpha_lo, alpha_hi);
}
int dev_sci_scan(int64_t m, const int32_t* in, int64_t* out) {
  if (m <= 0 || !in || !out) { set_error("dev_sci_scan: bad arguments"); return QEMB_ERR_ARG; }
  int64_t s = 0;
  for (int64_t k = 0; k < m; ++k) { out[k] = s; s += in[k]; }
  out[m] = s;
  return 0;
}
int dev_sci_sort(int64_t m, int64_t mpad, uint64_t* keys) {
  if (m < 0 || mpad < m || mpad < 1 || (mpad & (mpad - 1)) || !keys) { set_error("dev_sci_sort: bad arguments (mpad must be a power of two >= m)"); return QEMB_ERR_ARG; }
  std::vector<std::pair<uint64_t, uint64_t>> v((size_t)mpad, {~(uint64_t)0, ~(uint64_t)0});
  for (int64_t k = 0; k < m; ++k) v[(size_t)k] = {keys[2 * k], keys[2 * k + 1]};
  std::sort(v.begin(), v.end());
  for (int64_t k = 0; k < mpad; ++k) { keys[2 * k] = v[(size_t)k].first; keys[2 * k + 1] = v[(size_t)k].second; }
  return 0;
}
int dev_sci_flag_new(int64_t m, const uint64_t* cand, int64_t nA, const uint64_t* A, int64_t nB, const uint64_t* B, int32_t* flags) {
  if (m <= 0 || !cand || !flags || nA < 0 || nB < 0 || (nA > 0 && !A) || (nB > 0 && !B)) { set_error("dev_sci_flag_new: bad arguments"); return QEMB_ERR_ARG; }
  for (int64_t k = 0; k < m; ++k) {
    const uint64_t a = cand[2 * k], b = cand[2 * k + 1];
    bool keep = !(a == ~(uint64_t)0 && b == ~(uint64_t)0) && !(k > 0 && cand[2 * k - 2] == a && cand[2 * k - 1] == b);
    if (keep && nA > 0 && sci_contains(A, nA, a, b)) keep = false;
    if (keep && nB > 0 && sci_contains(B, nB, a, b)) keep = false;
    flags[k] = keep ? 1 : 0;
  }
  return 0;
}
int dev_sci_compact(int64_t m, const uint64_t* cand, const int32_t* flags, const int64_t* offsets, uint64_t* out) {
  if (m <= 0 || !cand || !flags || !offsets || !out) { set_error("dev_sci_compact: bad arguments"); return QEMB_ERR_ARG; }
  for (int64_t k = 0; k < m; ++k) if (flags[k]) { out[2 * offsets[k]] = cand[2 * k]; out[2 * offsets[k] + 1] = cand[2 * k + 1]; }
  return 0;
}
int dev_sci_merge(int64_t nA, const uint64_t* A, const double* cA, int64_t nB, const uint64_t* B, uint64_t* out, double* cout) {
  if (nA < 0 || nB < 0 || nA + nB <= 0 || (nA > 0 && !A) || (nB > 0 && !B) || !out) { set_error("dev_sci_merge: bad arguments"); return QEMB_ERR_ARG; }
  int64_t i = 0, j = 0, w = 0;
  while (i < nA || j < nB) {
    const bool fromA = j >= nB || (i < nA && sci_key_less(A[2 * i], A[2 * i + 1], B[2 * j], B[2 * j + 1]));
    const uint64_t* s = fromA ? A + 2 * i : B + 2 * j;
    out[2 * w] = s[0]; out[2 * w + 1] = s[1];
    if (cout) cout[w] = (fromA && cA) ? cA[i] : 0.0;
    ++w; if (fromA) ++i; else ++j;
  }
  return 0;
}
// row r against the runs of equal alpha, as the kernel walks them: a run whose alpha is more than two excitations away is skipped whole
template <class Visit>
static void csr_row(int64_t r, const uint64_t* keys, int64_t nseg, const int64_t* seg, Visit visit) {
  for (int64_t s = 0; s < nseg; ++s) {
    const int da = sci_popc(keys[2 * r] ^ keys[2 * seg[s]]) >> 1;
    if (da > 2) continue;
    for (int64_t k = seg[s]; k < seg[s + 1]; ++k) if (da + (sci_popc(keys[2 * r + 1] ^ keys[2 * k + 1]) >> 1) <= 2) visit(k);
  }
}
int dev_sci_csr_count(int64_t N, const uint64_t* keys, int64_t nseg, const int64_t* seg, int32_t* counts) {
  if (N <= 0 || !keys || !seg || !counts || nseg <= 0 || nseg > N) { set_error("dev_sci_csr_count: bad arguments"); return QEMB_ERR_ARG; }
  for (int64_t r = 0; r < N; ++r) { int cnt = 0; csr_row(r, keys, nseg, seg, [&](int64_t) { ++cnt; }); counts[r] = cnt; }
  return 0;
}
int dev_sci_csr_fill(int n, const double* h, const double* V, int64_t N, const uint64_t* keys, int64_t nseg, const int64_t* seg, const int64_t* rowptr, int32_t* col, double* val, double* hdiag) {
  const bool values = h && V && val && hdiag, pattern = !h && !V && !val && !hdiag;
  if (n <= 0 || n > kSciMaxOrb || N <= 0 || !(values || pattern) || !keys || !seg || !rowptr || !col || nseg <= 0 || nseg > N) { set_error("dev_sci_csr_fill: bad arguments"); return QEMB_ERR_ARG; }
  for (int64_t r = 0; r < N; ++r) {
    int64_t w = rowptr[r];
    csr_row(r, keys, nseg, seg, [&](int64_t k) {
      col[w] = (int32_t)k;
      if (values) {
        val[w] = sci_hij(n, h, V, keys[2 * r], keys[2 * r + 1], keys[2 * k], keys[2 * k + 1]);
        if (k == r) hdiag[r] = val[w];
      }
      ++w;
    });
  }
  return 0;
}
int dev_sci_spmv(int64_t N, const int64_t* rowptr, const int32_t* col, const double* val, const double* x, double* y) {
  if (N <= 0 || !rowptr || !col || !val || !x || !y) { set_error("dev_sci_spmv: bad arguments"); return QEMB_ERR_ARG; }
  for (int64_t r = 0; r < N; ++r) {
    double s = 0.0;
    for (int64_t k = rowptr[r]; k < rowptr[r + 1]; ++k) s += val[k] * x[col[k]];
    y[r] = s;
  }
  return 0;
}
int dev_sci_rdm(int n, int64_t N, const uint64_t* keys, const int64_t* rowptr, const int32_t* col, const double* c, double* dm1, double* dm2) {
  if (n <= 0 || n > kSciMaxOrb || N <= 0 || !keys || !rowptr || !col || !c || !dm1 || !dm2) { set_error("dev_sci_rdm: bad arguments"); return QEMB_ERR_ARG; }
  const int64_t n2 = (int64_t)n * n, n3 = n2 * n;
  auto at = [&](int p, int q, int r, int s) -> double& { return dm2[p * n3 + q * n2 + r * n + s]; };
  auto occupied = [](uint64_t s) { std::vector<int> v; for (int p = 0; p < 64; ++p) if ((s >> p) & 1) v.push_back(p); return v; };
  for (int64_t r = 0; r < N; ++r) for (int64_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
    const int64_t j = col[k];
    const SciExc e = sci_excitation(keys[2 * r], keys[2 * r + 1], keys[2 * j], keys[2 * j + 1]);
    const double w = (e.neg ? -1.0 : 1.0) * c[r] * c[j];
    const std::vector<int> occ[2] = {occupied(keys[2 * j]), occupied(keys[2 * j + 1])};
    if (e.degree == 0) {
      for (int s1 = 0; s1 < 2; ++s1) for (int q : occ[s1]) {
        dm1[q * n + q] += w;
        for (int s2 = 0; s2 < 2; ++s2) for (int s : occ[s2]) {
          if (s1 == s2 && q == s) continue;
          at(q, q, s, s) += w;
          if (s1 == s2) at(s, q, q, s) -= w;
        }
      }
    } else if (e.degree == 1) {
      dm1[e.i * n + e.a] += w;
      for (int s2 = 0; s2 < 2; ++s2) for (int q : occ[s2]) {
        if (s2 == e.spin1 && q == e.i) continue;
        at(e.a, e.i, q, q) += w; at(q, q, e.a, e.i) += w;
        if (s2 == e.spin1) { at(e.a, q, q, e.i) -= w; at(q, e.i, e.a, q) -= w; }
      }
    } else if (e.degree == 2) {
      at(e.a, e.i, e.b, e.j) += w; at(e.b, e.j, e.a, e.i) += w;
      if (e.spin1 == e.spin2) { at(e.a, e.j, e.b, e.i) -= w; at(e.b, e.i, e.a, e.j) -= w; }
    }
  }
  return 0;
}
// the kernel's lanes one after another, then its shuffle tree: lane l takes lane l ^ off at every step, and lane 0 holds the sum
int dev_sci_pt2_rows(int n, const double* h, const double* V, int64_t N, const uint64_t* keys, const double* c, int64_t nseg, const int64_t* seg, int64_t K, const uint64_t* ext,
                     double e_var, double eps, double dbl_bound, double* contrib) {
  if (n <= 0 || n > kSciMaxOrb || !h || !V || !keys || !c || !seg || !ext || !contrib || N <= 0 || nseg <= 0 || nseg > N || K <= 0 || !(eps > 0.0)) {
    set_error("dev_sci_pt2_rows: bad arguments"); return QEMB_ERR_ARG;
  }
  for (int64_t k = 0; k < K; ++k) {
    const uint64_t a = ext[2 * k], b = ext[2 * k + 1];
    double s[64], t[64];
    for (int lane = 0; lane < 64; ++lane) s[lane] = sci_pt2_lane(n, h, V, keys, c, nseg, (const long long*)seg, a, b, eps, dbl_bound, lane, 64);
    for (int off = 32; off > 0; off >>= 1) {
      for (int lane = 0; lane < 64; ++lane) t[lane] = s[lane] + s[lane ^ off];
      std::copy(t, t + 64, s);
    }
    contrib[k] = sci_pt2_term(s[0], e_var, sci_diag(n, h, V, a, b));
  }
  return 0;
}
// the kernel's order: 1024 strided partial sums, then its tree
int dev_sci_sum(int64_t m, const double* in, double* out) {
  if (m <= 0 || !in || !out) { set_error("dev_sci_sum: bad arguments"); return QEMB_ERR_ARG; }
  std::vector<double> s(1024, 0.0);
  for (int tid = 0; tid < 1024; ++tid) for (int64_t i = tid; i < m; i += 1024) s[(size_t)tid] += in[i];
  for (int off = 512; off > 0; off >>= 1) for (int tid = 0; tid < off; ++tid) s[(size_t)tid] += s[(size_t)(tid + off)];
  out[0] = s[0];
  return 0;
}
int dev_sci_dm2_finish(int n, int o_cum, const double* dm1, double* dm2) {
  if (n <= 0 || n > kSciMaxOrb || o_cum < 0 || o_cum > n || !dm1 || !dm2) { set_error("dev_sci_dm2_finish: bad arguments"); return QEMB_ERR_ARG; }
  int64_t idx = 0;
  for (int p = 0; p < n; ++p) for (int q = 0; q < n; ++q) for (int r = 0; r < n; ++r) for (int s = 0; s < n; ++s) dm2[idx++] -= cumulant_mean_field(n, o_cum, dm1, p, q, r, s);
  return 0;
}

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
