// sci_ops.hip -- the determinant-space passes of the selected CI on 64-bit occupation words (dev_ops.h: dev_sci_*; driver: sci.cpp; arithmetic: sci_core.h).
//
// screen     one workgroup per determinant of the slab, its lanes stride the flat list of excitations; count pass, scan, emit pass: dense output in a fixed order
//            (a key outside the alpha-word range of the call is written as the pad key of the sort: the slots stay where they are).
// scan       exclusive scan int32 -> int64 by ONE workgroup walking the array in pieces of 8192 (the arrays are counts per lane or per row: a few MB at most).
// sort       bitonic network on the 128-bit keys in global memory, one launch per (k, j) step; the set is what matters, and the network is deterministic.
// flag_new / compact / merge   binary searches in sorted lists; every output position has one owner.
// csr        one thread per row walks the runs of equal alpha: popcount of the alpha words rules out a whole run, then the betas of the run are compared.
// spmv       one wavefront per row, lanes stride the row, a fixed xor-shuffle tree.
// pt2_rows   one wavefront per determinant outside the space, lanes stride the runs of equal alpha of the space, a fixed xor-shuffle tree; sum: one workgroup, fixed order.
// rdm        one wavefront per row, one lane per stored pair: the excitation is recomputed from the two keys and its contributions are added with FP64 atomics.
// Everything but the RDM pass has one owner per output element and a fixed order of additions: the same bits on every call.
#include "hip_common.h"
#include "cumulant_core.h"
#include "sci_core.h"

namespace qemb {
namespace {

__global__ void __launch_bounds__(kSciScreenLanes) sci_screen_kernel(int n, const double* __restrict__ h, const double* __restrict__ V, const uint64_t* __restrict__ keys,
                                                                     const double* __restrict__ c, double eps, double dbl_bound, const long long* __restrict__ offsets,
                                                                     int* __restrict__ counts, uint64_t* __restrict__ out, uint64_t lo, uint64_t hi) {
  __shared__ SciLists L;
  const long long d = blockIdx.x;
  const uint64_t a = keys[2 * d], b = keys[2 * d + 1];
  if (threadIdx.x == 0) sci_lists(n, a, b, &L);
  __syncthreads();
  const long long slot = d * kSciScreenLanes + threadIdx.x;
  if (!offsets) {
    counts[slot] = sci_screen_lane(n, h, V, L, a, b, c[d], eps, dbl_bound, (int)threadIdx.x, kSciScreenLanes, [](int, uint64_t, uint64_t) {});
  } else {
    uint64_t* o = out + 4 * offsets[slot];
    sci_screen_lane(n, h, V, L, a, b, c[d], eps, dbl_bound, (int)threadIdx.x, kSciScreenLanes,
                    [o, lo, hi](int k, uint64_t na, uint64_t nb) { sci_put_in_range(o + 4 * k, na, nb, lo, hi); sci_put_in_range(o + 4 * k + 2, nb, na, lo, hi); });
  }
}

__global__ void __launch_bounds__(1024) sci_scan_kernel(long long m, const int* __restrict__ in, long long* __restrict__ out) {
  __shared__ long long s[1024];
  const int tid = threadIdx.x;
  long long carry = 0;
  for (long long base = 0; base < m; base += 8192) {
    const long long i0 = base + (long long)tid * 8;
    long long v[8], sum = 0;
    for (int k = 0; k < 8; ++k) { v[k] = i0 + k < m ? in[i0 + k] : 0; sum += v[k]; }
    s[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const long long t = tid >= off ? s[tid - off] : 0;
      __syncthreads();
      s[tid] += t;
      __syncthreads();
    }
    long long excl = s[tid] - sum + carry;
    for (int k = 0; k < 8; ++k) if (i0 + k < m) { out[i0 + k] = excl; excl += v[k]; }
    carry += s[1023];
    __syncthreads();
  }
  if (tid == 0) out[m] = carry;
}

__global__ void __launch_bounds__(256) sci_pad_kernel(long long m, long long mpad, uint64_t* keys) {
  const long long k = m + (long long)blockIdx.x * 256 + threadIdx.x;
  if (k < mpad) { keys[2 * k] = ~(uint64_t)0; keys[2 * k + 1] = ~(uint64_t)0; }
}
__global__ void __launch_bounds__(256) sci_bitonic_kernel(long long half, long long k, long long j, uint64_t* keys) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= half) return;
  const long long i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
  const uint64_t ai = keys[2 * i], bi = keys[2 * i + 1], al = keys[2 * l], bl = keys[2 * l + 1];
  const bool up = (i & k) == 0;
  if (up ? sci_key_less(al, bl, ai, bi) : sci_key_less(ai, bi, al, bl)) { keys[2 * i] = al; keys[2 * i + 1] = bl; keys[2 * l] = ai; keys[2 * l + 1] = bi; }
}

__global__ void __launch_bounds__(256) sci_flag_new_kernel(long long m, const uint64_t* __restrict__ cand, long long nA, const uint64_t* __restrict__ A, long long nB,
                                                           const uint64_t* __restrict__ B, int* __restrict__ flags) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= m) return;
  const uint64_t a = cand[2 * k], b = cand[2 * k + 1];
  bool keep = !(a == ~(uint64_t)0 && b == ~(uint64_t)0);
  if (keep && k > 0 && cand[2 * k - 2] == a && cand[2 * k - 1] == b) keep = false;
  if (keep && nA > 0 && sci_contains(A, nA, a, b)) keep = false;
  if (keep && nB > 0 && sci_contains(B, nB, a, b)) keep = false;
  flags[k] = keep ? 1 : 0;
}
__global__ void __launch_bounds__(256) sci_compact_kernel(long long m, const uint64_t* __restrict__ cand, const int* __restrict__ flags, const long long* __restrict__ offsets,
                                                          uint64_t* __restrict__ out) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= m || !flags[k]) return;
  out[2 * offsets[k]] = cand[2 * k]; out[2 * offsets[k] + 1] = cand[2 * k + 1];
}
// item k < nA: A[k] goes to k + (members of B below it); item nA + k: B[k] goes to k + (members of A below it)
__global__ void __launch_bounds__(256) sci_merge_kernel(long long nA, const uint64_t* __restrict__ A, const double* __restrict__ cA, long long nB, const uint64_t* __restrict__ B,
                                                        uint64_t* __restrict__ out, double* __restrict__ cout) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= nA + nB) return;
  const bool fromA = k < nA;
  const long long own = fromA ? k : k - nA;
  const uint64_t* src = fromA ? A : B;
  const uint64_t a = src[2 * own], b = src[2 * own + 1];
  const long long pos = own + (fromA ? sci_lower_bound(B, nB, a, b) : sci_lower_bound(A, nA, a, b));
  out[2 * pos] = a; out[2 * pos + 1] = b;
  if (cout) cout[pos] = (fromA && cA) ? cA[own] : 0.0;
}

template <bool FILL>
__global__ void __launch_bounds__(256) sci_csr_kernel(int n, const double* __restrict__ h, const double* __restrict__ V, long long N, const uint64_t* __restrict__ keys,
                                                      long long nseg, const long long* __restrict__ seg, const long long* __restrict__ rowptr, int* __restrict__ counts,
                                                      int* __restrict__ col, double* __restrict__ val, double* __restrict__ hdiag) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  const uint64_t ar = keys[2 * r], br = keys[2 * r + 1];
  long long w = FILL ? rowptr[r] : 0;
  int cnt = 0;
  for (long long s = 0; s < nseg; ++s) {
    const long long k0 = seg[s], k1 = seg[s + 1];
    const uint64_t as = keys[2 * k0];
    const int da = sci_popc(ar ^ as) >> 1;
    if (da > 2) continue;
    for (long long k = k0; k < k1; ++k) {
      const uint64_t bs = keys[2 * k + 1];
      if (da + (sci_popc(br ^ bs) >> 1) > 2) continue;
      if (FILL) {
        col[w] = (int)k;
        if (h) {      // (without integrals: the pattern alone)
          const double x = sci_hij(n, h, V, ar, br, as, bs);
          val[w] = x;
          if (k == r) hdiag[r] = x;
        }
        ++w;
      } else ++cnt;
    }
  }
  if (!FILL) counts[r] = cnt;
}

__global__ void __launch_bounds__(256) sci_spmv_kernel(long long N, const long long* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val,
                                                       const double* __restrict__ x, double* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= N) return;      // (a whole wavefront leaves together)
  double s = 0.0;
  for (long long k = rowptr[r] + lane; k < rowptr[r + 1]; k += 64) s += val[k] * x[col[k]];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) y[r] = s;
}

__global__ void __launch_bounds__(256) sci_rdm_kernel(int n, long long N, const uint64_t* __restrict__ keys, const long long* __restrict__ rowptr, const int* __restrict__ col,
                                                      const double* __restrict__ c, double* dm1, double* dm2) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= N) return;
  const long long n2 = (long long)n * n, n3 = n2 * n;
  auto add2 = [&](int p, int q, int rr, int s, double x) { atomicAdd(dm2 + p * n3 + q * n2 + rr * n + s, x); };
  const uint64_t a1 = keys[2 * r], b1 = keys[2 * r + 1];      // the bra
  const double cr = c[r];
  if (cr == 0.0) return;
  for (long long k = rowptr[r] + lane; k < rowptr[r + 1]; k += 64) {
    const long long j = col[k];
    double w = cr * c[j];
    if (w == 0.0) continue;
    const uint64_t a2 = keys[2 * j], b2 = keys[2 * j + 1];      // the ket
    const SciExc e = sci_excitation(a1, b1, a2, b2);
    if (e.neg) w = -w;
    if (e.degree == 0) {
      for (int s1 = 0; s1 < 2; ++s1) for (uint64_t x = s1 ? b2 : a2; x; x &= x - 1) {
        const int q = sci_ctz(x);
        atomicAdd(dm1 + q * n + q, w);
        for (int s2 = 0; s2 < 2; ++s2) for (uint64_t y = s2 ? b2 : a2; y; y &= y - 1) {
          const int s = sci_ctz(y);
          if (s1 == s2 && q == s) continue;
          add2(q, q, s, s, w);
          if (s1 == s2) add2(s, q, q, s, -w);
        }
      }
    } else if (e.degree == 1) {
      atomicAdd(dm1 + e.i * n + e.a, w);
      for (int s2 = 0; s2 < 2; ++s2) for (uint64_t y = s2 ? b2 : a2; y; y &= y - 1) {
        const int q = sci_ctz(y);
        if (s2 == e.spin1 && q == e.i) continue;
        add2(e.a, e.i, q, q, w); add2(q, q, e.a, e.i, w);
        if (s2 == e.spin1) { add2(e.a, q, q, e.i, -w); add2(q, e.i, e.a, q, -w); }
      }
    } else if (e.degree == 2) {
      add2(e.a, e.i, e.b, e.j, w); add2(e.b, e.j, e.a, e.i, w);
      if (e.spin1 == e.spin2) { add2(e.a, e.j, e.b, e.i, -w); add2(e.b, e.i, e.a, e.j, -w); }
    }
  }
}

// contrib[k] = S_a^2 / (e_var - H_aa) of external determinant k: one wavefront per determinant, its lanes stride the runs of equal alpha of the space
// (sci_pt2_lane), a fixed xor-shuffle tree; lane 0 forms the diagonal element and writes.  One owner and one order of additions per output.
__global__ void __launch_bounds__(256) sci_pt2_rows_kernel(int n, const double* __restrict__ h, const double* __restrict__ V, long long N, const uint64_t* __restrict__ keys,
                                                           const double* __restrict__ c, long long nseg, const long long* __restrict__ seg, long long K,
                                                           const uint64_t* __restrict__ ext, double e_var, double eps, double dbl_bound, double* __restrict__ contrib) {
  const int lane = threadIdx.x & 63;
  const long long k = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= K) return;      // (a whole wavefront leaves together)
  const uint64_t a = ext[2 * k], b = ext[2 * k + 1];
  double s = sci_pt2_lane(n, h, V, keys, c, nseg, seg, a, b, eps, dbl_bound, lane, 64);
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) contrib[k] = sci_pt2_term(s, e_var, sci_diag(n, h, V, a, b));
}
// out[0] = sum of in[0..m): ONE workgroup, every thread adds its elements tid, tid + 1024, ... in ascending order, then a fixed tree in shared memory
__global__ void __launch_bounds__(1024) sci_sum_kernel(long long m, const double* __restrict__ in, double* __restrict__ out) {
  __shared__ double s[1024];
  const int tid = threadIdx.x;
  double x = 0.0;
  for (long long i = tid; i < m; i += 1024) x += in[i];
  s[tid] = x;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if (tid < off) s[tid] += s[tid + off];
    __syncthreads();
  }
  if (tid == 0) out[0] = s[0];
}

// dm2 -= nc, the mean-field part of cumulant_core.h
__global__ void __launch_bounds__(256) sci_dm2_finish_kernel(int n, int o_cum, const double* __restrict__ dm1, double* __restrict__ dm2) {
  const long long n2 = (long long)n * n;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n2 * n2) return;
  const int pq = (int)(idx / n2), rs = (int)(idx - pq * n2);
  const int p = pq / n, q = pq - p * n, r = rs / n, s = rs - r * n;
  dm2[idx] -= cumulant_mean_field(n, o_cum, dm1, p, q, r, s);
}

inline bool grid_for(const char* who, long long items, int per_block, unsigned* grid) {
  const long long nb = (items + per_block - 1) / per_block;
  if (nb <= 0 || nb > 0x7fffffffLL) { set_error(std::string(who) + ": bad item count " + std::to_string(items)); return false; }
  *grid = (unsigned)nb;
  return true;
}
#define SCI_STREAM(st)                                                                              \
  hipStream_t st = hip_stream();                                                                    \
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }

}  // namespace

int dev_sci_screen_count(int n, const double* h, const double* V, int64_t nd, const uint64_t* keys, const double* c, double eps, double dbl_bound, int32_t* counts) {
  SCI_STREAM(st);
  unsigned grid;
  if (n <= 0 || n > kSciMaxOrb || !h || !V || !keys || !c || !counts || !(eps > 0.0) || !grid_for("dev_sci_screen_count", nd, 1, &grid)) { set_error("dev_sci_screen_count: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_sci_screen_count", sci_screen_kernel, dim3(grid), dim3(kSciScreenLanes), 0, st, n, h, V, keys, c, eps, dbl_bound, (const long long*)nullptr, counts, (uint64_t*)nullptr,
                (uint64_t)0, ~(uint64_t)0);
}
int dev_sci_screen_emit(int n, const double* h, const double* V, int64_t nd, const uint64_t* keys, const double* c, double eps, double dbl_bound, const int64_t* offsets, uint64_t* out,
                        uint64_t alpha_lo, uint64_t alpha_hi) {
  SCI_STREAM(st);
  unsigned grid;
  if (n <= 0 || n > kSciMaxOrb || !h || !V || !keys || !c || !offsets || !out || !(eps > 0.0) || !grid_for("dev_sci_screen_emit", nd, 1, &grid)) { set_error("dev_sci_screen_emit: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_sci_screen_emit", sci_screen_kernel, dim3(grid), dim3(kSciScreenLanes), 0, st, n, h, V, keys, c, eps, dbl_bound, (const long long*)offsets, (int*)nullptr, out, alpha_lo, alpha_hi);
}
int dev_sci_scan(int64_t m, const int32_t* in, int64_t* out) {
  SCI_STREAM(st);
  if (m <= 0 || !in || !out) { set_error("dev_sci_scan: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_sci_scan", sci_scan_kernel, dim3(1), dim3(1024), 0, st, (long long)m, in, (long long*)out);
}
int dev_sci_sort(int64_t m, int64_t mpad, uint64_t* keys) {
  SCI_STREAM(st);
  if (m < 0 || mpad < m || mpad < 1 || (mpad & (mpad - 1)) || !keys) { set_error("dev_sci_sort: bad arguments (mpad must be a power of two >= m)"); return QEMB_ERR_ARG; }
  unsigned grid;
  if (mpad > m) { if (!grid_for("dev_sci_sort", mpad - m, 256, &grid)) return QEMB_ERR_ARG; QTRY(launch("dev_sci_sort", sci_pad_kernel, dim3(grid), dim3(256), 0, st, (long long)m, (long long)mpad, keys)); }
  if (mpad < 2) return QEMB_OK;
  if (!grid_for("dev_sci_sort", mpad / 2, 256, &grid)) return QEMB_ERR_ARG;
  for (int64_t k = 2; k <= mpad; k <<= 1)
    for (int64_t j = k >> 1; j > 0; j >>= 1) QTRY(launch("dev_sci_sort", sci_bitonic_kernel, dim3(grid), dim3(256), 0, st, (long long)(mpad / 2), (long long)k, (long long)j, keys));
  return QEMB_OK;
}
int dev_sci_flag_new(int64_t m, const uint64_t* cand, int64_t nA, const uint64_t* A, int64_t nB, const uint64_t* B, int32_t* flags) {
  SCI_STREAM(st);
  unsigned grid;
  if (!cand || !flags || nA < 0 || nB < 0 || (nA > 0 && !A) || (nB > 0 && !B) || !grid_for("dev_sci_flag_new", m, 256, &grid)) { set_error("dev_sci_flag_new: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_sci_flag_new", sci_flag_new_kernel, dim3(grid), dim3(256), 0, st, (long long)m, cand, (long long)nA, A, (long long)nB, B, flags);
}
int dev_sci_compact(int64_t m, const uint64_t* cand, const int32_t* flags, const int64_t* offsets, uint64_t* out) {
  SCI_STREAM(st);
  unsigned grid;
  if (!cand || !flags || !offsets || !out || !grid_for("dev_sci_compact", m, 256, &grid)) { set_error("dev_sci_compact: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_sci_compact", sci_compact_kernel, dim3(grid), dim3(256), 0, st, (long long)m, cand, flags, (const long long*)offsets, out);
}
int dev_sci_merge(int64_t nA, const uint64_t* A, const double* cA, int64_t nB, const uint64_t* B, uint64_t* out, double* cout) {
  SCI_STREAM(st);
  unsigned grid;
  if (nA < 0 || nB < 0 || (nA > 0 && !A) || (nB > 0 && !B) || !out || !grid_for("dev_sci_merge", nA + nB, 256, &grid)) { set_error("dev_sci_merge: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_sci_merge", sci_merge_kernel, dim3(grid), dim3(256), 0, st, (long long)nA, A, cA, (long long)nB, B, out, cout);
}
int dev_sci_csr_count(int64_t N, const uint64_t* keys, int64_t nseg, const int64_t* seg, int32_t* counts) {
  SCI_STREAM(st);
  unsigned grid;
  if (!keys || !seg || !counts || nseg <= 0 || nseg > N || !grid_for("dev_sci_csr_count", N, 256, &grid)) { set_error("dev_sci_csr_count: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_sci_csr_count", sci_csr_kernel<false>, dim3(grid), dim3(256), 0, st, 0, (const double*)nullptr, (const double*)nullptr, (long long)N, keys, (long long)nseg,
                (const long long*)seg, (const long long*)nullptr, counts, (int*)nullptr, (double*)nullptr, (double*)nullptr);
}
int dev_sci_csr_fill(int n, const double* h, const double* V, int64_t N, const uint64_t* keys, int64_t nseg, const int64_t* seg, const int64_t* rowptr, int32_t* col, double* val, double* hdiag) {
  SCI_STREAM(st);
  unsigned grid;
  const bool values = h && V && val && hdiag, pattern = !h && !V && !val && !hdiag;
  if (n <= 0 || n > kSciMaxOrb || !(values || pattern) || !keys || !seg || !rowptr || !col || nseg <= 0 || nseg > N || !grid_for("dev_sci_csr_fill", N, 256, &grid)) {
    set_error("dev_sci_csr_fill: bad arguments"); return QEMB_ERR_ARG;
  }
  return launch("dev_sci_csr_fill", sci_csr_kernel<true>, dim3(grid), dim3(256), 0, st, n, h, V, (long long)N, keys, (long long)nseg, (const long long*)seg, (const long long*)rowptr,
                (int*)nullptr, col, val, hdiag);
}
int dev_sci_spmv(int64_t N, const int64_t* rowptr, const int32_t* col, const double* val, const double* x, double* y) {
  SCI_STREAM(st);
  unsigned grid;
  if (!rowptr || !col || !val || !x || !y || !grid_for("dev_sci_spmv", N, 4, &grid)) { set_error("dev_sci_spmv: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_sci_spmv", sci_spmv_kernel, dim3(grid), dim3(256), 0, st, (long long)N, (const long long*)rowptr, col, val, x, y);
}
int dev_sci_rdm(int n, int64_t N, const uint64_t* keys, const int64_t* rowptr, const int32_t* col, const double* c, double* dm1, double* dm2) {
  SCI_STREAM(st);
  unsigned grid;
  if (n <= 0 || n > kSciMaxOrb || !keys || !rowptr || !col || !c || !dm1 || !dm2 || !grid_for("dev_sci_rdm", N, 4, &grid)) { set_error("dev_sci_rdm: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_sci_rdm", sci_rdm_kernel, dim3(grid), dim3(256), 0, st, n, (long long)N, keys, (const long long*)rowptr, col, c, dm1, dm2);
}
int dev_sci_pt2_rows(int n, const double* h, const double* V, int64_t N, const uint64_t* keys, const double* c, int64_t nseg, const int64_t* seg, int64_t K, const uint64_t* ext,
                     double e_var, double eps, double dbl_bound, double* contrib) {
  SCI_STREAM(st);
  unsigned grid;
  if (n <= 0 || n > kSciMaxOrb || !h || !V || !keys || !c || !seg || !ext || !contrib || N <= 0 || nseg <= 0 || nseg > N || !(eps > 0.0) || !grid_for("dev_sci_pt2_rows", K, 4, &grid)) {
    set_error("dev_sci_pt2_rows: bad arguments"); return QEMB_ERR_ARG;
  }
  return launch("dev_sci_pt2_rows", sci_pt2_rows_kernel, dim3(grid), dim3(256), 0, st, n, h, V, (long long)N, keys, c, (long long)nseg, (const long long*)seg, (long long)K, ext, e_var, eps,
                dbl_bound, contrib);
}
int dev_sci_sum(int64_t m, const double* in, double* out) {
  SCI_STREAM(st);
  if (m <= 0 || !in || !out) { set_error("dev_sci_sum: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_sci_sum", sci_sum_kernel, dim3(1), dim3(1024), 0, st, (long long)m, in, out);
}
int dev_sci_dm2_finish(int n, int o_cum, const double* dm1, double* dm2) {
  SCI_STREAM(st);
  unsigned grid;
  if (n <= 0 || n > kSciMaxOrb || o_cum < 0 || o_cum > n || !dm1 || !dm2 || !grid_for("dev_sci_dm2_finish", (long long)n * n * n * n, 256, &grid)) { set_error("dev_sci_dm2_finish: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_sci_dm2_finish", sci_dm2_finish_kernel, dim3(grid), dim3(256), 0, st, n, o_cum, dm1, dm2);
}

}  // namespace qemb
