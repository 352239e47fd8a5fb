// loc_ops.hip -- orbital localisation as joint diagonalisation by Jacobi sweeps (arithmetic, the angle rule and the limits of the two variants: loc_core.h, shared
// with the scalar restatement loc_ops_hostcheck.cpp):
//   loc_lds_kernel     ONE workgroup, the stack and U in LDS, every sweep of the solve in one launch
//   loc_sums_kernel    f = sum_k sum_i (Q^k_ii)^2 and ||Q||^2 per slab of kSlab matrices (the host adds the slabs in order)
//   loc_pair_sums_kernel / loc_rotate_kernel   one round of the launch-per-round variant: the slab's partial sums of every pair, then the angles (every workgroup
//                      adds the partials of all slabs in the same order) and the rotation of the slab's matrices, rows and then columns, U as matrix K
// No atomics and no waiting between workgroups: each output element has one writer and every sum one fixed order.
#include <vector>
#include "hip_common.h"
#include "loc_core.h"

namespace qemb {
using namespace loc;

namespace {

constexpr int kLdsPairs = (kLdsMaxM + 1) / 2;

__global__ void __launch_bounds__(kThreads) loc_lds_kernel(const int K, const int m, double* __restrict__ Qg, double* __restrict__ Ug, const double stop_angle,
                                                           const int max_sweeps, double* __restrict__ out4) {
  extern __shared__ double loc_dyn[];                 // Q [K][m][m], then U [m][m]: matrix K of the stack
  __shared__ double scratch[kLdsParts * kLdsPairs * 3];      // the partial sums of a round's pairs; 2 x kThreads doubles of the f / norm reduction
  __shared__ double cs[kLdsPairs][2];
  __shared__ double th[kLdsPairs];
  __shared__ int pq[kLdsPairs][2];
  __shared__ double scal[3];                           // ||Q||^2, f, the sweep's largest |theta|
  static_assert(2 * kThreads <= kLdsParts * kLdsPairs * 3 && kLdsParts * kLdsPairs <= kThreads, "loc_lds_kernel: scratch");
  const int t = threadIdx.x;
  const int mm = m * m, np = (m + 1) & ~1, npairs = np / 2;
  double* Q = loc_dyn;
  double* U = loc_dyn + (size_t)K * mm;
  for (int e = t; e < K * mm; e += kThreads) Q[e] = Qg[e];
  for (int e = t; e < mm; e += kThreads) U[e] = (e / m == e % m) ? 1.0 : 0.0;
  __syncthreads();
  // f and ||Q||^2: thread t adds the matrices t, t + 256, ..., thread 0 the 256 partials in order
  auto sums = [&]() {
    double a = 0.0, b = 0.0;
    for (int k = t; k < K; k += kThreads) matrix_sums(Q + (size_t)k * mm, m, a, b);
    scratch[2 * t] = a; scratch[2 * t + 1] = b;
    __syncthreads();
    if (t == 0) {
      double f = 0.0, n2 = 0.0;
      for (int i = 0; i < kThreads; ++i) { f += scratch[2 * i]; n2 += scratch[2 * i + 1]; }
      scal[0] = n2; scal[1] = f;
    }
    __syncthreads();
  };
  sums();
  const double norm2 = scal[0];
  int sweeps = 0, converged = 0;
  while (sweeps < max_sweeps) {
    if (t == 0) scal[2] = 0.0;
    for (int r = 0; r < np - 1; ++r) {
      if (t < npairs * kLdsParts) {
        const int j = t / kLdsParts, s = t % kLdsParts;
        int p, q;
        rr_pair(np, r, j, p, q);
        double saa = 0.0, sdd = 0.0, sad = 0.0;
        if (q < m)
          for (int k = s; k < K; k += kLdsParts) pair_terms(Q + (size_t)k * mm, m, p, q, saa, sdd, sad);
        double* w = scratch + (s * kLdsPairs + j) * 3;
        w[0] = saa; w[1] = sdd; w[2] = sad;
      }
      __syncthreads();
      if (t < npairs) {
        int p, q;
        rr_pair(np, r, t, p, q);
        double theta = 0.0;
        if (q < m) {
          double saa = 0.0, sdd = 0.0, sad = 0.0;
          for (int s = 0; s < kLdsParts; ++s) {
            const double* w = scratch + (s * kLdsPairs + t) * 3;
            saa += w[0]; sdd += w[1]; sad += w[2];
          }
          theta = pair_angle(saa, sdd, sad, norm2);
        }
        pq[t][0] = p; pq[t][1] = q;
        cs[t][0] = cos(theta); cs[t][1] = sin(theta);
        th[t] = fabs(theta);
      }
      __syncthreads();
      if (t == 0)
        for (int j = 0; j < npairs; ++j)
          if (!(th[j] <= scal[2])) scal[2] = th[j];
      for (int it = t; it < K * npairs * m; it += kThreads) {
        const int x = it % m, j = (it / m) % npairs, k = it / (m * npairs);
        if (pq[j][1] < m && cs[j][1] != 0.0) rotate_rows(Q + (size_t)k * mm, m, pq[j][0], pq[j][1], x, cs[j][0], cs[j][1]);
      }
      __syncthreads();
      for (int it = t; it < (K + 1) * npairs * m; it += kThreads) {
        const int j = it % npairs, x = (it / npairs) % m, k = it / (m * npairs);
        if (pq[j][1] < m && cs[j][1] != 0.0) rotate_cols(Q + (size_t)k * mm, m, pq[j][0], pq[j][1], x, cs[j][0], cs[j][1]);
      }
      __syncthreads();
    }
    ++sweeps;
    if (scal[2] < stop_angle) { converged = 1; break; }      // the same value in every thread: the whole workgroup leaves together
    __syncthreads();                                        // thread 0 resets scal[2] at the top
  }
  sums();
  for (int e = t; e < K * mm; e += kThreads) Qg[e] = Q[e];
  for (int e = t; e < mm; e += kThreads) Ug[e] = U[e];
  if (t == 0) { out4[0] = (double)sweeps; out4[1] = scal[1]; out4[2] = (double)converged; out4[3] = norm2; }
}

__global__ void __launch_bounds__(kThreads) loc_identity_kernel(const int m, double* __restrict__ U) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < (long long)m * m) U[e] = (e / m == e % m) ? 1.0 : 0.0;
}

// slab b, matrix by matrix: thread t adds the rows t, t + 256, .. of the matrix, thread 0 the 256 partials in order and the slab's matrices in order
__global__ void __launch_bounds__(kThreads) loc_sums_kernel(const int K, const int m, const double* __restrict__ Q, double* __restrict__ out) {
  __shared__ double ps[kThreads], pn[kThreads];
  const int t = threadIdx.x;
  double f = 0.0, n2 = 0.0;
  for (int kk = 0; kk < kSlab; ++kk) {
    const long long k = (long long)blockIdx.x * kSlab + kk;
    if (k >= K) break;      // the same for every thread
    double a = 0.0, b = 0.0;
    matrix_sums_rows(Q + k * m * m, m, t, kThreads, a, b);
    ps[t] = a; pn[t] = b;
    __syncthreads();
    if (t == 0) {
      double fa = 0.0, na = 0.0;
      for (int i = 0; i < kThreads; ++i) { fa += ps[i]; na += pn[i]; }
      f += fa; n2 += na;
    }
    __syncthreads();
  }
  if (t == 0) { out[2 * blockIdx.x] = f; out[2 * blockIdx.x + 1] = n2; }
}

__global__ void __launch_bounds__(kThreads) loc_pair_sums_kernel(const int K, const int m, const double* __restrict__ Q, const int round, double* __restrict__ partials) {
  const int np = (m + 1) & ~1, npairs = np / 2;
  const long long k0 = (long long)blockIdx.x * kSlab, k1 = k0 + kSlab < K ? k0 + kSlab : K;
  for (int j = threadIdx.x; j < npairs; j += kThreads) {
    int p, q;
    rr_pair(np, round, j, p, q);
    double saa = 0.0, sdd = 0.0, sad = 0.0;
    if (q < m)
      for (long long k = k0; k < k1; ++k) pair_terms(Q + k * m * m, m, p, q, saa, sdd, sad);
    double* w = partials + ((long long)blockIdx.x * npairs + j) * 3;
    w[0] = saa; w[1] = sdd; w[2] = sad;
  }
}

// grid: the slabs of the K + 1 matrices (U is matrix K).  Block 0 also keeps the sweep's largest |theta| (its only writer; the launches of a sweep follow one another).
__global__ void __launch_bounds__(kThreads) loc_rotate_kernel(const int K, const int m, double* __restrict__ Q, double* __restrict__ U, const int round, const int nslab_k,
                                                              const double* __restrict__ partials, const double norm2, double* __restrict__ thmax) {
  __shared__ double cs[kMaxM / 2][2];
  __shared__ short pq[kMaxM / 2][2];
  __shared__ double red[kThreads];
  const int t = threadIdx.x;
  const int np = (m + 1) & ~1, npairs = np / 2;
  double mine = 0.0;
  for (int j = t; j < npairs; j += kThreads) {
    int p, q;
    rr_pair(np, round, j, p, q);
    double theta = 0.0;
    if (q < m) {
      double saa = 0.0, sdd = 0.0, sad = 0.0;
      for (int b = 0; b < nslab_k; ++b) {
        const double* w = partials + ((long long)b * npairs + j) * 3;
        saa += w[0]; sdd += w[1]; sad += w[2];
      }
      theta = pair_angle(saa, sdd, sad, norm2);
    }
    pq[j][0] = (short)p; pq[j][1] = (short)q;
    cs[j][0] = cos(theta); cs[j][1] = sin(theta);
    if (!(fabs(theta) <= mine)) mine = fabs(theta);
  }
  red[t] = mine;
  __syncthreads();
  if (blockIdx.x == 0 && t == 0) {
    double v = thmax[0];
    for (int i = 0; i < kThreads; ++i)
      if (!(red[i] <= v)) v = red[i];
    thmax[0] = v;
  }
  const long long k0 = (long long)blockIdx.x * kSlab, k1 = k0 + kSlab < K + 1 ? k0 + kSlab : K + 1;
  const long long kq = k1 < K ? k1 : K;      // the rows pass leaves U alone
  const long long per = (long long)npairs * m;
  for (long long it = t; it < (kq - k0) * per; it += kThreads) {
    const int x = (int)(it % m), j = (int)((it / m) % npairs);
    const long long k = k0 + it / per;
    if (pq[j][1] < m && cs[j][1] != 0.0) rotate_rows(Q + k * m * m, m, pq[j][0], pq[j][1], x, cs[j][0], cs[j][1]);
  }
  __syncthreads();
  for (long long it = t; it < (k1 - k0) * per; it += kThreads) {
    const int j = (int)(it % npairs), x = (int)((it / npairs) % m);
    const long long k = k0 + it / per;
    double* M = k < K ? Q + k * m * m : U;
    if (pq[j][1] < m && cs[j][1] != 0.0) rotate_cols(M, m, pq[j][0], pq[j][1], x, cs[j][0], cs[j][1]);
  }
}

#define LOC_STREAM(st)                                                                                 \
  hipStream_t st = hip_stream();                                                                       \
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }

struct Work {
  double* p = nullptr;
  ~Work() { if (p) dev_free(p); }
};

int read_sums(hipStream_t st, int K, int m, const double* Q, double* slab_sums, int64_t nsl, double* f, double* n2) {
  QTRY(launch("dev_joint_diag", loc_sums_kernel, dim3((unsigned)nsl), dim3(kThreads), 0, st, K, m, Q, slab_sums));
  std::vector<double> h(2 * (size_t)nsl);
  QTRY(dev_d2h(h.data(), slab_sums, sizeof(double) * h.size()));
  *f = 0.0; *n2 = 0.0;
  for (int64_t b = 0; b < nsl; ++b) { *f += h[2 * b]; *n2 += h[2 * b + 1]; }
  return QEMB_OK;
}

}  // namespace

int dev_joint_diag(int64_t K64, int64_t m64, double* Q, double* U, double stop_angle, int max_sweeps, int* sweeps_out, double* f_out, int* converged_out) {
  LOC_STREAM(st);
  if (int rc = check_joint_diag("dev_joint_diag", K64, m64, Q != nullptr, U != nullptr, stop_angle, max_sweeps)) return rc;
  const int K = (int)K64, m = (int)m64;
  int sweeps = 0, converged = 1;
  double f = 0.0;
  Work w;
  void* wp = nullptr;
  QTRY(dev_alloc(&wp, sizeof(double) * (size_t)work_doubles(K, m)));
  w.p = (double*)wp;
  if (m > 0) QTRY(launch("dev_joint_diag", loc_identity_kernel, dim3((unsigned)(((long long)m * m + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, m, U));
  if (K == 0 || m == 0) {
    QTRY(dev_sync());
  } else if (m == 1 || max_sweeps == 0) {
    double n2;
    Work s;
    QTRY(dev_alloc(&wp, sizeof(double) * 2 * (size_t)slabs(K)));
    s.p = (double*)wp;
    QTRY(read_sums(st, K, m, Q, s.p, slabs(K), &f, &n2));
    converged = m == 1;
  } else if (in_lds(K, m)) {
    const size_t lds = sizeof(double) * (size_t)(K + 1) * m * m;
    QTRY(launch("dev_joint_diag", loc_lds_kernel, dim3(1), dim3(kThreads), lds, st, K, m, Q, U, stop_angle, max_sweeps, w.p));
    double h[4];
    QTRY(dev_d2h(h, w.p, sizeof h));
    sweeps = (int)h[0]; f = h[1]; converged = (int)h[2];
  } else {
    const int npairs = (m + 1) / 2;
    const int64_t nsl = slabs(K);
    double* partials = w.p;
    double* thmax = w.p + 3 * nsl * npairs;
    double* slab_sums = thmax + 1;
    double n2 = 0.0;
    QTRY(read_sums(st, K, m, Q, slab_sums, nsl, &f, &n2));
    converged = 0;
    const int np = (m + 1) & ~1;
    while (sweeps < max_sweeps) {
      QTRY(dev_fill(thmax, 1, 0.0));
      for (int r = 0; r < np - 1; ++r) {
        QTRY(launch("dev_joint_diag", loc_pair_sums_kernel, dim3((unsigned)nsl), dim3(kThreads), 0, st, K, m, Q, r, partials));
        QTRY(launch("dev_joint_diag", loc_rotate_kernel, dim3((unsigned)slabs((int64_t)K + 1)), dim3(kThreads), 0, st, K, m, Q, U, r, (int)nsl, partials, n2, thmax));
      }
      double th = 0.0;
      QTRY(dev_d2h(&th, thmax, sizeof th));
      ++sweeps;
      if (th < stop_angle) { converged = 1; break; }
    }
    QTRY(read_sums(st, K, m, Q, slab_sums, nsl, &f, &n2));
  }
  if (!std::isfinite(f)) { set_error("dev_joint_diag: the stack holds a NaN or an infinity"); return QEMB_ERR_NUMERIC; }
  if (sweeps_out) *sweeps_out = sweeps;
  if (f_out) *f_out = f;
  if (converged_out) *converged_out = converged;
  return QEMB_OK;
}

}  // namespace qemb
