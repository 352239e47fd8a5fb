// fci.cpp -- determinant-space FCI on the device (fci.h): tables, one application of H, Davidson-Liu, RDMs.
#include "fci.h"
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <utility>

namespace qemb {

int64_t fci_string_count(int n, int nsocc) {
  if (nsocc < 0 || nsocc > n) return 0;
  int64_t c = 1;
  for (int k = 1; k <= nsocc; ++k) c = c * (n - nsocc + k) / k;
  return c;
}

int64_t fci_slab_count(int64_t ns, int64_t rows) { return rows <= 0 || rows >= ns ? 1 : (ns + rows - 1) / rows; }

int64_t fci_bytes_slab(int n, int nsocc, int max_space, int64_t rows) {
  const int64_t ns = fci_string_count(n, nsocc), N = ns * ns, n2 = (int64_t)n * n;
  const int64_t nlink = (int64_t)nsocc * (n - nsocc + 1), R = rows <= 0 || rows > ns ? ns : rows;
  return 8 * (2 * n2 * R * ns + (2 * (int64_t)max_space + 4) * N + 8 * n2 * n2) + 4 * ns * (nlink + 1);
}

int64_t fci_rows_that_fit(int n, int nsocc, int max_space, double room) {
  const int64_t ns = fci_string_count(n, nsocc);
  const double per_row = 16.0 * n * n * (double)ns, fixed = (double)fci_bytes_slab(n, nsocc, max_space, 1) - per_row;
  if (room < fixed + per_row) return 0;
  int64_t rows = (int64_t)std::min((double)ns, std::floor((room - fixed) / per_row));
  while (rows > 1 && (double)fci_bytes_slab(n, nsocc, max_space, rows) > room) --rows;      // (the division above in floating point: settle the last row exactly)
  return rows;
}

// ---- strings and link tables: host, once per (n, nsocc)
int fci_tables(int n, int nsocc, const FciTables** out) {
  static std::mutex mu;
  static std::map<std::pair<int, int>, std::unique_ptr<FciTables>> cache;
  if (n <= 0 || n > kFciMaxOrb || nsocc <= 0 || nsocc > n) { set_error("fci_tables: need 0 < nsocc <= n <= " + std::to_string(kFciMaxOrb)); return QEMB_ERR_ARG; }
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find({n, nsocc});
  if (it != cache.end()) { *out = it->second.get(); return 0; }
  std::unique_ptr<FciTables> T(new FciTables());
  T->n = n; T->nsocc = nsocc; T->nlink = nsocc * (n - nsocc + 1); T->ns = fci_string_count(n, nsocc);
  std::vector<int32_t> index((size_t)1 << n, -1);
  for (uint32_t s = 0; s < (1u << n); ++s) if (__builtin_popcount(s) == nsocc) { index[s] = (int32_t)T->strings.size(); T->strings.push_back((int32_t)s); }
  const int64_t ns = T->ns;
  T->links.assign((size_t)(T->nlink * ns), 0);
  for (int64_t I = 0; I < ns; ++I) {
    const uint32_t si = (uint32_t)T->strings[(size_t)I];
    int l = 0;
    for (int p = 0; p < n; ++p) {
      if (!((si >> p) & 1)) continue;
      for (int q = 0; q < n; ++q) {      // |I> = +- E_pq |J>: J holds q where I holds p
        if (q != p && ((si >> q) & 1)) continue;
        const uint32_t sj = (si & ~(1u << p)) | (1u << q);
        const int lo = p < q ? p : q, hi = p < q ? q : p;
        const uint32_t between = hi - lo > 1 ? (sj >> (lo + 1)) & ((1u << (hi - lo - 1)) - 1u) : 0u;
        const int neg = __builtin_popcount(between) & 1;
        T->links[(size_t)(l * ns + I)] = (index[sj] << 9) | ((p * n + q) << 1) | neg;
        ++l;
      }
    }
  }
  void* d = nullptr;
  QTRY(dev_alloc(&d, sizeof(int32_t) * (size_t)ns));
  T->strings_dev = (int32_t*)d;
  QTRY(dev_h2d(T->strings_dev, T->strings.data(), sizeof(int32_t) * (size_t)ns));
  QTRY(dev_alloc(&d, sizeof(int32_t) * T->links.size()));
  T->links_dev = (int32_t*)d;
  QTRY(dev_h2d(T->links_dev, T->links.data(), sizeof(int32_t) * T->links.size()));
  *out = T.get();
  cache[{n, nsocc}] = std::move(T);
  return 0;
}

void fci_one_body(int n, const double* h, const double* V, double* k) {
  const int64_t n2 = (int64_t)n * n;
  for (int p = 0; p < n; ++p) for (int q = 0; q < n; ++q) {
    double s = 0.0;
    for (int r = 0; r < n; ++r) s += V[(int64_t)(p * n + r) * n2 + r * n + q];
    k[p * n + q] = h[p * n + q] - 0.5 * s;
  }
}

int fci_apply(const FciTables& T, const double* k_dev, const double* V_dev, const double* c, double* D, double* G, double* sigma, int64_t rows) {
  const int64_t n2 = (int64_t)T.n * T.n, R = rows > 0 ? std::min(rows, T.ns) : T.ns;
  // slab by slab, ascending: D_s, G_s = V D_s, then every determinant takes what the slab holds for it (the links are scanned once per slab)
  for (int64_t a0 = 0; a0 < T.ns; a0 += R) {
    const int64_t a1 = std::min(T.ns, a0 + R), Ns = (a1 - a0) * T.ns;
    QTRY(dev_fci_gather_slab(T.n, T.ns, T.nlink, T.links_dev, c, a0, a1, D));
    QTRY(gemm(n2, Ns, n2, 1.0, V_dev, n2, true, D, Ns, false, 0.0, G, Ns));      // G_s = V D_s
    QTRY(dev_fci_sigma_slab(T.n, T.ns, T.nlink, T.links_dev, k_dev, a0, a1, D, G, sigma));
  }
  return 0;
}

namespace fci_detail {      // (declared in fci.h: the selected-CI iteration of sci.cpp shares them)
// eigenvalues (ascending) and eigenvectors (columns of V) of a small symmetric matrix by cyclic Jacobi; A [m][m] is overwritten
void small_eigh(int m, std::vector<double>& A, std::vector<double>& w, std::vector<double>& V) {
  V.assign((size_t)m * m, 0.0);
  for (int i = 0; i < m; ++i) V[(size_t)i * m + i] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0, dia = 0.0;
    for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) (i == j ? dia : off) += A[(size_t)i * m + j] * A[(size_t)i * m + j];
    if (off <= 1e-32 * (dia > 0.0 ? dia : 1.0)) break;
    for (int p = 0; p < m; ++p) for (int q = p + 1; q < m; ++q) {
      const double apq = A[(size_t)p * m + q];
      if (apq == 0.0) continue;
      const double th = (A[(size_t)q * m + q] - A[(size_t)p * m + p]) / (2.0 * apq);
      const double t = (th >= 0.0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
      const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
      for (int k = 0; k < m; ++k) {
        const double akp = A[(size_t)k * m + p], akq = A[(size_t)k * m + q];
        A[(size_t)k * m + p] = cs * akp - sn * akq; A[(size_t)k * m + q] = sn * akp + cs * akq;
      }
      for (int k = 0; k < m; ++k) {
        const double apk = A[(size_t)p * m + k], aqk = A[(size_t)q * m + k];
        A[(size_t)p * m + k] = cs * apk - sn * aqk; A[(size_t)q * m + k] = sn * apk + cs * aqk;
      }
      for (int k = 0; k < m; ++k) {
        const double vkp = V[(size_t)k * m + p], vkq = V[(size_t)k * m + q];
        V[(size_t)k * m + p] = cs * vkp - sn * vkq; V[(size_t)k * m + q] = sn * vkp + cs * vkq;
      }
    }
  }
  std::vector<int> order(m);
  for (int i = 0; i < m; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return A[(size_t)a * m + a] < A[(size_t)b * m + b]; });
  std::vector<double> Vs((size_t)m * m);
  w.resize(m);
  for (int j = 0; j < m; ++j) { w[j] = A[(size_t)order[j] * m + order[j]]; for (int k = 0; k < m; ++k) Vs[(size_t)k * m + j] = V[(size_t)k * m + order[j]]; }
  V.swap(Vs);
}

// host[j] = <x, ys[j]>, eight products per pass (dev_dot_many); scratch: >= 8 doubles on the device
int dots(int64_t N, const double* x, const std::vector<const double*>& ys, double* scratch, double* host) {
  const int m = (int)ys.size();
  for (int j0 = 0; j0 < m; j0 += 8) {
    const int cnt = std::min(8, m - j0);
    QTRY(dev_dot_many(N, x, cnt, ys.data() + j0, scratch));
    QTRY(dev_d2h(host + j0, scratch, sizeof(double) * cnt));
  }
  return 0;
}
// out = sum_j coef[j] xs[j] (+ out when accumulate), eight terms per pass
int combine(int64_t N, const std::vector<double>& coef, const std::vector<const double*>& xs, bool accumulate, double* out) {
  const int m = (int)xs.size();
  for (int j0 = 0; j0 < m; j0 += 8)
    QTRY(dev_lincomb(N, std::min(8, m - j0), coef.data() + j0, xs.data() + j0, (j0 == 0 && !accumulate) ? 0.0 : 1.0, out));
  return 0;
}
void symmetrise_dm1(int n, double* dm1) {
  for (int p = 0; p < n; ++p) for (int q = 0; q < p; ++q) { const double s = 0.5 * (dm1[p * n + q] + dm1[q * n + p]); dm1[p * n + q] = dm1[q * n + p] = s; }
}

// c / |c|, largest-magnitude component positive (ties: the lowest index)
static int normalise_signed(int64_t N, double* c, bool compensated) {
  std::vector<double> ch((size_t)N);
  QTRY(dev_d2h(ch.data(), c, sizeof(double) * N));
  double nrm = 0.0; int64_t big = 0;
  for (int64_t I = 0; I < N; ++I) { nrm += ch[(size_t)I] * ch[(size_t)I]; if (std::fabs(ch[(size_t)I]) > std::fabs(ch[(size_t)big])) big = I; }
  if (compensated) {
    // The plain sum above absorbs every c_I^2 below half an ulp of the running sum once the leading determinant is in: at (14, 7) that tail is 2.2e-11 of the norm,
    // at (16, 8) 1.2e-10 (measured), and Tr dm1 and the energy from the RDMs are off by as much.  The slabbed FCI solve, which is the one that reaches those sizes,
    // sums with compensation (Neumaier); the unslabbed solve and the selected CI keep the plain sum and their bits.
    double s = 0.0, comp = 0.0;
    for (int64_t I = 0; I < N; ++I) {
      const double x = ch[(size_t)I] * ch[(size_t)I], t2 = s + x;
      comp += std::fabs(s) >= x ? (s - t2) + x : (x - t2) + s;
      s = t2;
    }
    nrm = s + comp;
  }
  const double scale = (ch[(size_t)big] < 0.0 ? -1.0 : 1.0) / std::sqrt(nrm);
  if (scale != 1.0) QTRY(axpby(N, scale, c, 0.0, c));
  return 0;
}

int davidson(int64_t N, const std::function<int(const double*, double*)>& apply, const double* hdiag, double conv_tol, int max_cycle, int max_space, double lindep,
             bool compensated, double* c, FciResult* res) {
  const int ms = (int)std::min<int64_t>(max_space, N);
  *res = FciResult();
  DBuf r, t, scal;
  QTRY(r.alloc(N)); QTRY(t.alloc(N)); QTRY(scal.alloc(8));
  std::vector<DBuf> B((size_t)ms), S((size_t)ms);
  for (int j = 0; j < ms; ++j) { QTRY(B[j].alloc(N)); QTRY(S[j].alloc(N)); }
  auto ptrs = [&](const std::vector<DBuf>& X, int cnt) { std::vector<const double*> p((size_t)cnt); for (int j = 0; j < cnt; ++j) p[j] = X[j].p; return p; };
  auto norm2 = [&](const double* x, double* out) { std::vector<const double*> self(1, x); return dots(N, x, self, scal, out); };
  QTRY(dcopy(N, c, B[0]));
  QTRY(apply(B[0], S[0]));
  res->n_iter = 1;
  int m = 1;
  std::vector<double> Hs((size_t)ms * ms, 0.0), row((size_t)ms), y, w, A;
  QTRY(dots(N, S[0], ptrs(B, 1), scal, row.data()));
  Hs[0] = row[0];
  for (;;) {
    // ---- the small eigenproblem on the host: lowest Ritz pair
    A.assign((size_t)m * m, 0.0);
    for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) A[(size_t)i * m + j] = Hs[(size_t)i * ms + j];
    std::vector<double> Vv;
    small_eigh(m, A, w, Vv);
    y.assign((size_t)m, 0.0);
    for (int j = 0; j < m; ++j) y[j] = Vv[(size_t)j * m];
    const double theta = w[0];
    // ---- residual r = sum_j y_j (sigma_j - theta b_j)
    std::vector<double> cy(y), cb((size_t)m);
    for (int j = 0; j < m; ++j) cb[j] = -theta * y[j];
    QTRY(combine(N, cy, ptrs(S, m), false, r));
    QTRY(combine(N, cb, ptrs(B, m), true, r));
    double rr = 0.0;
    QTRY(norm2(r, &rr));
    res->e = theta; res->residual = std::sqrt(rr > 0.0 ? rr : 0.0);
    res->converged = res->residual <= conv_tol;
    bool stop = res->converged || res->n_iter >= max_cycle;
    if (!stop) {
      if (m == ms) {      // collapse to the current Ritz vector and its image (t serves twice: no further vector)
        QTRY(combine(N, y, ptrs(B, m), false, t));
        QTRY(dcopy(N, t, B[0]));
        QTRY(combine(N, y, ptrs(S, m), false, t));
        QTRY(dcopy(N, t, S[0]));
        m = 1; Hs[0] = theta; y.assign(1, 1.0);
      }
      // ---- correction: (H_II - theta)^-1 r, orthogonalised twice against the basis
      QTRY(dev_fci_precond(N, r, hdiag, theta, t));
      for (int pass = 0; pass < 2; ++pass) {
        QTRY(dots(N, t, ptrs(B, m), scal, row.data()));
        std::vector<double> neg((size_t)m);
        for (int j = 0; j < m; ++j) neg[j] = -row[j];
        QTRY(combine(N, neg, ptrs(B, m), true, t));
      }
      double tt = 0.0;
      QTRY(norm2(t, &tt));
      const double tn = std::sqrt(tt > 0.0 ? tt : 0.0);
      if (!(tn > lindep) || m == ms) stop = true;      // nothing left to add: the space is exhausted (m == ms after the collapse: the space itself has one dimension)
      else {
        QTRY(axpby(N, 1.0 / tn, t, 0.0, B[m]));
        QTRY(apply(B[m], S[m]));
        res->n_iter += 1;
        QTRY(dots(N, S[m], ptrs(B, m + 1), scal, row.data()));
        for (int j = 0; j <= m; ++j) Hs[(size_t)m * ms + j] = Hs[(size_t)j * ms + m] = row[j];
        ++m;
        continue;
      }
    }
    QTRY(combine(N, y, ptrs(B, m), false, c));      // the Ritz vector
    return normalise_signed(N, c, compensated);
  }
}
}  // namespace fci_detail
using namespace fci_detail;

int fci_davidson(const FciTables& T, const double* h_host, const double* V_dev, const FciOptions& opt, double* c, FciResult* res, int64_t rows) {
  const int n = T.n;
  const int64_t n2 = (int64_t)n * n, N = T.ndet();
  if (opt.max_space < 2 || opt.max_cycle < 1 || !(opt.conv_tol > 0.0) || !(opt.lindep >= 0.0)) {
    set_error("fci: need max_space >= 2, max_cycle >= 1, conv_tol > 0 and lindep >= 0"); return QEMB_ERR_ARG;
  }
  // ---- k, the diagonal and the start vector (the unit vector at the lowest diagonal; ties: the lowest index)
  std::vector<double> Vh((size_t)(n2 * n2)), kh((size_t)n2);
  QTRY(dev_d2h(Vh.data(), V_dev, sizeof(double) * n2 * n2));
  fci_one_body(n, h_host, Vh.data(), kh.data());
  DBuf kd, hd, hdiag, D, G;
  QTRY(kd.alloc(n2)); QTRY(hd.alloc(n2)); QTRY(hdiag.alloc(N));
  const int64_t ncol = (rows > 0 ? std::min(rows, T.ns) : T.ns) * T.ns;      // columns of D and G: one slab of alpha rows, or the whole space
  QTRY(D.alloc(n2 * ncol)); QTRY(G.alloc(n2 * ncol));
  QTRY(dev_h2d(kd, kh.data(), sizeof(double) * n2));
  QTRY(dev_h2d(hd, h_host, sizeof(double) * n2));
  QTRY(dev_fci_diag(n, T.ns, T.strings_dev, hd, V_dev, hdiag));
  int64_t start = 0;
  {
    std::vector<double> dh((size_t)N);
    QTRY(dev_d2h(dh.data(), hdiag, sizeof(double) * N));
    for (int64_t I = 1; I < N; ++I) if (dh[(size_t)I] < dh[(size_t)start]) start = I;
  }
  QTRY(dev_fill(c, N, 0.0));
  const double one = 1.0;
  QTRY(dev_h2d(c + start, &one, sizeof(double)));
  auto apply = [&](const double* x, double* y) { return fci_apply(T, kd, V_dev, x, D, G, y, rows); };
  return davidson(N, apply, hdiag, opt.conv_tol, opt.max_cycle, opt.max_space, opt.lindep, rows > 0, c, res);
}

int fci_rdm12(const FciTables& T, const double* c, int o_cum, double* dm1_host, double* dm2_dev, int64_t rows) {
  const int n = T.n;
  const int64_t n2 = (int64_t)n * n, R = rows > 0 ? std::min(rows, T.ns) : T.ns;
  DBuf D, d1, A;
  QTRY(D.alloc(n2 * R * T.ns)); QTRY(d1.alloc(n2));
  if (dm2_dev) QTRY(A.alloc(n2 * n2));
  for (int64_t a0 = 0; a0 < T.ns; a0 += R) {      // slab by slab: dm1 += D_s c_s and A += D_s D_s^T (the products accumulate, beta = 1 after the first slab)
    const int64_t a1 = std::min(T.ns, a0 + R), Ns = (a1 - a0) * T.ns;
    const double beta = a0 == 0 ? 0.0 : 1.0;
    QTRY(dev_fci_gather_slab(n, T.ns, T.nlink, T.links_dev, c, a0, a1, D));
    QTRY(dev_gemv_rows(n2, Ns, D, Ns, c + a0 * T.ns, d1, 1.0, beta));
    if (dm2_dev) QTRY(gemm(n2, n2, Ns, 1.0, D, Ns, true, D, Ns, true, beta, A, n2));      // A[pq][rs] = sum_I D[pq][I] D[rs][I]
  }
  QTRY(dev_d2h(dm1_host, d1, sizeof(double) * n2));
  symmetrise_dm1(n, dm1_host);
  if (!dm2_dev) return 0;
  QTRY(dev_h2d(d1, dm1_host, sizeof(double) * n2));
  QTRY(dev_fci_dm2(n, o_cum, A, d1, dm2_dev));
  return dev_sync();      // (D, A and d1 go back to the pool on return)
}

}  // namespace qemb
