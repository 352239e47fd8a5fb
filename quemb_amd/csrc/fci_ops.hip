// fci_ops.hip -- the passes of the determinant-space FCI around its one FP64 product (dev_ops.h: dev_fci_*; driver: fci.cpp).
//
// Knowles-Handy form: with D[pq][I] = sum_J <I|E_pq|J> c_J (E = E^alpha + E^beta) one application of H is
//     G = V D  (the MFMA GEMM, V[pq][rs] = (pq|rs)),      sigma_I = sum_pq k_pq D[pq][I] + 1/2 sum_pq sum_J <I|E_pq|J> G[pq][J].
// Both passes here are GATHERS: one thread owns the determinant I = (Ia, Ib) and every entry of its column of D -- no atomics, a fixed order of additions,
// the same bits on every run.  Ib is the fast thread index: the alpha links of a wave read one row of c / G contiguously (Ia, hence J, is uniform across
// the threads of a row), the beta links gather within one row of ns doubles (27 kB at n = 14: cache), D is written in runs of consecutive I per pq.
// The link table of one spin: links[l * ns + I] = (J << 9) | (pq << 1) | neg with <I|E_pq|J> = neg ? -1 : +1, nlink = nsocc (n - nsocc + 1) words per string
// (string fast: the threads of a wave read consecutive words).  Within one spin a string meets every pq at most once.
// Bytes of one application: D written (zeros, then the links) and read, G written and read: four passes over 8 n^2 N_det.
#include "hip_common.h"
#include "cumulant_core.h"

namespace qemb {
namespace {

// Both passes work on a slab of alpha rows [a0, a1) (all beta strings: the determinants a0 ns <= I < a1 ns, contiguous in c[Ia][Ib]); Ns = (a1 - a0) ns columns.
// The whole space is the slab (0, ns).
// gather: D_s[pq][I - a0 ns] for the determinants of the slab from the whole vector c.  The owner writes every entry of its column: zeros where no link lands,
// then the alpha links |Ia Ib> <- E_pq |Ja Ib>, then the beta links |Ia Ib> <- E_pq |Ia Jb> added to what this thread stored before.
__global__ void __launch_bounds__(256) fci_gather_slab_kernel(int n, long long ns, int nlink, const int* __restrict__ links, const double* __restrict__ c,
                                                              long long a0, long long a1, double* Ds) {
  const long long Ns = (a1 - a0) * ns;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;      // the column of D_s
  if (t >= Ns) return;
  const long long Ia = a0 + t / ns, Ib = t - (Ia - a0) * ns;
  const int n2 = n * n;
  for (int pq = 0; pq < n2; ++pq) Ds[(long long)pq * Ns + t] = 0.0;
  for (int l = 0; l < nlink; ++l) {
    const int w = links[(long long)l * ns + Ia];
    const double x = c[(long long)(w >> 9) * ns + Ib];
    Ds[(long long)((w >> 1) & 255) * Ns + t] = (w & 1) ? -x : x;
  }
  for (int l = 0; l < nlink; ++l) {
    const int w = links[(long long)l * ns + Ib];
    const double x = c[Ia * ns + (w >> 9)];
    double* d = Ds + (long long)((w >> 1) & 255) * Ns + t;
    *d += (w & 1) ? -x : x;
  }
}

// sigma: every determinant I of the WHOLE space takes what the slab holds for it -- the one-body term when I lies in the slab, and 1/2 G_s[pq][J - a0 ns] over
// those links (pq, J) of I whose J lies in the slab: an alpha link when a0 <= Ja < a1, a beta link (Ja = Ia) when I's own row is in range.  Still a gather: one
// thread per I, no atomics; the slab at a0 = 0 starts sigma, every later one adds to it, so ascending slabs give one fixed order of additions per slab height.
// Ib is the fast thread index: Ia, the words links[l ns + Ia] and both range tests are uniform over the threads of a row, so a wave (but for the one that straddles
// two rows) takes each branch whole, and the alpha reads of G_s stay contiguous.  Outside the slab's rows a thread reads its nlink alpha words and the few G_s rows
// they select: the link table is rescanned once per slab.
__global__ void __launch_bounds__(256) fci_sigma_slab_kernel(int n, long long ns, int nlink, const int* __restrict__ links, const double* __restrict__ k,
                                                             long long a0, long long a1, const double* __restrict__ Ds, const double* __restrict__ Gs, double* sigma) {
  const long long N = ns * ns, Ns = (a1 - a0) * ns;
  const long long I = (long long)blockIdx.x * 256 + threadIdx.x;
  if (I >= N) return;
  const long long Ia = I / ns, Ib = I - Ia * ns;
  const bool mine = Ia >= a0 && Ia < a1;
  const int n2 = n * n;
  double one = 0.0, two = 0.0;
  if (mine) {
    const long long t = I - a0 * ns;
    for (int pq = 0; pq < n2; ++pq) one += k[pq] * Ds[(long long)pq * Ns + t];
  }
  for (int l = 0; l < nlink; ++l) {
    const int w = links[(long long)l * ns + Ia];
    const long long Ja = w >> 9;
    if (Ja < a0 || Ja >= a1) continue;
    const double x = Gs[(long long)((w >> 1) & 255) * Ns + (Ja - a0) * ns + Ib];
    two += (w & 1) ? -x : x;
  }
  if (mine) {
    for (int l = 0; l < nlink; ++l) {
      const int w = links[(long long)l * ns + Ib];
      const double x = Gs[(long long)((w >> 1) & 255) * Ns + (Ia - a0) * ns + (w >> 9)];
      two += (w & 1) ? -x : x;
    }
  }
  const double add = one + 0.5 * two;
  sigma[I] = a0 == 0 ? add : sigma[I] + add;
}

// H_II from the occupations: sum_i (na_i + nb_i) h_ii + 1/2 sum_ij [(na_i na_j + nb_i nb_j)(J_ij - K_ij) + 2 na_i nb_j J_ij], J_ij = (ii|jj), K_ij = (ij|ji)
__global__ void __launch_bounds__(256) fci_diag_kernel(int n, long long ns, const int* __restrict__ strings, const double* __restrict__ h, const double* __restrict__ V,
                                                       double* __restrict__ hdiag) {
  const long long N = ns * ns;
  const long long I = (long long)blockIdx.x * 256 + threadIdx.x;
  if (I >= N) return;
  const long long Ia = I / ns, Ib = I - Ia * ns;
  const unsigned a = (unsigned)strings[Ia], b = (unsigned)strings[Ib];
  const long long n2 = (long long)n * n;
  double e = 0.0;
  for (int i = 0; i < n; ++i) {
    const int ai = (a >> i) & 1, bi = (b >> i) & 1;
    if (!(ai | bi)) continue;
    double s = (ai + bi) * h[i * n + i], t = 0.0;
    for (int j = 0; j < n; ++j) {
      const int aj = (a >> j) & 1, bj = (b >> j) & 1;
      if (!(aj | bj)) continue;
      const double Jij = V[(long long)(i * n + i) * n2 + j * n + j], Kij = V[(long long)(i * n + j) * n2 + j * n + i];
      t += (ai * aj + bi * bj) * (Jij - Kij) + (ai * bj + bi * aj) * Jij;
    }
    e += s + 0.5 * t;
  }
  hdiag[I] = e;
}

// out = r / (H_II - theta), the denominator kept away from zero (1e-8, with its sign)
__global__ void __launch_bounds__(256) fci_precond_kernel(long long N, const double* __restrict__ r, const double* __restrict__ hdiag, double theta, double* __restrict__ out) {
  const long long I = (long long)blockIdx.x * 256 + threadIdx.x;
  if (I >= N) return;
  double d = hdiag[I] - theta;
  if (fabs(d) < 1e-8) d = d < 0.0 ? -1e-8 : 1e-8;
  out[I] = r[I] / d;
}

// dm2[p,q,r,s] = A[qp][rs] - delta_qr dm1[p,s]   (A[pq][rs] = sum_I D[pq][I] D[rs][I] = <E_qp E_rs>; PySCF's dm2[p,q,r,s] = <p+ r+ s q>), every element written once;
// o_cum >= 0: minus the mean-field part nc of the reference (cumulant_core.h)
__global__ void __launch_bounds__(256) fci_dm2_kernel(int n, int o_cum, const double* __restrict__ A, const double* __restrict__ dm1, double* __restrict__ out) {
  const int n2 = n * n;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n2 * n2) return;
  const int pq = idx / n2, rs = idx - pq * n2;
  const int p = pq / n, q = pq - p * n, r = rs / n, s = rs - r * n;
  double x = A[(q * n + p) * n2 + rs];
  if (q == r) x -= dm1[p * n + s];
  if (o_cum >= 0) x -= cumulant_mean_field(n, o_cum, dm1, p, q, r, s);
  out[idx] = x;
}

inline unsigned det_grid(int64_t N) { return (unsigned)((N + 255) / 256); }

}  // namespace

int dev_fci_gather_slab(int n, int64_t ns, int nlink, const int32_t* links, const double* c, int64_t a0, int64_t a1, double* Ds) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (int rc = fci_check_args("dev_fci_gather_slab", n, ns, nlink, links, c, Ds)) return rc;
  if (int rc = fci_check_slab("dev_fci_gather_slab", ns, a0, a1)) return rc;
  return launch("dev_fci_gather_slab", fci_gather_slab_kernel, dim3(det_grid((a1 - a0) * ns)), dim3(256), 0, st, n, ns, nlink, links, c, a0, a1, Ds);
}

int dev_fci_sigma_slab(int n, int64_t ns, int nlink, const int32_t* links, const double* k, int64_t a0, int64_t a1, const double* Ds, const double* Gs, double* sigma) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (int rc = fci_check_args("dev_fci_sigma_slab", n, ns, nlink, links, Ds, sigma)) return rc;
  if (int rc = fci_check_slab("dev_fci_sigma_slab", ns, a0, a1)) return rc;
  if (!k || !Gs) { set_error("dev_fci_sigma_slab: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_fci_sigma_slab", fci_sigma_slab_kernel, dim3(det_grid(ns * ns)), dim3(256), 0, st, n, ns, nlink, links, k, a0, a1, Ds, Gs, sigma);
}

int dev_fci_diag(int n, int64_t ns, const int32_t* strings, const double* h, const double* V, double* hdiag) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (int rc = fci_check_args("dev_fci_diag", n, ns, 1, strings, h, hdiag)) return rc;
  if (!V) { set_error("dev_fci_diag: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_fci_diag", fci_diag_kernel, dim3(det_grid(ns * ns)), dim3(256), 0, st, n, ns, strings, h, V, hdiag);
}

int dev_fci_precond(int64_t N, const double* r, const double* hdiag, double theta, double* out) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (N <= 0 || N > kFciMaxDet || !r || !hdiag || !out) { set_error("dev_fci_precond: bad arguments"); return QEMB_ERR_ARG; }
  return launch("dev_fci_precond", fci_precond_kernel, dim3(det_grid(N)), dim3(256), 0, st, N, r, hdiag, theta, out);
}

int dev_fci_dm2(int n, int o_cum, const double* A, const double* dm1, double* out) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (n <= 0 || n > kFciMaxOrb || o_cum > n || !A || !dm1 || !out) { set_error("dev_fci_dm2: bad arguments"); return QEMB_ERR_ARG; }
  const int n4 = n * n * n * n;
  return launch("dev_fci_dm2", fci_dm2_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, n, o_cum, A, dm1, out);
}

}  // namespace qemb
