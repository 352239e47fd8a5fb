// cumulant_core.h -- the mean-field part of a 2-RDM, stated once for the kernels (fci_ops.hip, sci_ops.hip) and the mock's selected-CI restatement
// (sci_ops_hostcheck.cpp).  fci_ops_hostcheck.cpp keeps the literal statements of the reference as the independent form.
#pragma once

#if defined(__HIPCC__)
#define QEMB_NC_HD __host__ __device__ __forceinline__
#else
#define QEMB_NC_HD inline
#endif

namespace qemb {

// nc of molbe/solver.py:513-527 with hf = 2 I_occ over the first o_cum orbitals and del = dm1 - hf (dm1 [n][n]):
//   nc[p,q,r,s] = hf_pq hf_rs + hf_pq del_rs + del_pq hf_rs - (hf_ps hf_qr + hf_ps del_qr + del_ps hf_qr) / 2
QEMB_NC_HD double cumulant_mean_field(int n, int o_cum, const double* dm1, int p, int q, int r, int s) {
  const double hf_pq = (p == q && p < o_cum) ? 2.0 : 0.0, hf_rs = (r == s && r < o_cum) ? 2.0 : 0.0;
  const double hf_ps = (p == s && p < o_cum) ? 2.0 : 0.0, hf_qr = (q == r && q < o_cum) ? 2.0 : 0.0;
  const double d_pq = dm1[p * n + q] - hf_pq, d_rs = dm1[r * n + s] - hf_rs, d_ps = dm1[p * n + s] - hf_ps, d_qr = dm1[q * n + r] - hf_qr;
  return hf_pq * hf_rs + hf_pq * d_rs + d_pq * hf_rs - 0.5 * (hf_ps * hf_qr + hf_ps * d_qr + d_ps * hf_qr);
}

}  // namespace qemb
