// kdf.h -- k-point density-fitted fragment ERIs of the periodic driver (quemb_amd/kbe_eri_kpoint.py; what kbe/pbe.py:529-565 asks libdmet for with
// int_transform = "out-core-DF").  The k-point GDF tensor -- one complex block L^{ki,kj}[P,mu,nu] = (P | mu_ki* nu_kj) per k-point pair -- stays resident; a fragment
// with embedding orbitals C^k = TA_k receives a REAL 3-index factor of its own with N_k naux rows:
//     M^q[P,pq]  = sum_ki (C^ki)^H L^{ki,ki+q}[P] C^{ki+q}                       q = kj - ki, one class per k-point of a mesh that closes
//     (pq|rs)    = N_k^-3 sum_q sum_P Re( M^q[P,pq] conj(M^q[P,rs]) )
//     factor rows: N_k^-3/2 Re M^q for q = -q;  (2 N_k^-3)^1/2 Re M^q and (2 N_k^-3)^1/2 Im M^q for ONE class of every pair (q, -q)
// Nothing of size N_k^3 exists: the supercell route holds N_k naux x (N_k nao)^2 doubles, this one the N_k (N_k + n_self) / 2 pair blocks of the kept classes.
#pragma once
#include <cstdint>
#include <vector>
#include "dev_ops.h"
#include "tensor_utils.h"

namespace qemb {

class Fragment;

class KdfContext {
 public:
  int nk = 0, naux = 0, nao = 0;
  // qclass[ki * nk + kj]: the class of kj - ki (0 <= class < nk, every row and column a permutation);  qconj[q]: the class of -q
  int create(int nk_, int naux_, int nao_, const int* qclass_, const int* qconj_);
  bool kept(int q) const { return q <= qconj_[q]; }            // of a pair (q, -q) the class with the smaller number is computed
  int n_kept() const;
  // L: naux x nao x nao interleaved complex128 (host).  A pair of a class that is not kept is accepted and not stored.
  int set_pair(int ki, int kj, const double* L_host);
  // TA_k: nk x nao x n interleaved complex128 (host).  factor_only: the fragment lives on the factor (Fragment::adopt_df_only), else it receives the 4-fold block
  // (the pair product of the factor) and the factor beside it.  out_s4_host (nullable): the block on the host.
  int transform(const double* TA_host, int n, double* out_s4_host, Fragment* frag, int factor_only);
  // bytes: the resident pair blocks with the staging block of an upload / the work space of one transform (with_block: the n^4 / 4 block is formed too)
  static int64_t resident_bytes(int nk, int naux, int nao, int n_kept);
  static int64_t work_bytes(int nk, int naux, int nao, int n, int n_kept, bool with_block);
  // need <= min(free device memory, limit_bytes) (limit_bytes < 0: the free memory alone), else QEMB_ERR_ALLOC with nk, naux, nao in the message; allocates nothing
  static int guard(int nk, int naux, int nao, int64_t resident, int64_t work, int64_t limit_bytes);

 private:
  std::vector<int> qclass_, qconj_, partner_;      // partner_[q * nk + ki] = the kj with qclass[ki, kj] == q
  std::vector<DBuf> pair_;                          // [ki * nk + kj]: [naux * nao][re (ld) | im (ld)]
};

}  // namespace qemb
