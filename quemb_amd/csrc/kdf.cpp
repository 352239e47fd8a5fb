// kdf.cpp -- k-point density-fitted fragment ERIs (see kdf.h; derivation and cost table in DESIGN.md section 4).
#include "kdf.h"
#include <cmath>
#include <cstdio>
#include "ao2mo.h"
#include "fragment.h"

namespace qemb {

static inline int64_t npair(int64_t n) { return n * (n + 1) / 2; }

int KdfContext::n_kept() const {
  int c = 0;
  for (int q = 0; q < nk; ++q) c += kept(q) ? 1 : 0;
  return c;
}

int64_t KdfContext::resident_bytes(int nk, int naux, int nao, int n_kept) {
  const int64_t blk = (int64_t)naux * nao * 2 * kdf_ld(nao);
  return 8 * ((int64_t)n_kept * nk * blk + (int64_t)naux * nao * nao * 2);      // the pair blocks + the interleaved block of one upload
}

int64_t KdfContext::work_bytes(int nk, int naux, int nao, int n, int n_kept, bool with_block) {
  const int64_t ld = kdf_ld(nao), np = npair(n);
  int64_t d = (int64_t)nk * nao * n * 2;                      // TA_k
  d += (int64_t)nk * (4 * ld * n + 4 * (int64_t)nao * n);     // stacked operands
  d += (int64_t)naux * nao * 2 * n;                           // first quarter
  d += (int64_t)naux * 2 * n * n;                             // M^q
  d += (int64_t)nk * naux * np;                               // the factor
  d += dev_kdf_partial_count(naux, n) + 2 * (int64_t)n_kept;
  if (with_block) d += np * np;
  return 8 * d;
}

int KdfContext::guard(int nk, int naux, int nao, int64_t resident, int64_t work, int64_t limit_bytes) {
  size_t free_b = 0, total_b = 0;
  QTRY(dev_mem_info(&free_b, &total_b));
  double room = (double)free_b;
  if (limit_bytes >= 0 && (double)limit_bytes < room) room = (double)limit_bytes;
  if ((double)resident + (double)work > room) {
    set_error("k-point DF: with nk = " + std::to_string(nk) + ", naux = " + std::to_string(naux) + ", nao = " + std::to_string(nao) + " the resident pair blocks take " +
              std::to_string((double)resident * 1e-9) + " GB and the work space of a fragment " + std::to_string((double)work * 1e-9) + " GB, more than the " +
              std::to_string(room * 1e-9) + " GB of device memory they may take");
    return QEMB_ERR_ALLOC;
  }
  return QEMB_OK;
}

int KdfContext::create(int nk_, int naux_, int nao_, const int* qc, const int* qj) {
  if (nk_ <= 0 || naux_ <= 0 || nao_ <= 0 || !qc || !qj) { set_error("qemb_kdf_create: bad arguments"); return QEMB_ERR_ARG; }
  nk = nk_; naux = naux_; nao = nao_;
  qclass_.assign(qc, qc + (size_t)nk * nk); qconj_.assign(qj, qj + nk);
  partner_.assign((size_t)nk * nk, -1);
  for (int q = 0; q < nk; ++q)
    if (qconj_[q] < 0 || qconj_[q] >= nk || qj[qconj_[q]] != q) { set_error("qemb_kdf_create: qconj is not an involution of the " + std::to_string(nk) + " classes"); return QEMB_ERR_ARG; }
  for (int ki = 0; ki < nk; ++ki) for (int kj = 0; kj < nk; ++kj) {
    const int q = qclass_[(size_t)ki * nk + kj];
    if (q < 0 || q >= nk || partner_[(size_t)q * nk + ki] >= 0) {
      set_error("qemb_kdf_create: the mesh does not close: the classes of kj - ki for ki = " + std::to_string(ki) + " are not a permutation of the k-points");
      return QEMB_ERR_ARG;
    }
    partner_[(size_t)q * nk + ki] = kj;
  }
  for (int ki = 0; ki < nk; ++ki) for (int kj = 0; kj < nk; ++kj)
    if (qclass_[(size_t)kj * nk + ki] != qconj_[qclass_[(size_t)ki * nk + kj]]) { set_error("qemb_kdf_create: qclass[kj,ki] is not the conjugate class of qclass[ki,kj]"); return QEMB_ERR_ARG; }
  QTRY(guard(nk, naux, nao, resident_bytes(nk, naux, nao, n_kept()), 0, -1));
  pair_.clear(); pair_.resize((size_t)nk * nk);
  return QEMB_OK;
}

int KdfContext::set_pair(int ki, int kj, const double* L) {
  if (ki < 0 || ki >= nk || kj < 0 || kj >= nk || !L) { set_error("qemb_kdf_set_pair: bad arguments (ki = " + std::to_string(ki) + ", kj = " + std::to_string(kj) + ")"); return QEMB_ERR_ARG; }
  if (!kept(qclass_[(size_t)ki * nk + kj])) return QEMB_OK;      // the -q partner of a kept class: M^-q = conj(M^q), nothing of it is read
  const int64_t rows = (int64_t)naux * nao;
  DBuf z;
  QTRY(z.alloc(rows * nao * 2));
  QTRY(dev_h2d(z, L, sizeof(double) * rows * nao * 2));
  DBuf& blk = pair_[(size_t)ki * nk + kj];
  QTRY(blk.alloc(rows * 2 * kdf_ld(nao)));
  int rc = dev_kdf_split(rows, nao, z, blk);
  if (rc == 0) rc = dev_sync();      // z is released on return
  if (rc) blk.release();
  return rc;
}

int KdfContext::transform(const double* TA, int n, double* out_host, Fragment* frag, int factor_only) {
  if (nk <= 0) { set_error("qemb_kdf_transform: no context"); return QEMB_ERR_ARG; }
  if (!TA || n <= 0) { set_error("qemb_kdf_transform: bad arguments"); return QEMB_ERR_ARG; }
  if (!frag && (factor_only || !out_host)) { set_error("qemb_kdf_transform: nowhere to put the result (factor_only needs a fragment handle)"); return QEMB_ERR_ARG; }
  if (frag && frag->n() != n) { set_error("fragment handle has a different n"); return QEMB_ERR_ARG; }
  for (int q = 0; q < nk; ++q) {
    if (!kept(q)) continue;
    for (int ki = 0; ki < nk; ++ki) {
      const int kj = partner_[(size_t)q * nk + ki];
      if (!pair_[(size_t)ki * nk + kj].p) {
        set_error("qemb_kdf_transform: the pair block (ki = " + std::to_string(ki) + ", kj = " + std::to_string(kj) + ") of class " + std::to_string(q) + " has not been set");
        return QEMB_ERR_ARG;
      }
    }
  }
  const bool with_block = !factor_only || out_host;
  const int nkept = n_kept();
  QTRY(guard(nk, naux, nao, 0, work_bytes(nk, naux, nao, n, nkept, with_block), -1));
  const int64_t ld = kdf_ld(nao), np = npair(n), nrows = (int64_t)nk * naux;
  const int64_t csz = 4 * ld * n, dsz = 4 * (int64_t)nao * n;
  DBuf ta, Cs, Dk, X, Macc, F, part, scal;
  QTRY(ta.alloc((int64_t)nk * nao * n * 2)); QTRY(Cs.alloc(nk * csz)); QTRY(Dk.alloc(nk * dsz));
  QTRY(X.alloc((int64_t)naux * nao * 2 * n)); QTRY(Macc.alloc((int64_t)naux * 2 * n * n)); QTRY(F.alloc(nrows * np));
  QTRY(part.alloc(dev_kdf_partial_count(naux, n))); QTRY(scal.alloc(2 * (int64_t)nkept));
  QTRY(dev_h2d(ta, TA, sizeof(double) * nk * nao * n * 2));
  QTRY(dev_kdf_stack(nk, nao, n, ta, Cs, Dk));
  const double c = 1.0 / ((double)nk * (double)nk * (double)nk);
  int64_t row0 = 0;
  int iq = 0;
  for (int q = 0; q < nk; ++q) {
    if (!kept(q)) continue;
    const int paired = qconj_[q] != q;
    for (int ki = 0; ki < nk; ++ki) {      // the sum over ki in a fixed order: beta = 1 on the same accumulator
      const int kj = partner_[(size_t)q * nk + ki];
      // X[(P,mu)][re p | im p] = [L_re | L_im][(P,mu)] . [[C_re, C_im], [-C_im, C_re]]  (K = 2 ld; the padding of both operands is zero)
      QTRY(gemm((int64_t)naux * nao, 2 * (int64_t)n, 2 * ld, 1.0, pair_[(size_t)ki * nk + kj], 2 * ld, true, Cs.p + kj * csz, 2 * (int64_t)n, false, 0.0, X, 2 * (int64_t)n));
      // M[P][re | im][p][q] += conj(C^ki)^T X[P]:  X[P] read as (mu, re|im) x q, the left operand stored K x M
      QTRY(gemm(2 * (int64_t)n, n, 2 * (int64_t)nao, 1.0, Dk.p + ki * dsz, 2 * (int64_t)n, false, X, n, false, ki == 0 ? 0.0 : 1.0, Macc, n, naux, 0,
                2 * (int64_t)nao * n, 2 * (int64_t)n * n));
    }
    QTRY(dev_kdf_pack(naux, n, Macc, paired, std::sqrt(paired ? 2.0 * c : c), F.p + row0 * np, np, part, scal.p + 2 * iq));
    row0 += (paired ? 2 : 1) * (int64_t)naux;
    ++iq;
  }
  if (row0 != nrows) { set_error("qemb_kdf_transform: the class tables do not give N_k naux factor rows"); return QEMB_ERR_ARG; }
  std::vector<double> sc(2 * (size_t)nkept);
  QTRY(dev_d2h(sc.data(), scal, sizeof(double) * 2 * nkept));
  double asym = 0.0, amax = 0.0;
  for (int k = 0; k < nkept; ++k) { asym = std::fmax(asym, sc[2 * k]); amax = std::fmax(amax, sc[2 * k + 1]); }
  if (!(asym <= 1e-8 * amax)) {      // (also catches a NaN)
    char num[32];
    std::snprintf(num, sizeof num, "%.3e", amax > 0 ? asym / amax : asym);
    set_error(std::string("qemb_kdf_transform: M^q is not symmetric in its two embedding orbitals, largest deviation ") + num +
              " relative to its largest element: the embedding basis TA_k is not time-reversal symmetric");
    return QEMB_ERR_NUMERIC;
  }
  if (with_block) {
    DBuf s4;
    QTRY(s4.alloc(np * np));
    QTRY(df_pair_product(np, nrows, F, s4));
    if (out_host) QTRY(dev_d2h(out_host, s4, sizeof(double) * np * np));
    if (!factor_only && frag) {
      QTRY(frag->adopt_eri_s4(std::move(s4)));
      return frag->adopt_df_factor(std::move(F), (int)nrows);
    }
  }
  return frag ? frag->adopt_df_only(std::move(F), (int)nrows) : QEMB_OK;
}

}  // namespace qemb
