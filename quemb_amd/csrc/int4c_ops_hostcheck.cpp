// int4c_ops_hostcheck.cpp -- scalar restatement of the device operations of the four-centre integral path for the mock device layer of tests/hostcheck.
// Everything below is compiled only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and int4c_ops.hip provides the operations.
// The arithmetic of one item is the inline code of int4c_core.h that the kernels instantiate per thread; here the items of a class run in a loop.
#ifdef QEMB_HOSTCHECK
#include "int4c_core.h"

namespace qemb {
namespace {

using namespace int4c;

template <int LA, int LB>
void run_pairs(const PairArgs& g) {
  for (int64_t item = 0; item < g.pairs.n * kPrimPairs; ++item) pair_item<LA, LB>(g, item);
}

template <int LA, int LB, int LC, int LD>
void run_class(const ClassArgs& g) {
  const int64_t nitem = class_items<LC, LD>(g);
  for (int64_t item = 0; item < nitem; ++item) quartet_item<LA, LB, LC, LD>(g, item);
}

template <int LA, int LB>
void run_bra(int kc, const ClassArgs& g) {
  constexpr int bc = pair_class(LA, LB);
  switch (kc) {
    case 0: run_class<LA, LB, 0, 0>(g); break;
    case 1: if constexpr (bc >= 1) run_class<LA, LB, 1, 0>(g); break;
    case 2: if constexpr (bc >= 2) run_class<LA, LB, 1, 1>(g); break;
    case 3: if constexpr (bc >= 3) run_class<LA, LB, 2, 0>(g); break;
    case 4: if constexpr (bc >= 4) run_class<LA, LB, 2, 1>(g); break;
    case 5: if constexpr (bc >= 5) run_class<LA, LB, 2, 2>(g); break;
  }
}

template <int LA, int LB, int LC, int LD>
void run_jk(const JkArgs& g) {
  const int64_t nitem = jk_items<LC, LD>(g);
  for (int64_t item = 0; item < nitem; ++item) quartet_jk_item<LA, LB, LC, LD>(g, item);      // QEMB_JK_ADD is a plain += here: one fixed order
}

template <int LA, int LB>
void run_jk_bra(int kc, const JkArgs& g) {
  constexpr int bc = pair_class(LA, LB);
  switch (kc) {
    case 0: run_jk<LA, LB, 0, 0>(g); break;
    case 1: if constexpr (bc >= 1) run_jk<LA, LB, 1, 0>(g); break;
    case 2: if constexpr (bc >= 2) run_jk<LA, LB, 1, 1>(g); break;
    case 3: if constexpr (bc >= 3) run_jk<LA, LB, 2, 0>(g); break;
    case 4: if constexpr (bc >= 4) run_jk<LA, LB, 2, 1>(g); break;
    case 5: if constexpr (bc >= 5) run_jk<LA, LB, 2, 2>(g); break;
  }
}

}  // namespace

int dev_int4c_pairs(int la, int lb, const int4c::PairArgs& g) {
  if (int rc = int4c_check_pairs(la, lb, g)) return rc;
  switch (pair_class(la, lb)) {
    case 0: run_pairs<0, 0>(g); break;
    case 1: run_pairs<1, 0>(g); break;
    case 2: run_pairs<1, 1>(g); break;
    case 3: run_pairs<2, 0>(g); break;
    case 4: run_pairs<2, 1>(g); break;
    default: run_pairs<2, 2>(g); break;
  }
  return 0;
}

int dev_int4c_class(int la, int lb, int lc, int ld, const int4c::ClassArgs& g) {
  if (int rc = int4c_check_class(la, lb, lc, ld, g)) return rc;
  const int kc = pair_class(lc, ld);
  switch (pair_class(la, lb)) {
    case 0: run_bra<0, 0>(kc, g); break;
    case 1: run_bra<1, 0>(kc, g); break;
    case 2: run_bra<1, 1>(kc, g); break;
    case 3: run_bra<2, 0>(kc, g); break;
    case 4: run_bra<2, 1>(kc, g); break;
    default: run_bra<2, 2>(kc, g); break;
  }
  return 0;
}

int dev_int4c_jk_class(int la, int lb, int lc, int ld, const int4c::JkArgs& g) {
  if (int rc = int4c_check_jk(la, lb, lc, ld, g)) return rc;
  const int kc = pair_class(lc, ld);
  switch (pair_class(la, lb)) {
    case 0: run_jk_bra<0, 0>(kc, g); break;
    case 1: run_jk_bra<1, 0>(kc, g); break;
    case 2: run_jk_bra<1, 1>(kc, g); break;
    case 3: run_jk_bra<2, 0>(kc, g); break;
    case 4: run_jk_bra<2, 1>(kc, g); break;
    default: run_jk_bra<2, 2>(kc, g); break;
  }
  return 0;
}

int dev_int4c_pairprod(const int4c::PairProdArgs& g) {
  if (int rc = int4c_check_pairprod(g)) return rc;
  for (int64_t r = 0; r < g.rows; ++r)
    for (int64_t pq = 0; pq < g.npq; ++pq) pairprod_item(g, r, pq);
  return 0;
}

int dev_int4c_add_transpose(int64_t m, double* A) {
  if (m <= 0 || m > 0x7fffffffLL || !A) { set_error("dev_int4c_add_transpose: bad arguments"); return QEMB_ERR_ARG; }
  for (int64_t i = 0; i < m; ++i)
    for (int64_t j = 0; j < m; ++j) addt_item(A, m, i, j);
  return 0;
}

int dev_int4c_dmax(const int3c::Shell* sh, int nshell, int64_t N, const double* dm, double* out) {
  if (!sh || nshell <= 0 || N <= 0 || !dm || !out) { set_error("dev_int4c_dmax: bad arguments"); return QEMB_ERR_ARG; }
  for (int64_t item = 0; item < (int64_t)nshell * nshell; ++item) dmax_item(sh, nshell, N, dm, out, item);
  return 0;
}

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
