// int4c_ops_hostcheck.cpp -- scalar restatement of the device operations of the four-centre integral path for the mock device layer of tests/hostcheck.
// Everything below is compiled only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and int4c_ops.hip provides the operations.
// The arithmetic of one item is the inline code of int4c_core.h that the kernels instantiate per thread; here the items of a class run in a loop, and the class
// is chosen by the dispatchers of int_dispatch.h that choose the kernel in int4c_ops.hip.
#ifdef QEMB_HOSTCHECK
#include "int_dispatch.h"

namespace qemb {
using namespace int4c;

int dev_int4c_pairs(int la, int lb, const int4c::PairArgs& g) {
  if (int rc = int4c_check_pairs(la, lb, g)) return rc;
  return dispatch_pair(pair_class(la, lb), [&](auto A, auto B) {
    for (int64_t item = 0; item < g.pairs.n * kPrimPairs; ++item) pair_item<A(), B()>(g, item);
    return 0;
  });
}

int dev_int4c_class(int la, int lb, int lc, int ld, const int4c::ClassArgs& g) {
  if (int rc = int4c_check_class(la, lb, lc, ld, g)) return rc;
  return dispatch_quartet(pair_class(la, lb), pair_class(lc, ld), "dev_int4c_class", [&](auto A, auto B, auto C, auto D) {
    const int64_t nitem = class_items<C(), D()>(g);
    for (int64_t item = 0; item < nitem; ++item) quartet_item<A(), B(), C(), D()>(g, item);
    return 0;
  });
}

int dev_int4c_jk_class(int la, int lb, int lc, int ld, const int4c::JkArgs& g) {
  if (int rc = int4c_check_jk(la, lb, lc, ld, g)) return rc;
  return dispatch_quartet(pair_class(la, lb), pair_class(lc, ld), "dev_int4c_jk_class", [&](auto A, auto B, auto C, auto D) {
    const int64_t nitem = jk_items<C(), D()>(g);
    for (int64_t item = 0; item < nitem; ++item) quartet_jk_item<A(), B(), C(), D()>(g, item);      // QEMB_JK_ADD is a plain += here: one fixed order
    return 0;
  });
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
