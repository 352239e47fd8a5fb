// int3c_ops_hostcheck.cpp -- scalar restatement of the device operations of the DF integral path for the mock device layer of tests/hostcheck.
// Everything below is compiled only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and int3c_ops.hip provides the operations.
// The arithmetic of one block is the inline code of int3c_core.h that the kernels instantiate per thread; here the blocks of a class run in a loop, and the
// class is chosen by the dispatcher of int_dispatch.h that chooses the kernel in int3c_ops.hip.
#ifdef QEMB_HOSTCHECK
#include "int_dispatch.h"

namespace qemb {
using namespace int3c;

int dev_boys(int m_max, int64_t n, const double* x, double* out) {
  if (int rc = int3c_check_boys(m_max, n, x, out)) return rc;
  for (int64_t i = 0; i < n; ++i) {
    double F[2 * kMaxL + 2 * 2 + 1];
    boys(m_max, x[i], F);
    for (int m = 0; m <= m_max; ++m) out[i * (m_max + 1) + m] = F[m];
  }
  return 0;
}

int dev_int3c_class(int la, int lb, int lp, const int3c::ClassArgs& g) {
  if (int rc = int3c_check_class(la, lb, lp, g)) return rc;
  return dispatch_int3c(la, lb, lp, [&](auto A, auto B, auto P) {
    for (int64_t item = 0; item < g.npair * g.naux_sh; ++item) class_item<A(), B(), P()>(g, item);
    return 0;
  });
}

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
