// int3c_ops_hostcheck.cpp -- scalar restatement of the device operations of the DF integral path for the mock device layer of tests/hostcheck.
// Everything below is compiled only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and int3c_ops.hip provides the operations.
// The arithmetic of one block is the inline code of int3c_core.h that the kernels instantiate per thread; here the blocks of a class run in a loop.
#ifdef QEMB_HOSTCHECK
#include "int3c_core.h"

namespace qemb {
namespace {

using namespace int3c;

template <int LA, int LB, int LP>
void run_class(const ClassArgs& g) {
  const int64_t nitem = g.npair * g.naux_sh;
  for (int64_t item = 0; item < nitem; ++item) class_item<LA, LB, LP>(g, item);
}

template <int LA, int LB>
void run_ab(int lp, const ClassArgs& g) {
  switch (lp) {
    case 0: return run_class<LA, LB, 0>(g);
    case 1: return run_class<LA, LB, 1>(g);
    case 2: return run_class<LA, LB, 2>(g);
    case 3: return run_class<LA, LB, 3>(g);
    default: return run_class<LA, LB, 4>(g);
  }
}

}  // namespace

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
  switch (la * 8 + lb) {
    case 0: run_ab<0, 0>(lp, g); break;
    case 8: run_ab<1, 0>(lp, g); break;
    case 9: run_ab<1, 1>(lp, g); break;
    case 16: run_ab<2, 0>(lp, g); break;
    case 17: run_ab<2, 1>(lp, g); break;
    case 18: run_ab<2, 2>(lp, g); break;
    case 24: run_ab<3, 0>(lp, g); break;
    default: run_ab<4, 0>(lp, g); break;
  }
  return 0;
}

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
