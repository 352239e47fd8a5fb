// int1e_ops_hostcheck.cpp -- scalar restatement of the one-electron integral kernel for the mock device layer of tests/hostcheck.
// Everything below is compiled only with -DQEMB_HOSTCHECK: in the product build this file is an empty object and int1e_ops.hip provides the operation.
// The arithmetic is the inline code of int1e_core.h that the kernel instantiates per lane; here the 64 lanes of a shell pair run in a loop and their blocks are
// added by the same binary tree, in the same order, as the kernel's shuffle reduction.
#ifdef QEMB_HOSTCHECK
#include "int_dispatch.h"
#include "int1e_core.h"

namespace qemb {
using namespace int1e;

int dev_int1e_class(int la, int lb, const int1e::Args& g) {
  if (int rc = int1e_check_class(la, lb, g)) return rc;
  return dispatch_pair(int4c::pair_class(la, lb), [&](auto A, auto B) {
    constexpr int nb = int3c::ncart(A()) * int3c::ncart(B());
    double part[kLanes][kMaxBlock];
    for (int64_t k = 0; k < g.npair; ++k)
      for (int kind = 0; kind < kKinds; ++kind) {
        if (!g.out[kind]) continue;
        for (int lane = 0; lane < kLanes; ++lane) partial<A(), B()>(kind, g, k, lane, kLanes, part[lane]);
        for (int off = kLanes / 2; off > 0; off >>= 1)
          for (int lane = 0; lane < off; ++lane)
            for (int e = 0; e < nb; ++e) part[lane][e] += part[lane + off][e];
        store_block<A(), B()>(g, k, g.out[kind], part[0]);
      }
    return 0;
  });
}

}  // namespace qemb
#endif  // QEMB_HOSTCHECK
