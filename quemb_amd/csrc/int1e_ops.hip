// int1e_ops.hip -- the one-electron integrals S, T, V on the device (dev_ops.h: dev_int1e_class; driver in int3c.cpp: int1e_fill; arithmetic in int1e_core.h).
//
// One kernel instantiation per orbital pair class (l_a >= l_b <= 2); one wavefront (a 64-thread workgroup) per shell pair of the class.  The nuclear attraction
// is the expensive part -- work per shell pair ~ atoms x primitive pairs -- so the lanes stride over the (primitive pair, atom) items, each keeping a private
// Cartesian block of at most 36 doubles; the 64 blocks are added by a shuffle tree in a fixed order, lane 0 applies the Cartesian -> spherical matrices and stores
// the block and its mirror image.  S, T and the three dipole components run through the same three steps with the primitive pairs as items.  No atomics: every element is stored once.
// The compiler's resource report of the six classes is in DESIGN.md section 4, "DF mean field on the device".
#include "hip_common.h"
#include "int_dispatch.h"
#include "int1e_core.h"

namespace qemb {
namespace {

using namespace int1e;

template <int LA, int LB>
__global__ void __launch_bounds__(kLanes) int1e_class_kernel(const Args g) {
  const int64_t k = blockIdx.x;
  const int lane = threadIdx.x;
  double acc[int3c::ncart(LA) * int3c::ncart(LB)];
  for (int kind = 0; kind < kKinds; ++kind) {
    double* out = g.out[kind];
    if (!out) continue;      // uniform over the grid
    partial<LA, LB>(kind, g, k, lane, kLanes, acc);
    for (int e = 0; e < int3c::ncart(LA) * int3c::ncart(LB); ++e) {
      double v = acc[e];
      for (int off = kLanes / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kLanes);
      acc[e] = v;
    }
    if (lane == 0) store_block<LA, LB>(g, k, out, acc);
  }
}

}  // namespace

int dev_int1e_class(int la, int lb, const int1e::Args& g) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (int rc = int1e_check_class(la, lb, g)) return rc;
  if (g.npair == 0) return QEMB_OK;
  return dispatch_pair(int4c::pair_class(la, lb), [&](auto A, auto B) {
    return launch("dev_int1e_class", int1e_class_kernel<A(), B()>, dim3((unsigned)g.npair), dim3(kLanes), 0, st, g);
  });
}

}  // namespace qemb
