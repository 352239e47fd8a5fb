// hip_common.h -- shared helpers for the HIP translation units of libqemb_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "dev_ops.h"

namespace qemb {
hipStream_t hip_stream();  // the library stream (created by dev_init)

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      ::qemb::set_error(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " at " +   \
                        __FILE__ + ":" + std::to_string(__LINE__));                           \
      return QEMB_ERR_DEVICE;                                                              \
    }                                                                                         \
  } while (0)

// One launch of kernel(args...) -- every argument is converted to the kernel's own parameter type -- and its check.  who: the calling dev_* function, for the message.
template <class... P, class... X>
int launch(const char* who, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, X&&... args) {
  static_assert(sizeof...(P) == sizeof...(X), "launch: one argument per kernel parameter");
  hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<X&&>(args)...);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error(std::string(who) + ": kernel launch failed: " + hipGetErrorString(e)); return QEMB_ERR_DEVICE; }
  return QEMB_OK;
}
// One 1-D launch of kernel(g, nitem): nitem work items in blocks of bs threads (bs: the kernel's launch bound).  who: for the messages.
template <class Args>
int launch_items(void (*kernel)(Args, long long), int bs, const Args& g, long long nitem, const char* who, hipStream_t st) {
  const long long nb = (nitem + bs - 1) / bs;
  if (nb > 0x7fffffffLL) { set_error(std::string(who) + ": too many blocks in one launch"); return QEMB_ERR_ARG; }
  if (nb <= 0) return QEMB_OK;
  return launch(who, kernel, dim3((unsigned)nb), dim3(bs), 0, st, g, nitem);
}

// The block's index and the grid's extent as the (BID, GDIM) a groupable kernel's wrapper hands to its body (grouped_launch.h).
__device__ __forceinline__ uint3 block_id() { return make_uint3(blockIdx.x, blockIdx.y, blockIdx.z); }
__device__ __forceinline__ uint3 grid_dim() { return make_uint3(gridDim.x, gridDim.y, gridDim.z); }

// XCD-aware logical block index of the tiled HBM passes (round 4; profiles/r04_hbm_pmc.json).  Workgroups are dealt round-robin over the eight
// XCDs, each with its own L2, so neighbouring 32 x 32 tiles -- whose 256-byte row pieces start at arbitrary offsets and share their first and
// last 128-byte lines -- ran on different XCDs and every shared line was fetched from HBM twice: FETCH_SIZE showed 1.2-1.5 x the algorithmic
// reads for the unpack, scatter and finishing passes.  Here the linear block number is mapped so that each XCD works through ONE contiguous
// range of the logical order (x fastest): neighbours in x run on the same XCD at about the same time and meet in its L2.  A bijection of the
// grid: placement is a matter of speed only (inside a grouped launch the member's blocks are offset and it is merely another permutation).
__device__ __forceinline__ uint3 xcd_logical_block(const uint3 BID, const uint3 GDIM) {
  const unsigned long long total = (unsigned long long)GDIM.x * GDIM.y * GDIM.z;
  const unsigned long long lin = ((unsigned long long)BID.z * GDIM.y + BID.y) * GDIM.x + BID.x;
  const unsigned long long q = total >> 3, r = total & 7ull;
  const unsigned long long xcd = lin & 7ull, k = lin >> 3;
  const unsigned long long base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  const unsigned long long L = base + k;
  const unsigned long long xy = (unsigned long long)GDIM.x * GDIM.y;
  return make_uint3((unsigned)(L % GDIM.x), (unsigned)((L % xy) / GDIM.x), (unsigned)(L / xy));
}
}  // namespace qemb
