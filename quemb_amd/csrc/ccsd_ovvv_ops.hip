// ccsd_ovvv_ops.hip -- one pass over ovvv for the two products of the CCSD update that read it in the same layout (dev_ops.h: dev_ccsd_ovvv_pass):
//   ZB[k,c,a,i] = sum_d ovvv[k,c,a,d] t1[i,d]                      (M = o v^2, N = o, K = v)
//   PA[i,a]     = sum_{k,c,d} Thk[k,c,i,d] ovvv[k,c,a,d]           (M = o, N = v, K = o v^2;  Thk: Theta in slab order -- the update passes S = 2T - T')
// Both contract the slab A_s[a,d] = ovvv[k,c,:,:] (s = k v + c, v x v, contiguous) over d, so one product per slab,
//   D_s[a, n] = sum_d A_s[a,d] B_s[n,d],    B_s = [ t1 (o rows) ; Thk[s] (o rows) ]   (2 o <= 16 NT columns),
// gives ZB[s] in its first o columns and the slab's share of PA^T in the next o.  The block is read from HBM once instead of twice, and the padded
// matrix work is ceil(v/16) x NT tiles of v_mfma_f64_16x16x4_f64 per slab instead of 32 + 32 columns (and v padded to 256) in two GEMMs.
//
//  * A persistent grid of G workgroups (dev_ccsd_ovvv_slabs: one per CU, eight waves).  Workgroup g owns the contiguous slabs
//    [g S / G, (g + 1) S / G), S = o v, and walks them in order: the map and the order are fixed, there are no atomics, two runs give the same bits.
//  * One flat sequence of steps (slab, K chunk of 32).  The rows of a step -- 16 ceil(v/16) rows of A_s, then 16 NT rows of B_s -- are staged through one
//    [row][BK + 2] LDS image (the conflict-free image of gemm_f64.hip for K-contiguous operands), two buffers, one barrier per step.  The global loads of
//    step t + 1 (the next slab's first chunk included) are issued into registers before the MFMAs of step t and stored to LDS behind them; the MFMA
//    fragments are read from LDS one k-step ahead.  Rows beyond v
//    or 2 o are clamped to the last valid row (their products land in rows / columns that are never stored); k beyond v is selected to zero.
//  * The ceil(v/16) x NT accumulator tiles are dealt to the eight waves in contiguous ranges of at most OV_MAXU (39 tiles -> 7 x 5 + 4 at v = 200, o = 20).
//    After a slab the columns n < o are stored as ZB[s] (one contiguous v x o block) and cleared by a per-lane select; the columns o <= n < 2 o stay in
//    the registers over all slabs of the workgroup and are written once, as the partial slab PA[g][i][a].  dev_ccsd_t1_assemble adds the G slabs in order.
//    A workgroup without a slab writes zeros.
#include <cstdint>
#include "hip_common.h"

namespace qemb {
namespace ovvv_pass {      // (a named namespace: profiles list the kernel by its name)

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int OV_BK = 32;                 // K chunk of one step
constexpr int OV_LD = OV_BK + 2;          // row stride of the LDS image (doubles)
constexpr int OV_T = 512;                 // threads: eight waves, two per SIMD
constexpr int OV_WAVES = OV_T / 64;
constexpr int OV_MAXU = CCSD_OVVV_MAX_TILES / OV_WAVES;      // accumulator tiles per wave
constexpr int OV_MAXCH = (16 * CCSD_OVVV_MAX_ROWT * (OV_BK / 2) + OV_T - 1) / OV_T;      // staged 16-byte items per thread and step: 256 (RT + NT) items over 512 threads

struct OvvvArgs {
  const double* ovvv; const double* t1; const double* thk;
  double* zb; double* pa;
  int o, v, rt;            // rt = ceil(v / 16)
  long long nslab;         // o v
};

// VEC2: v even -- every pair (row, d .. d + 1) is 16-byte aligned and entirely inside or outside its row; else two 8-byte loads
template <int NT, bool VEC2>
__global__ void __launch_bounds__(OV_T) ccsd_ovvv_pass_kernel(const OvvvArgs g) {
  extern __shared__ __attribute__((aligned(16))) double ov_smem[];
  const int o = g.o, v = g.v, RT = g.rt;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rows = 16 * (RT + NT);
  const int items = rows * (OV_BK / 2);
  const int nch = (items + OV_T - 1) / OV_T;
  double* const buf0 = ov_smem;
  double* const buf1 = ov_smem + rows * OV_LD;

  const long long G = gridDim.x, bid = blockIdx.x;
  const long long s_beg = bid * g.nslab / G, s_end = (bid + 1) * g.nslab / G;
  const int nchunk = (v + OV_BK - 1) / OV_BK;
  const long long nstep = (s_end - s_beg) * nchunk;

  // ---- this wave's accumulator tiles: units u = ct RT + rt in [u_beg, u_beg + cnt)
  const int units = RT * NT, per = (units + OV_WAVES - 1) / OV_WAVES;
  const int u_beg = wave * per < units ? wave * per : units - 1;
  const int cnt = (units - wave * per) < 0 ? 0 : ((units - wave * per) < per ? (units - wave * per) : per);
  const int ct_beg = u_beg / RT, rt_beg = u_beg - ct_beg * RT;
  auto next_tile = [&](int& rt, int& ct) { ++rt; if (rt == RT) { rt = 0; ct = ct + 1 < NT ? ct + 1 : ct; } };      // (past the last tile: stays inside the image)
  // the rows of slot j's two fragments in the LDS image (wave-uniform): both are read per tile -- one more LDS read per MFMA than keeping the NT column
  // fragments and selecting, but no select chain and a third of the scalar registers
  int a_off[OV_MAXU], b_off[OV_MAXU];
  {
    int rt = rt_beg, ct = ct_beg;
#pragma unroll
    for (int j = 0; j < OV_MAXU; ++j) { a_off[j] = (16 * rt) * OV_LD; b_off[j] = (16 * (RT + ct)) * OV_LD; next_tile(rt, ct); }
  }
  d4 acc[OV_MAXU];
#pragma unroll
  for (int j = 0; j < OV_MAXU; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};

  // ---- this thread's staged items: item = tid + c OV_T -> (row R, pair p) of the step's image
  constexpr int PPR = OV_BK / 2;            // pairs per row of the image
  const int p2 = (tid % PPR) * 2;           // first k of the pair inside the chunk (the same for every c: the thread count is a multiple of PPR)
  int row_off[OV_MAXCH], row_kind[OV_MAXCH];      // offset of the row in its source; source: 0 the ovvv slab, 1 t1, 2 the slab's Thk rows
#pragma unroll
  for (int c = 0; c < OV_MAXCH; ++c) {
    int R = (tid + c * OV_T) / PPR;
    R = R < rows ? R : rows - 1;
    if (R < 16 * RT) { const int a = R < v ? R : v - 1; row_off[c] = a * v; row_kind[c] = 0; }
    else {
      int n = R - 16 * RT;
      n = n < 2 * o ? n : 2 * o - 1;
      row_kind[c] = n < o ? 1 : 2;
      row_off[c] = (n < o ? n : n - o) * v;
    }
  }
  // No branch around a load and no use of a loaded value before stash: a branch, or a select on the value, makes the compiler wait for the load where it
  // stands, and the loads of a step would then run one after the other instead of beside the MFMAs.  Items beyond the image (c >= nch, or the second half of
  // the threads in the last round) load the image's last row again -- a line the same wave has just asked for -- and are not stored.
  double reg[OV_MAXCH][2];
  int fetched_d = 0;                        // the first k of this thread's pair in the step the registers hold: k >= v is stored as zero
  auto fetch = [&](long long s, int k0) {
    const double* __restrict__ pA = g.ovvv + s * (long long)v * v;
    const double* __restrict__ pT = g.thk + s * (long long)o * v;
    const int d = k0 + p2;
    fetched_d = d;
#pragma unroll
    for (int c = 0; c < OV_MAXCH; ++c) {
      const double* __restrict__ src = (row_kind[c] == 0 ? pA : row_kind[c] == 1 ? g.t1 : pT) + row_off[c];
      if constexpr (VEC2) {
        const int dc = d < v ? d : v - 2;
        const d2 x = *reinterpret_cast<const d2*>(src + dc);
        reg[c][0] = x[0];
        reg[c][1] = x[1];
      } else {
        const int d0 = d < v ? d : v - 1, d1 = d + 1 < v ? d + 1 : v - 1;
        reg[c][0] = src[d0];
        reg[c][1] = src[d1];
      }
    }
  };
  auto stash = [&](double* __restrict__ S) {
    const bool in0 = fetched_d < v, in1 = fetched_d + 1 < v;
#pragma unroll
    for (int c = 0; c < OV_MAXCH; ++c) {
      const int item = tid + c * OV_T;
      if (c < nch && item < items) *reinterpret_cast<d2*>(S + (item / PPR) * OV_LD + p2) = d2{in0 ? reg[c][0] : 0.0, in1 ? reg[c][1] : 0.0};
    }
  };

  if (nstep > 0) {
    fetch(s_beg, 0);
    stash(buf0);
    __syncthreads();
    long long s = s_beg;
    int ch = 0;
    for (long long t = 0; t < nstep; ++t) {
      // the next step's operands (the last step asks for itself again: no branch around the loads)
      {
        const bool last = (t + 1 == nstep);
        const bool wrap = (ch + 1 == nchunk);
        const long long sn = last ? s : (wrap ? s + 1 : s);
        const int chn = last ? ch : (wrap ? 0 : ch + 1);
        fetch(sn, chn * OV_BK);
      }
      const double* __restrict__ S = (t & 1) ? buf1 : buf0;
      const int kleft = v - ch * OV_BK;
      const int nks = ((kleft < OV_BK ? kleft : OV_BK) + 3) >> 2;
      const double* __restrict__ frag = S + l15 * OV_LD + l4;      // lane (l15, l4) of a fragment: row l15 of its 16-row tile, k = l4 of the k-step
      // fragments one k-step ahead of the MFMAs that use them (two register sets): the eight waves leave the barrier together and ask the LDS for their
      // fragments at the same time, so a k-step's reads come back later than the other wave of the SIMD needs for its MFMAs -- unless they were asked for
      // a whole k-step earlier.  (The last k-step asks for itself again: no branch around the reads.)
      auto load_frags = [&](double (&bf)[OV_MAXU], double (&af)[OV_MAXU], int ks) {
#pragma unroll
        for (int j = 0; j < OV_MAXU; ++j) { af[j] = frag[a_off[j] + 4 * ks]; bf[j] = frag[b_off[j] + 4 * ks]; }
      };
      auto mfmas = [&](const double (&bf)[OV_MAXU], const double (&af)[OV_MAXU]) {
#pragma unroll
        for (int j = 0; j < OV_MAXU; ++j)
          if (j < cnt) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[j], bf[j], acc[j], 0, 0, 0);
      };
      double bf0[OV_MAXU], af0[OV_MAXU], bf1[OV_MAXU], af1[OV_MAXU];
      load_frags(bf0, af0, 0);
      for (int ks = 0; ks < nks; ks += 2) {
        load_frags(bf1, af1, ks + 1 < nks ? ks + 1 : nks - 1);
        mfmas(bf0, af0);
        if (ks + 1 < nks) {
          load_frags(bf0, af0, ks + 2 < nks ? ks + 2 : nks - 1);
          mfmas(bf1, af1);
        }
      }
      if (ch + 1 == nchunk) {
        // the slab is done: its t1 columns are ZB[s] (v x o, contiguous), stored and cleared; the Thk columns stay
        double* __restrict__ zb = g.zb + s * (long long)v * o;
        int rt = rt_beg, ct = ct_beg;
#pragma unroll
        for (int j = 0; j < OV_MAXU; ++j) {
          if (j < cnt && 16 * ct < o) {
            const int i = 16 * ct + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int a = 16 * rt + l4 + 4 * r;
              if (a < v && i < o) zb[(long long)a * o + i] = acc[j][r];
              acc[j][r] = (i < o) ? 0.0 : acc[j][r];
            }
          }
          next_tile(rt, ct);
        }
        ch = 0; ++s;
      } else {
        ++ch;
      }
      stash((t & 1) ? buf0 : buf1);
      __syncthreads();
    }
  }
  // ---- the workgroup's partial slab PA[g][i][a] from the columns o <= n < 2 o
  double* __restrict__ pa = g.pa + bid * (long long)o * v;
  int rt = rt_beg, ct = ct_beg;
#pragma unroll
  for (int j = 0; j < OV_MAXU; ++j) {
    if (j < cnt) {
      const int i = 16 * ct + l15 - o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int a = 16 * rt + l4 + 4 * r;
        if (a < v && i >= 0 && i < o) pa[(long long)i * v + a] = acc[j][r];
      }
    }
    next_tile(rt, ct);
  }
}

size_t ovvv_lds_bytes(int64_t o, int64_t v) {
  const int64_t rt = (v + 15) / 16, nt = (2 * o + 15) / 16;
  return (size_t)(2 * 16 * (rt + nt) * OV_LD) * sizeof(double);
}

template <int NT, bool VEC2>
int launch_ovvv(const OvvvArgs& a, int G, size_t lds, hipStream_t st) {
  auto kern = ccsd_ovvv_pass_kernel<NT, VEC2>;
  static bool attr_set = false;     // (benign if two threads both set it once)
  if (!attr_set) {
    HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(CCSD_OVVV_MAX_ROWT * 2 * 16 * OV_LD * sizeof(double))));
    attr_set = true;
  }
  return launch("dev_ccsd_ovvv_pass", kern, dim3((unsigned)G), dim3(OV_T), lds, st, a);
}

}  // namespace ovvv_pass
using namespace ovvv_pass;

// G: one workgroup of eight waves per CU
int dev_ccsd_ovvv_slabs(int64_t o, int64_t v) {
  if (!ccsd_ovvv_shape_ok(o, v)) return 0;
  static const int ncu = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError(); n = 256; }
    return n;
  }();
  return ncu;
}

int dev_ccsd_ovvv_pass(int64_t o, int64_t v, const double* ovvv, const double* t1, const double* Thk, double* ZB, double* PA) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (!ccsd_ovvv_shape_ok(o, v)) { set_error("dev_ccsd_ovvv_pass: shape outside the kernel's limits (ccsd_ovvv_shape_ok)"); return QEMB_ERR_ARG; }
  if (!ovvv || !t1 || !Thk || !ZB || !PA) { set_error("dev_ccsd_ovvv_pass: bad arguments"); return QEMB_ERR_ARG; }
  const int G = dev_ccsd_ovvv_slabs(o, v);
  OvvvArgs a{ovvv, t1, Thk, ZB, PA, (int)o, (int)v, (int)((v + 15) / 16), (long long)(o * v)};
  const size_t lds = ovvv_lds_bytes(o, v);
  const int nt = (int)((2 * o + 15) / 16);
  const bool vec2 = (v % 2) == 0 && (((uintptr_t)ovvv | (uintptr_t)t1 | (uintptr_t)Thk) & 15) == 0;      // 16-byte loads: every row then starts on a 16-byte boundary
#define QEMB_OVVV_CASE(N)                                                                                  \
  if (nt == N) return vec2 ? launch_ovvv<N, true>(a, G, lds, st) : launch_ovvv<N, false>(a, G, lds, st);
  QEMB_OVVV_CASE(1)
  QEMB_OVVV_CASE(2)
  QEMB_OVVV_CASE(3)
  QEMB_OVVV_CASE(4)
#undef QEMB_OVVV_CASE
  set_error("dev_ccsd_ovvv_pass: no kernel for this n_occ");
  return QEMB_ERR_ARG;
}

}  // namespace qemb
