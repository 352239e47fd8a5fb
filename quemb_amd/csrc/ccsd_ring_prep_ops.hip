// ccsd_ring_prep_ops.hip -- two passes of the CCSD update that consume the raw ZB through an LDS transpose: the rank-n_occ update of U with U += ZB^T in
// the same sweep (dev_ops.h: dev_ccsd_u_update; second half of this file), and the t1-dependent parts of both ring intermediates in one pass
// (dev_ops.h: dev_ccsd_ring_prep):
//   W2[i,a,k,c] = W2base[i,a,k,c] + ZC[k,i,a,c] - sum_l t1[l,a] OC[k,i,l,c]                                   (OC[k,i,l,c] = ovoo[l,c,k,i])
//   R [i,a,k,c] = P1[i,a,k,c] + W1base[i,a,k,c] + ZB[k,c,a,i] - sum_l t1[l,a] OB[k,i,l,c] - 1/2 W2[i,a,k,c]   (OB[k,i,l,c] = ovoo[k,c,l,i])
// ZB is [k][c][a][i], ZC is [k][i][a][c], everything else [i][a][k][c]; ZB and ZC are only read.
// Order of the additions, the same in the scalar twin (ccsd_ring_prep_ops_hostcheck.cpp):
//   W2 = (W2base + ZC) - sC,   R = (((P1 + W1base) + ZB) - sB) - 1/2 W2,
// sB, sC: the sums over l from zero in ascending l, four at a time as v_mfma_f64_16x16x4_f64 adds them.  No atomics, a fixed map of outputs to lanes:
// two runs give the same bits.
//
//  * One workgroup (four waves) per (k, 16 values of a, 16 values of c) and all i.  For that set ZB[k,c,a0..,:] is one contiguous run of 16 o doubles per c:
//    the sixteen runs are read along i (16-byte loads when o is even, else 8-byte) into an LDS image [c][a][i] and read back with c across the lanes --
//    the transpose i <-> c of the pass.  Row stride 16 o + 2 (o even) or 16 o + 1 doubles: the sixteen lanes of one a fall on sixteen different banks.
//  * Wave w takes i = w, w + 4, ...  For one i the two corrections are two 16 x 16 x o products with the same left operand t1[:, a0..]^T, held as
//    ceil(o/4) MFMA fragments for the whole workgroup; the right operands are the [l][c] slabs OB[k,i], OC[k,i] (o^3 v doubles each, read from L2: a slab is
//    used by the ceil(v/16) workgroups of its row of tiles).  On the vector unit the 2 o multiply-adds per element would cost as much as the rank-n_occ
//    updates this pass replaces (dev_ops_hip.hip, small_k_update_mfma_kernel); on the matrix pipe they are 2 ceil(o/4) instructions per 256 elements.
//  * The result fragment of lane (l15, l4) is (a = a0 + l4 + 4 r, c = c0 + l15), r < 4: every load of P1, W1base, W2base, ZC and every store of R, W2 is
//    sixteen lanes on 128 contiguous bytes of a row [i][a][k][:], four rows per instruction.  Neighbouring c tiles run on one XCD (xcd_logical_block).
#include <cstdint>
#include "hip_common.h"

namespace qemb {
namespace ring_prep {      // (a named namespace: profiles list the kernel by its name)

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int RP_T = 256;                 // threads: four waves
constexpr int RP_WAVES = RP_T / 64;
constexpr int RP_TILE = 16;               // a and c values of a workgroup (one MFMA result tile)

struct RingPrepArgs {
  const double* t1; const double* P1; const double* W1base; const double* W2base; const double* ZB; const double* ZC; const double* OB; const double* OC;
  double* R; double* W2;
  int o, v, tiles, ldc;      // tiles = ceil(v / 16); ldc: row stride of the LDS image (doubles)
};

// KS = ceil(o / 4) k-steps.  VEC2: o even and ZB on a 16-byte boundary -- every run of ZB then starts on one and has an even length
template <int KS, bool VEC2>
__global__ void __launch_bounds__(RP_T) ccsd_ring_prep_kernel(const RingPrepArgs g) {
  extern __shared__ __attribute__((aligned(16))) double rp_smem[];
  const int o = g.o, v = g.v, ldc = g.ldc;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint3 LB = xcd_logical_block(block_id(), grid_dim());
  const int ct = (int)(LB.x % (unsigned)g.tiles), at = (int)(LB.x / (unsigned)g.tiles), k = (int)LB.y;
  const int c0 = RP_TILE * ct, a0 = RP_TILE * at;
  const int nc = (v - c0 < RP_TILE) ? v - c0 : RP_TILE, na = (v - a0 < RP_TILE) ? v - a0 : RP_TILE;

  // ---- ZB[k, c0 .. c0 + nc, a0 .. a0 + na, :] -> image[c][a o + i]
  {
    const int run = na * o;
    const long long row = (long long)v * o;
    const double* __restrict__ zb = g.ZB + (((long long)k * v + c0) * v + a0) * o;
    if constexpr (VEC2) {
      const int pairs = run >> 1;
      for (int idx = tid; idx < nc * pairs; idx += RP_T) {
        const int cl = idx / pairs, j = 2 * (idx - cl * pairs);
        *reinterpret_cast<d2*>(rp_smem + cl * ldc + j) = *reinterpret_cast<const d2*>(zb + cl * row + j);
      }
    } else {
      for (int idx = tid; idx < nc * run; idx += RP_T) {
        const int cl = idx / run, j = idx - cl * run;
        rp_smem[cl * ldc + j] = zb[cl * row + j];
      }
    }
  }
  // ---- the left operand of both products: t1[l, a0 + l15], l = 4 ks + l4 (zero beyond o or v)
  const int c = c0 + l15;
  const bool cin = c < v;
  double af[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int l = 4 * ks + l4, a = a0 + l15;
    af[ks] = (l < o && a < v) ? g.t1[(long long)l * v + a] : 0.0;
  }
  __syncthreads();

  for (int i = wave; i < o; i += RP_WAVES) {
    const long long slab = ((long long)k * o + i) * o * v;
    const double* __restrict__ ob = g.OB + slab;
    const double* __restrict__ oc = g.OC + slab;
    double bb[KS], bc[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int l = 4 * ks + l4;
      const bool in = cin && l < o;
      bb[ks] = in ? ob[(long long)l * v + c] : 0.0;
      bc[ks] = in ? oc[(long long)l * v + c] : 0.0;
    }
    double p1[4], w1[4], w2[4], zc[4], zb[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int al = l4 + 4 * r, a = a0 + al;
      const bool in = cin && a < v;
      const long long off = (((long long)i * v + a) * o + k) * v + c;
      p1[r] = in ? g.P1[off] : 0.0;
      w1[r] = in ? g.W1base[off] : 0.0;
      w2[r] = in ? g.W2base[off] : 0.0;
      zc[r] = in ? g.ZC[(((long long)k * o + i) * v + a) * v + c] : 0.0;
      zb[r] = in ? rp_smem[l15 * ldc + al * o + i] : 0.0;
    }
    d4 sB = {0.0, 0.0, 0.0, 0.0}, sC = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      sB = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ks], bb[ks], sB, 0, 0, 0);
      sC = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ks], bc[ks], sC, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = a0 + l4 + 4 * r;
      if (cin && a < v) {
        const long long off = (((long long)i * v + a) * o + k) * v + c;
        const double w = (w2[r] + zc[r]) - sC[r];
        g.W2[off] = w;
        g.R[off] = (((p1[r] + w1[r]) + zb[r]) - sB[r]) - 0.5 * w;
      }
    }
  }
}

// The rank-n_occ update of U with the transposed addend folded in (dev_ops.h: dev_ccsd_u_update), one sweep over U instead of two:
//   U[i,j,a,b] = (U[i,j,a,b] + Z[i,a,b,j]) - sum_k A[i,j,k,a] t1[k,b]
// The same scheme with the roles turned: one workgroup per (i, 16 a, 16 b) and all j; Z[i,a,b0..,:] is one contiguous run of 16 o doubles per a, staged as the
// image [a][b o + j]; wave w takes j = w, w + 4, ...; the left operand of the 16 x 16 x o product is the slab A[i,j] ([k][a], read along a), the right one t1[:, b0..]
// in registers.  The result lane (a = a0 + l4 + 4 r, b = b0 + l15) reads and writes 128 contiguous bytes of a row U[i,j,a,:] per sixteen lanes.
struct UUpdateArgs {
  const double* A; const double* t1; const double* Z; double* U;
  int o, v, tiles, ldc;
};
template <int KS, bool VEC2>
__global__ void __launch_bounds__(RP_T) ccsd_u_update_kernel(const UUpdateArgs g) {
  extern __shared__ __attribute__((aligned(16))) double rp_smem[];
  const int o = g.o, v = g.v, ldc = g.ldc;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint3 LB = xcd_logical_block(block_id(), grid_dim());
  const int bt = (int)(LB.x % (unsigned)g.tiles), at = (int)(LB.x / (unsigned)g.tiles), i = (int)LB.y;
  const int b0 = RP_TILE * bt, a0 = RP_TILE * at;
  const int nb = (v - b0 < RP_TILE) ? v - b0 : RP_TILE, na = (v - a0 < RP_TILE) ? v - a0 : RP_TILE;
  // ---- Z[i, a0 .. a0 + na, b0 .. b0 + nb, :] -> image[a][b o + j]
  {
    const int run = nb * o;
    const long long row = (long long)v * o;
    const double* __restrict__ z = g.Z + (((long long)i * v + a0) * v + b0) * o;
    if constexpr (VEC2) {
      const int pairs = run >> 1;
      for (int idx = tid; idx < na * pairs; idx += RP_T) {
        const int al = idx / pairs, q = 2 * (idx - al * pairs);
        *reinterpret_cast<d2*>(rp_smem + al * ldc + q) = *reinterpret_cast<const d2*>(z + al * row + q);
      }
    } else {
      for (int idx = tid; idx < na * run; idx += RP_T) {
        const int al = idx / run, q = idx - al * run;
        rp_smem[al * ldc + q] = z[al * row + q];
      }
    }
  }
  // ---- the right operand: t1[k, b0 + l15], k = 4 ks + l4 (zero beyond o or v)
  const int b = b0 + l15;
  const bool bin = b < v;
  double bf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int k = 4 * ks + l4;
    bf[ks] = (k < o && bin) ? g.t1[(long long)k * v + b] : 0.0;
  }
  __syncthreads();

  for (int j = wave; j < o; j += RP_WAVES) {
    const long long ij = (long long)i * o + j;
    const double* __restrict__ As = g.A + ij * o * v;
    double* __restrict__ Uz = g.U + ij * v * v;
    double af[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = 4 * ks + l4, a = a0 + l15;
      af[ks] = (k < o && a < v) ? As[(long long)k * v + a] : 0.0;
    }
    double u[4], z[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int al = l4 + 4 * r, a = a0 + al;
      const bool in = bin && a < v;
      u[r] = in ? Uz[(long long)a * v + b] : 0.0;
      z[r] = in ? rp_smem[al * ldc + l15 * o + j] : 0.0;
    }
    d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ks], bf[ks], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int a = a0 + l4 + 4 * r;
      if (bin && a < v) Uz[(long long)a * v + b] = (u[r] + z[r]) - acc[r];
    }
  }
}

static int rp_ldc(int64_t o) { return (int)(RP_TILE * o + ((o % 2 == 0) ? 2 : 1)); }

template <int KS, bool VEC2>
int launch_ring_prep(const RingPrepArgs& a, hipStream_t st) {
  auto kern = ccsd_ring_prep_kernel<KS, VEC2>;
  static bool attr_set = false;     // (benign if two threads both set it once)
  if (!attr_set) {
    HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(RP_TILE * rp_ldc(CCSD_RING_PREP_MAX_O) * sizeof(double))));
    attr_set = true;
  }
  const size_t lds = (size_t)RP_TILE * a.ldc * sizeof(double);
  return launch("dev_ccsd_ring_prep", kern, dim3((unsigned)(a.tiles * a.tiles), (unsigned)a.o), dim3(RP_T), lds, st, a);
}

template <int KS, bool VEC2>
int launch_u_update(const UUpdateArgs& a, hipStream_t st) {
  auto kern = ccsd_u_update_kernel<KS, VEC2>;
  static bool attr_set = false;     // (benign if two threads both set it once)
  if (!attr_set) {
    HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(RP_TILE * rp_ldc(CCSD_RING_PREP_MAX_O) * sizeof(double))));
    attr_set = true;
  }
  const size_t lds = (size_t)RP_TILE * a.ldc * sizeof(double);
  return launch("dev_ccsd_u_update", kern, dim3((unsigned)(a.tiles * a.tiles), (unsigned)a.o), dim3(RP_T), lds, st, a);
}

}  // namespace ring_prep
using namespace ring_prep;

int dev_ccsd_ring_prep(int64_t o, int64_t v, const double* t1, const double* P1, const double* W1base, const double* W2base, const double* ZB, const double* ZC,
                       const double* OB, const double* OC, double* R, double* W2) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (!ccsd_ring_prep_shape_ok(o, v)) { set_error("dev_ccsd_ring_prep: shape outside the kernel's limits (ccsd_ring_prep_shape_ok)"); return QEMB_ERR_ARG; }
  if (!t1 || !P1 || !W1base || !W2base || !ZB || !ZC || !OB || !OC || !R || !W2) { set_error("dev_ccsd_ring_prep: bad arguments"); return QEMB_ERR_ARG; }
  RingPrepArgs a{t1, P1, W1base, W2base, ZB, ZC, OB, OC, R, W2, (int)o, (int)v, (int)((v + RP_TILE - 1) / RP_TILE), rp_ldc(o)};
  const bool vec2 = (o % 2) == 0 && ((uintptr_t)ZB & 15) == 0;
  if (!vec2) a.ldc = (int)(RP_TILE * o + 1);
  const int ks = (int)((o + 3) / 4);
#define QEMB_RING_PREP_CASE(N)                                                                                  \
  if (ks == N) return vec2 ? launch_ring_prep<N, true>(a, st) : launch_ring_prep<N, false>(a, st);
  QEMB_RING_PREP_CASE(1)
  QEMB_RING_PREP_CASE(2)
  QEMB_RING_PREP_CASE(3)
  QEMB_RING_PREP_CASE(4)
  QEMB_RING_PREP_CASE(5)
  QEMB_RING_PREP_CASE(6)
  QEMB_RING_PREP_CASE(7)
  QEMB_RING_PREP_CASE(8)
#undef QEMB_RING_PREP_CASE
  set_error("dev_ccsd_ring_prep: no kernel for this n_occ");
  return QEMB_ERR_ARG;
}

int dev_ccsd_u_update(int64_t o, int64_t v, const double* A, const double* t1, const double* Z, double* U) {
  hipStream_t st = hip_stream();
  if (!st) { set_error("libqemb_hip: call qemb_init(device) first"); return QEMB_ERR_DEVICE; }
  if (!ccsd_ring_prep_shape_ok(o, v)) { set_error("dev_ccsd_u_update: shape outside the kernel's limits (ccsd_ring_prep_shape_ok)"); return QEMB_ERR_ARG; }
  if (!A || !t1 || !Z || !U) { set_error("dev_ccsd_u_update: bad arguments"); return QEMB_ERR_ARG; }
  const bool vec2 = (o % 2) == 0 && ((uintptr_t)Z & 15) == 0;
  UUpdateArgs a{A, t1, Z, U, (int)o, (int)v, (int)((v + RP_TILE - 1) / RP_TILE), vec2 ? rp_ldc(o) : (int)(RP_TILE * o + 1)};
  const int ks = (int)((o + 3) / 4);
#define QEMB_U_UPDATE_CASE(N)                                                                                  \
  if (ks == N) return vec2 ? launch_u_update<N, true>(a, st) : launch_u_update<N, false>(a, st);
  QEMB_U_UPDATE_CASE(1)
  QEMB_U_UPDATE_CASE(2)
  QEMB_U_UPDATE_CASE(3)
  QEMB_U_UPDATE_CASE(4)
  QEMB_U_UPDATE_CASE(5)
  QEMB_U_UPDATE_CASE(6)
  QEMB_U_UPDATE_CASE(7)
  QEMB_U_UPDATE_CASE(8)
#undef QEMB_U_UPDATE_CASE
  set_error("dev_ccsd_u_update: no kernel for this n_occ");
  return QEMB_ERR_ARG;
}

}  // namespace qemb
