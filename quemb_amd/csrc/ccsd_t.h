// ccsd_t.h -- the perturbative triples correction E_(T) of closed-shell CCSD with a diagonal Fock matrix, from amplitudes and MO blocks on the device
// (Fragment::ccsd_t, qemb_op_ccsd_t).  The expression is stated in ccsd_t_core.h.
//
// The virtual orbitals are cut into tiles of Tv; only tile triples A >= B >= C are visited, in ascending order.  Per call two images are formed,
//   P[a][b][i][f'] = (ia|fb) for f' = f < v, -t2[m,i,b,a] for f' = v + m     and     Q[f'][c][k][j] = t2[k,j,c,f] for f' = f < v, (kc|mj) for f' = v + m,
// and per tile triple g for each of the six arrangements (X,Y,Z) of its tiles is one batched FP64 MFMA product through dev_gemm: per a in X the rows
// (b in Y, i) of P times the columns (c in Z, k, j) of Q -- one contiguous range --, K = v + o, into a buffer of its own (arrangements of equal tiles share
// one).  The particle term is the first v of K, the hole term the last o (ccsd_t_core.h says which arrangement of it a buffer holds).  The assembly kernel
// (ccsd_t_ops.hip) adds the six buffers, forms V, r3(V) and W r3(V) / D and writes one partial sum per (a,b,c); the partials are added in a fixed order and
// the tile triples in ascending order: the same bits on every call.
// Flops: 2 o^3 v^3 (v + o), all of them in the products (each unique triple six times over the symmetry, a sixth of the triples).  Bytes: every buffer is
// written once and read once, 8 o^3 v^3 each way.
#pragma once
#include <cstdint>
#include "dev_ops.h"

namespace qemb {

struct CcsdTStats {
  int tile = 0;
  int64_t n_tile_triples = 0;
  double ms_images = 0.0, ms_gemm = 0.0, ms_assemble = 0.0;      // device time of the three stages of the call (0 with QEMB_TIMERS=0)
  double gemm_flops = 0.0;                                       // 2 M N K batch of the products issued
};

// the tiles the default choice walks down, and the bytes the six buffers of the default may take: three quarters of the 256 MiB Infinity Cache,
// so that what the products write is still there when the assembly reads it (o = 20: Tv = 8, 188 MiB)
constexpr int kCcsdTTiles[] = {16, 8, 4, 2, 1};
constexpr int64_t kCcsdTBufferBytes = (int64_t)192 << 20;

// device bytes of one call beside the handed-in arrays: the two images (v^2 o + v o^2) (v + o), the six buffers, the partial sums, and beyond the LDS form of
// the kernel its scratch
int64_t ccsd_t_bytes(int64_t o, int64_t v, int64_t tile);
// the largest tile of kCcsdTTiles (cut to v) whose buffers fit kCcsdTBufferBytes and whose working set fits room_bytes; 0: not even Tv = 1 fits the room
int ccsd_t_pick_tile(int64_t o, int64_t v, double room_bytes);
inline int64_t ccsd_t_tile_triples(int64_t v, int64_t tile) { const int64_t nt = (v + tile - 1) / tile; return nt * (nt + 1) * (nt + 2) / 6; }

// e_t (host) from device arrays: t1 [o][v], t2 [o][o][v][v], ovvv [o][v][v][v] = (ia|bc), ovoo [o][v][o][o] = (ia|jk), ovov [o][v][o][v] = (ia|jb), eo [o], ev [v].
// tile >= 1 (cut to v).  Fewer than two occupied or two virtual orbitals (no triples): 0.0 without a launch.  Nothing handed in is written.
int ccsd_t_energy(int o, int v, const double* t1, const double* t2, const double* ovvv, const double* ovoo, const double* ovov, const double* eo, const double* ev,
                  int tile, double* e_t, CcsdTStats* stats);

}  // namespace qemb
