// ccsd_t.cpp -- driver of the perturbative triples correction (see ccsd_t.h; the arithmetic of the assembly step in ccsd_t_core.h).
#include "ccsd_t.h"
#include <algorithm>
#include "ccsd_t_core.h"
#include "tensor_utils.h"

namespace qemb {

int64_t ccsd_t_bytes(int64_t o, int64_t v, int64_t tile) {
  const int64_t T = std::min(std::max<int64_t>(tile, 1), std::max<int64_t>(v, 1)), o3 = o * o * o;
  const int64_t images = (v * v * o + v * o * o) * (v + o);      // [a][b][i][v + o] and [v + o][c][k][j]
  return 8 * (images + 6 * T * T * T * o3 + T * T * T + ccsd_t_tile_triples(v, T) + 1 + ccsd_t_scratch_elems(o, T));
}

// dst[i0 s0 + i1 s1 + i2 s2 + i3 s3] = alpha * src[i0][i1][i2][i3], src contiguous with the extents d0 .. d3
static int place4(double* dst, const double* src, int64_t d0, int64_t d1, int64_t d2, int64_t d3, int64_t s0, int64_t s1, int64_t s2, int64_t s3, double alpha) {
  Copy4Desc c{};
  c.in = src; c.out = dst; c.alpha = alpha; c.beta = 0.0;
  c.dim[0] = d0; c.dim[1] = d1; c.dim[2] = d2; c.dim[3] = d3;
  c.si[3] = 1; c.si[2] = d3; c.si[1] = d3 * d2; c.si[0] = d3 * d2 * d1;
  c.so[0] = s0; c.so[1] = s1; c.so[2] = s2; c.so[3] = s3;
  return dev_copy4(c);
}

int ccsd_t_pick_tile(int64_t o, int64_t v, double room_bytes) {
  int last = 0;
  for (int t : kCcsdTTiles) {
    const int64_t T = std::min<int64_t>(t, v);
    if ((int)T == last) continue;      // (cut to v: the same tile again)
    last = (int)T;
    if (T > 1 && 8 * 6 * T * T * T * o * o * o > kCcsdTBufferBytes) continue;
    if ((double)ccsd_t_bytes(o, v, T) <= room_bytes) return (int)T;
  }
  return 0;
}

int ccsd_t_energy(int o, int v, const double* t1, const double* t2, const double* ovvv, const double* ovoo, const double* ovov, const double* eo, const double* ev,
                  int tile, double* e_t, CcsdTStats* stats) {
  if (e_t) *e_t = 0.0;
  if (stats) *stats = CcsdTStats();
  if (o < 0 || v < 0 || !e_t) { set_error("ccsd_t: bad arguments"); return QEMB_ERR_ARG; }
  if (o < 2 || v < 2) return 0;      // no three electrons can leave the reference
  if (!t1 || !t2 || !ovvv || !ovoo || !ovov || !eo || !ev || tile < 1) { set_error("ccsd_t: bad arguments (the amplitudes, three MO blocks, the orbital energies and a tile >= 1)"); return QEMB_ERR_ARG; }
  const int64_t O = o, V = v, T = std::min(tile, v), o3 = O * O * O, oo = O * O;
  const int64_t nt = (V + T - 1) / T, ntrip = ccsd_t_tile_triples(V, T);
  double ms0[3] = {0, 0, 0};
  const int slots[3] = {TIMER_T_IMAGES, TIMER_T_GEMM, TIMER_T_ASSEMBLE};
  for (int k = 0; k < 3; ++k) QTRY(dev_timer_read(slots[k], &ms0[k], nullptr));
  const int64_t K = V + O;      // the particle and the hole term in one product
  DBuf P, Q, G[6], part, tsum, e, scratch;
  QTRY(P.alloc(V * V * O * K)); QTRY(Q.alloc(K * V * oo));
  for (int k = 0; k < 6; ++k) QTRY(G[k].alloc(T * T * T * o3));
  QTRY(part.alloc(T * T * T)); QTRY(tsum.alloc(ntrip)); QTRY(e.alloc(1));
  if (!ccsd_t_lds_form(o)) QTRY(scratch.alloc(ccsd_t_scratch_elems(o, T)));
  {
    TimerScope lap(TIMER_T_IMAGES);
    // P[a][b][i][f] = (ia|fb), P[a][b][i][v + m] = -t2[m,i,b,a];   Q[f][c][k][j] = t2[k,j,c,f], Q[v + m][c][k][j] = (kc|mj)
    QTRY(place4(P, ovvv, O, V, V, V, K, V * O * K, O * K, 1, 1.0));                 // ovvv[i][a][b][f]
    QTRY(place4(P.p + V, t2, O, O, V, V, K, 1, V * O * K, O * K, -1.0));            // t2[i][m][a][b] = t2[m,i,b,a]
    QTRY(place4(Q, t2, O, O, V, V, O, 1, oo, V * oo, 1.0));                         // t2[k][j][c][f]
    QTRY(place4(Q.p + V * V * oo, ovoo, O, V, O, O, O, oo, V * oo, 1, 1.0));        // ovoo[k][c][m][j]
    QTRY(lap.close());
  }
  QTRY(dev_fill(tsum, ntrip, 0.0));
  double flops = 0.0;
  int64_t t = 0;
  for (int64_t tA = 0; tA < nt; ++tA) for (int64_t tB = 0; tB <= tA; ++tB) for (int64_t tC = 0; tC <= tB; ++tC, ++t) {
    if (T == 1 && tA == tC) continue;      // the one element of this triple is a = b = c: identically zero
    const int64_t tl[3] = {tA, tB, tC};
    static const int arr[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};      // (X,Y,Z) of G_ABC, G_ACB, G_BAC, G_BCA, G_CAB, G_CBA
    CcsdTArgs A{};
    {
      TimerScope lap(TIMER_T_GEMM);
      for (int k = 0; k < 6; ++k) {
        const int64_t X = tl[arr[k][0]], Y = tl[arr[k][1]], Z = tl[arr[k][2]];
        int same = -1;      // an earlier arrangement of the same three tiles: the same buffer
        for (int q = 0; q < k && same < 0; ++q) if (tl[arr[q][0]] == X && tl[arr[q][1]] == Y && tl[arr[q][2]] == Z) same = q;
        if (same >= 0) { A.g[k] = A.g[same]; continue; }
        const int64_t x0 = X * T, y0 = Y * T, z0 = Z * T, tx = std::min(T, V - x0), ty = std::min(T, V - y0), tz = std::min(T, V - z0);
        // per x: C[(y,p)][(z,r,q)] = sum_{f'} P[x][y][p][f'] Q[f'][z][r][q]
        QTRY(gemm(ty * O, tz * oo, K, 1.0, P.p + (x0 * V + y0) * O * K, K, true, Q.p + z0 * oo, V * oo, false, 0.0, G[k], tz * oo, tx, V * O * K, 0, ty * O * tz * oo));
        flops += 2.0 * (double)(ty * O) * (double)(tz * oo) * (double)K * (double)tx;
        A.g[k] = G[k];
      }
      QTRY(lap.close());
    }
    A.o = o; A.v = v;
    A.a0 = (int)(tA * T); A.b0 = (int)(tB * T); A.c0 = (int)(tC * T);
    A.ta = (int)std::min(T, V - A.a0); A.tb = (int)std::min(T, V - A.b0); A.tc = (int)std::min(T, V - A.c0);
    A.t1 = t1; A.ovov = ovov; A.eo = eo; A.ev = ev;
    A.partial = part; A.scratch = scratch.p;
    {
      TimerScope lap(TIMER_T_ASSEMBLE);
      QTRY(dev_ccsd_t_assemble(A));
      QTRY(dev_ccsd_t_sum((int64_t)A.ta * A.tb * A.tc, part, tsum, t));
      QTRY(lap.close());
    }
  }
  QTRY(dev_ccsd_t_total(ntrip, tsum, e));
  QTRY(dev_d2h(e_t, e, sizeof(double)));
  if (stats) {
    stats->tile = (int)T; stats->n_tile_triples = ntrip; stats->gemm_flops = flops;
    double ms1[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) QTRY(dev_timer_read(slots[k], &ms1[k], nullptr));
    stats->ms_images = ms1[0] - ms0[0]; stats->ms_gemm = ms1[1] - ms0[1]; stats->ms_assemble = ms1[2] - ms0[2];
  }
  return 0;
}

}  // namespace qemb
