// gemm_tiles.h -- the production tile configurations of dev_gemm, stated once.  The dispatcher (gemm_f64.hip) instantiates its kernels from
// this list and the drivers that choose a tile themselves read its dimensions from here, so the two cannot disagree.  The ids are part of the
// test / tool surface (qemb_set_gemm_config, qemb_op_gemm_probe, profiles/): never renumbered.
#pragma once
#include <cstdint>

namespace qemb {

// X(id, rows x cols, WM, WN, WAVES_M, WAVES_N, BK, MODE1, CLASSIC): a workgroup of WAVES_M x WAVES_N waves, each holding WM x WN MFMA tiles of 16 x 16,
// k-steps of BK.  MODE1: the large tiles run the MODE 1 main loop (explicit one-k-step-ahead LDS fragment reads, LDS stores spread behind the MFMA
// rows) when the operands allow 16-byte loads; the single-column wave tiles and the small / skinny tiles, which are latency or HBM bound and want the
// two-tiles-deep register prefetch, keep the classic loop.  CLASSIC: the classic (MODE 0) loop of a MODE 1 tile is addressable as id + 200, for A/B
// measurements (tools/gemm_modes.py) and for the bit-for-bit comparison tests/test_gpu_ops.py::test_gemm_mode1_equals_classic_loop runs, so that a
// toolchain change that breaks the hand-counted LDS waits of MODE 1 is caught (same summation order: results must be identical).
#define QEMB_GEMM_TILES(X)                                                                                                                                  \
  X(0, 128x128, 4, 4, 2, 2, 16, 1, 1)       /* 4 waves */                                                                                                   \
  X(1, 64x64, 2, 2, 2, 2, 16, 1, 1)         /* 4 waves */                                                                                                   \
  X(2, 32x32, 1, 1, 2, 2, 32, 0, 0)         /* 4 waves */                                                                                                   \
  X(4, 128x256, 4, 4, 2, 4, 16, 1, 1)       /* 8 waves: the (ov)^3 ring products of large fragments */                                                      \
  X(10, 224x128_COL, 14, 1, 1, 8, 16, 0, 0) /* 8 waves along N: all packed (i >= j) rows of o = 20 in ONE tile, 15 LDS fragment reads per 14 MFMAs */        \
  X(11, 112x128_COL, 7, 1, 1, 8, 16, 0, 0)  /* 8 waves along N */                                                                                           \
  X(12, 64x128_COL, 4, 1, 1, 8, 16, 0, 0)   /* 8 waves along N */                                                                                           \
  X(13, 224x128, 7, 2, 2, 4, 16, 1, 1)      /* 8 waves as 2 x 4: 9 LDS fragment reads per 14 MFMAs (15 for cfg 10) */                                       \
  X(15, 192x128, 6, 2, 2, 4, 16, 1, 1)      /* 8 waves as 2 x 4 (the 190 antisymmetric pair rows of o = 20) */                                              \
  X(20, 128x32, 4, 1, 2, 2, 16, 0, 0)       /* 4 waves: tall products with N = n_occ (the t1 contractions of ovvv) */                                       \
  X(21, 32x128, 1, 4, 2, 2, 16, 0, 0)       /* 4 waves: the same with M = n_occ */                                                                          \
  X(33, 112x128, 7, 2, 1, 4, 16, 1, 1)      /* 4 waves, TWO workgroups per CU (66 KB of LDS each): short-K products */                                      \
  X(34, 128x224, 2, 7, 4, 2, 16, 1, 1)      /* 8 waves as 4 x 2 (2 x 7 MFMA tiles per wave): tall products with 192 < N <= 224 */                           \
  X(35, 160x128, 5, 2, 2, 4, 16, 1, 1)      /* 8 waves as 2 x 4: pair-row counts that 160 divides well (465 = npair(30)) */                                 \
  X(36, 80x128, 5, 2, 1, 4, 16, 1, 1)       /* 4 waves as 1 x 4, two workgroups per CU: the 66-80 packed pair rows of n_occ = 12 (mid-size fragments) */    \
  X(37, 96x96, 3, 3, 2, 2, 16, 1, 1)        /* 4 waves as 2 x 2: square products of 1000-2000 rows and columns (the rings of mid-size fragments) */         \
  X(38, 48x128, 3, 2, 1, 4, 16, 1, 0)       /* 4 waves as 1 x 4: the 36-45 packed pair rows of n_occ = 9 (the 80-row tile: 44 % of its MFMAs on padding) */
// X(id, tile): the same tile under a kernel symbol of its own (TAG 1), so that the pp-ladder shows as itself in profiles
#define QEMB_GEMM_LADDER_TWINS(X) X(23, 224x128) X(25, 192x128)

enum : int {
#define QEMB_X(id, name, wm, wn, waves_m, waves_n, bk, mode1, classic) GEMM_##name = id,
  QEMB_GEMM_TILES(QEMB_X)
#undef QEMB_X
  GEMM_CLASSIC = 200      // + id: the classic main loop of a MODE 1 tile
};

struct GemmTile { int wm, wn, waves_m, waves_n, bk, mode1; };
constexpr GemmTile gemm_tile(int cfg) {
  switch (cfg) {
#define QEMB_X(id, name, wm, wn, waves_m, waves_n, bk, mode1, classic) case id: return GemmTile{wm, wn, waves_m, waves_n, bk, mode1};
    QEMB_GEMM_TILES(QEMB_X)
#undef QEMB_X
    default: return GemmTile{0, 0, 0, 0, 0, 0};
  }
}
constexpr int gemm_tile_rows(int cfg) { return gemm_tile(cfg).wm * 16 * gemm_tile(cfg).waves_m; }
constexpr int gemm_tile_cols(int cfg) { return gemm_tile(cfg).wn * 16 * gemm_tile(cfg).waves_n; }
constexpr int64_t gemm_tile_count(int cfg, int64_t M, int64_t N) {
  return ((M + gemm_tile_rows(cfg) - 1) / gemm_tile_rows(cfg)) * ((N + gemm_tile_cols(cfg) - 1) / gemm_tile_cols(cfg));
}
// the id that runs `cfg` under the pp-ladder's kernel symbol (cfg itself where the tile has no such twin)
constexpr int gemm_tile_ladder_symbol(int cfg) {
  switch (cfg) {
#define QEMB_X(id, name) case GEMM_##name: return id;
    QEMB_GEMM_LADDER_TWINS(QEMB_X)
#undef QEMB_X
    default: return cfg;
  }
}
// the table itself, entry by entry in the order it is written (qemb_gemm_tile_table: tests and tools enumerate the tiles from here, not from a list of their own)
struct GemmTileEntry { int id, rows, cols, bk, mode1, has_classic, ladder_twin; };
constexpr int gemm_tile_entries() {
#define QEMB_X(id, name, wm, wn, waves_m, waves_n, bk, mode1, classic) +1
  return 0 QEMB_GEMM_TILES(QEMB_X);
#undef QEMB_X
}
inline bool gemm_tile_entry(int index, GemmTileEntry* e) {
  static const GemmTileEntry table[] = {
#define QEMB_X(id, name, wm, wn, waves_m, waves_n, bk, mode1, classic) \
    {id, gemm_tile_rows(id), gemm_tile_cols(id), bk, mode1, classic, gemm_tile_ladder_symbol(id) != id ? gemm_tile_ladder_symbol(id) : -1},
    QEMB_GEMM_TILES(QEMB_X)
#undef QEMB_X
  };
  if (index < 0 || index >= gemm_tile_entries()) return false;
  *e = table[index];
  return true;
}
// 193..224 rows (columns) fit ONE 224-row (224-column) tile: 1.8 % padding at n = 220 instead of the 14 % of two 128-wide tiles
constexpr bool fits_one_224_tile(int64_t n) { return n > gemm_tile_rows(GEMM_192x128) && n <= gemm_tile_rows(GEMM_224x128); }

}  // namespace qemb
