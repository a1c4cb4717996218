// Launch geometry of the four GEMM families (gemm.hip, gemm_dma.hip, gemm_split_dispatch.hpp, gemm_planes.hip): the L2-blocked
// tile order and the split-K ranges.  Host only, plain integers in and out: the dispatchers keep none of this arithmetic, and
// tests/test_gemm_geometry_host.py pins it without a GPU (through the two debug exports at the end of gemm.hip).
#pragma once
#include <stdint.h>

namespace mt {

struct TileGrid { int m_tiles, n_tiles, grid_x, group_n; };

// Tiles of bm x bn over an M x N output.  Tall problems (>= 32 row tiles, >= 2 column tiles) walk their tiles in column groups
// (group_n > 0; gemm_core.hpp tile_of): a group's operand panels, `panel_bytes` per column tile, take ~2 MB of an XCD's 4 MB L2,
// and grid_x is padded to 8 (XCDs) x whole rows of tiles.  group_n == 0: plain order, one block per tile.
inline TileGrid tile_grid(int M, int N, int bm, int bn, int64_t panel_bytes) {
  TileGrid g{(M + bm - 1) / bm, (N + bn - 1) / bn, 0, 0};
  g.grid_x = g.m_tiles * g.n_tiles;
  if (g.m_tiles >= 32 && g.n_tiles >= 2) {
    const int64_t gn = (2 << 20) / (panel_bytes > 0 ? panel_bytes : 1);
    g.group_n = gn < 1 ? 1 : (gn > g.n_tiles ? g.n_tiles : (int)gn);
    g.grid_x = 8 * ((g.m_tiles + 7) / 8) * g.n_tiles;
  }
  return g;
}

// K_XCD: K-range-major over the XCDs (gemm_split.hpp): a multiple of 8 ranges, one block per tile and range -- the caller sets
// group_n = 0 and grid.x = tiles.  K_XCD_CAPPED also keeps >= 256 contraction rows per range (needs K >= 2048).
enum KForm { K_PLAIN = 0, K_XCD = 1, K_XCD_CAPPED = 2 };

struct SplitK { int k_chunk, ranges, grid_y, xcd_k; };     // ranges = the non-empty ones (det_gemm_setup's count); grid_y >= ranges

// K ranges of a split-K launch.  split_k > 0 is the caller's count; otherwise auto_target > 0 asks for about that many blocks over
// `tiles` output tiles, at >= 256 contraction rows each (the fp32 atomics of the epilogue stay a small fraction of the work), and
// auto_target == 0 means one range.  k_chunk is a multiple of k_round (the K step of the loop that runs it; 16 for the K_XCD forms).
inline SplitK split_k_ranges(int K, int tiles, int split_k, int auto_target, int k_round, KForm form) {
  int splits = split_k;
  if (splits <= 0 && auto_target > 0) {
    splits = (auto_target + tiles - 1) / tiles;
    const int max_splits = K / 256 > 0 ? K / 256 : 1;
    if (splits > max_splits) splits = max_splits;
  }
  if (splits < 1) splits = 1;
  if (form != K_PLAIN) {
    splits = (splits + 4) / 8 * 8;
    if (form == K_XCD_CAPPED && splits > (K / 256) / 8 * 8) splits = (K / 256) / 8 * 8;
    if (splits < 8) splits = 8;
    k_round = 16;
  }
  SplitK r;
  r.k_chunk = ((K + splits - 1) / splits + k_round - 1) / k_round * k_round;
  r.ranges = (K + r.k_chunk - 1) / r.k_chunk;
  r.grid_y = form == K_PLAIN ? r.ranges : (r.ranges + 7) / 8 * 8;      // no K range beyond the last non-empty group of 8
  r.xcd_k = form != K_PLAIN;
  return r;
}

}  // namespace mt
