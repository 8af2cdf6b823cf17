// The tiles of the convolution kernels and the typed kernel choice (host only): the ONE statement of what the kernels are instantiated
// for.  The host chooser (conv_igemm.hip), dispatch_tile (conv_igemm.inc) and the batched units all expand this table.
#pragma once

// Implicit-GEMM tiles, X(TC, TP, WAVES_C, WAVES_P, batched): channels x pixels, the 4 waves arranged WAVES_C x WAVES_P over the tile
// (each wave's output row >= 128 B wherever the tile allows: full-line stores), batched = conv_batch_<dtype>.hip instantiates it too.
// A pixel tile writes WAVES_P column-sum partial rows.  To add a tile: one row.
// (Round 1 also built 256-pixel tiles, 3- and 4-deep pipelines and alternative wave layouts for the sweep in tools/conv_tune.py; none
// was ever the best choice, and with one epilogue body per activation they cost minutes of build time: removed.)
#define MTBT_CONV_TILES(X) \
  X(128, 128, 2, 2, true)  \
  X(96, 128, 1, 4, false)  \
  X(64, 128, 1, 4, false)  \
  X(32, 128, 1, 4, false)  \
  X(128, 64, 2, 2, true)   \
  X(96, 64, 2, 2, false)   \
  X(64, 64, 1, 4, true)    \
  X(32, 64, 1, 4, true)

// wave rows of a tile = column-sum partial rows per pixel tile; 0: no such tile
inline int conv_tile_waves_p(int TC, int TP) {
#define MTBT_X(tc, tp, wc, wp, b) if (TC == tc && TP == tp) return wp;
  MTBT_CONV_TILES(MTBT_X)
#undef MTBT_X
  return 0;
}

inline bool conv_tile_batched(int TC, int TP) {
#define MTBT_X(tc, tp, wc, wp, b) if (TC == tc && TP == tp) return b;
  MTBT_CONV_TILES(MTBT_X)
#undef MTBT_X
  return false;
}

// Direct 3x3 kernels (conv3x3_direct.inc): column-sum partial rows per 16 x 16 tile.  First formulation: each of the 4 waves owns four
// tile rows; row-reuse: a wave's row half (the channel halves write disjoint columns).
constexpr int DIRECT_CS_ROWS = 4, DIRECT_RR_CS_ROWS = 2;
constexpr int DIRECT_TP = 256;   // the pixel tile mtbt_conv_kernel_choice reports for them

enum ConvKind { CONV_IGEMM = 0, CONV_DIRECT3X3 = 1, CONV_PW_STREAM = 2 };   // the public choice[0] values

// What conv_choose decides for one call (or one batch): the kernel, its tile and the column-sum partial layout it writes.
struct ConvChoice {
  ConvKind kind;
  int TC, TP;        // channel / pixel tile (direct: TP = DIRECT_TP; streaming kernel: K, 128 pixels per workgroup)
  bool wide;         // implicit GEMM: 128-byte K-steps
  bool row_reuse;    // direct 3x3: the row-reuse formulation
  long cs_rows;      // partial rows x floats per row in colsum_ws (streaming kernel: none)
  int cs_pitch;
};
