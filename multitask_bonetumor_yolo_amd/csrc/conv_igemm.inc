// Implicit-GEMM convolution on gfx950 MFMA, NHWC activations, KRSC weights.
//
//   D[k][p] = sum_{r,s,c} W[k][r][s][c] * X[n(p), oy(p)*st - pad + r, ox(p)*st - pad + s, c]
//
// GEMM view: rows = output channels (MFMA "A" operand = weights), columns = output pixels
// (MFMA "B" operand = gathered input), reduction = (r,s,c) in KRSC order.  With this orientation the
// 16x16 accumulator of one MFMA holds, per lane, FOUR CONSECUTIVE OUTPUT CHANNELS of one pixel
// (row = 4*(lane>>4)+reg, col = lane&15), i.e. an 8-byte (bf16) / 16-byte (f32) contiguous piece of
// the NHWC output, so the epilogue stores vector pieces straight from the accumulator.
//
// Workgroup: 256 threads = 4 waves arranged WAVES_C x WAVES_P over a TC x TP (channels x pixels)
// tile.  Per K-step both operand tiles (TC and TP rows of BKB bytes) go global -> LDS by LDS-DMA
// (global_load_lds_dwordx4; the im2col gather is just a per-lane SOURCE address, padding reads a zero
// constant), double-buffered in LDS with ONE barrier per step: the DMA of step t+1 is issued before the
// MFMAs of step t.  LDS rows are XOR-swizzled (on the DMA source side, LDS destination is lane-linear)
// so that the ds_read_b128 fragment reads are bank-conflict-free (checked against the gfx950 lane-group rule).
//
// bf16: v_mfma_f32_16x16x32_bf16 (one 16-B chunk = 8 k per lane).  f32: v_mfma_f32_16x16x4_f32, the
// exact-fp32 parity path; a lane's 16-B chunk holds 4 consecutive k which feed 4 MFMAs (the k order
// inside the reduction is permuted identically for both operands).
#pragma once
#include "common.h"
#include "conv_params.h"
#include "conv_tiles.h"
#include "conv_dma.h"
#include "conv_epilogue.h"

namespace {


template <int CPR> __device__ __forceinline__ int swz(int row) {
  if constexpr (CPR == 4) return (-(row >> 2)) & 3;   // 64-B rows
  else return (row >> 1) & 7;                         // 128-B rows
}

template <typename T, int TC, int TP, int WAVES_C, int WAVES_P, int BKB, int NBUF>
__global__ __launch_bounds__(256, 2) void conv_igemm_kernel(const ConvP p) {
  const unsigned bid = blockIdx.x;
#include "conv_igemm_body.inc"
}

#ifdef MTBT_CONV_BATCH_UNIT
// Batched form: grid = (blocks of one member, members).  Every member's block range is the single call's padded grid (a multiple of 8),
// and x is the fastest grid dimension, so a member's pixel tiles meet the XCDs as they do in a call of its own.
template <typename T, int TC, int TP, int WAVES_C, int WAVES_P, int BKB, int NBUF>
__global__ __launch_bounds__(256, 2) void conv_igemm_batch_kernel(const ConvBatchP b) {
  const ConvP p = conv_member(b, (int)blockIdx.y);
  const unsigned bid = blockIdx.x;
#include "conv_igemm_body.inc"
}
#endif

// One call (q a ConvP, n = 1) or one batch (q a ConvBatchP) of `kernel` on TC x TP tiles: the grid and the LDS bytes.
template <int TC, int TP, int WAVES_C, int BKB, int NBUF, typename Kernel, typename Params>
int launch_tile(Kernel kernel, Params q, int n, hipStream_t stream) {
  constexpr int CPR = BKB / 16;
  constexpr int TCS = ((TC * CPR + 255) / 256) * 256 / CPR;
  constexpr int lds_main = NBUF * (TCS + TP) * BKB;
  constexpr int lds_epi = 2 * 4 * 16 * ((TC / WAVES_C) * 4 + 16);
  constexpr int lds = (lds_main > lds_epi ? lds_main : lds_epi) + 2 * TC * 4;
  static_assert(lds <= 160 * 1024, "this (tile, depth) does not fit the CU's 160 KiB of LDS");
  return conv_launch_tiles(kernel, q, TC, ((long)conv_of(q).M + TP - 1) / TP, n, lds, stream);
}

// every tile of the table (conv_tiles.h)
template <typename T, int BKB, int NBUF>
int dispatch_tile(const ConvP& p, int TC, int TP, hipStream_t s) {
#define MTBT_X(tc, tp, wc, wp, batched) \
  if (TC == tc && TP == tp) return launch_tile<tc, tp, wc, BKB, NBUF>(conv_igemm_kernel<T, tc, tp, wc, wp, BKB, NBUF>, p, 1, s);
  MTBT_CONV_TILES(MTBT_X)
#undef MTBT_X
  return MTBT_EINVAL;
}

#ifdef MTBT_CONV_BATCH_UNIT
// the table's batched tiles, with 128-byte K-steps
template <typename T>
int dispatch_tile_batch(const ConvBatchP& b, int n, int TC, int TP, hipStream_t s) {
#define MTBT_X(tc, tp, wc, wp, batched) \
  if constexpr (batched) { if (TC == tc && TP == tp) return launch_tile<tc, tp, wc, 128, 2>(conv_igemm_batch_kernel<T, tc, tp, wc, wp, 128, 2>, b, n, s); }
  MTBT_CONV_TILES(MTBT_X)
#undef MTBT_X
  return MTBT_EINVAL;
}
#endif

}  // namespace
