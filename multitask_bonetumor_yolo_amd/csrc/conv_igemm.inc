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

template <typename T, int TC, int TP, int WAVES_C, int WAVES_P, int BKB, int NBUF>
int launch_batch(const ConvBatchP& b, int n, hipStream_t stream) {
  ConvBatchP q = b;
  q.p.ctiles = (b.p.K + TC - 1) / TC;
  const long ptiles = ((long)b.p.M + TP - 1) / TP;
  q.p.ptiles_per_xcd = (int)((ptiles + 7) / 8);
  const long blocks = (long)q.p.ptiles_per_xcd * 8 * q.p.ctiles;
  if (blocks <= 0 || blocks > 0x7fffffffL || n < 1 || n > MTBT_CONV_BATCH_MAX) return MTBT_EINVAL;
  constexpr int CPR = BKB / 16;
  constexpr int TCS = ((TC * CPR + 255) / 256) * 256 / CPR;
  constexpr int lds_main = NBUF * (TCS + TP) * BKB;
  constexpr int lds_epi = 2 * 4 * 16 * ((TC / WAVES_C) * 4 + 16);
  constexpr int lds = (lds_main > lds_epi ? lds_main : lds_epi) + 2 * TC * 4;
  static_assert(lds <= 160 * 1024, "LDS");
  if (int rc = mtbt_allow_lds(conv_igemm_batch_kernel<T, TC, TP, WAVES_C, WAVES_P, BKB, NBUF>, lds)) return rc;
  hipLaunchKernelGGL((conv_igemm_batch_kernel<T, TC, TP, WAVES_C, WAVES_P, BKB, NBUF>), dim3((unsigned)blocks, (unsigned)n), dim3(256), lds, stream, q);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}
#endif

template <typename T, int TC, int TP, int WAVES_C, int WAVES_P, int BKB, int NBUF>
int launch(const ConvP& p, hipStream_t stream) {
  ConvP q = p;
  q.ctiles = (p.K + TC - 1) / TC;
  const long ptiles = ((long)p.M + TP - 1) / TP;
  q.ptiles_per_xcd = (int)((ptiles + 7) / 8);
  const long blocks = (long)q.ptiles_per_xcd * 8 * q.ctiles;
  if (blocks <= 0 || blocks > 0x7fffffffL) return MTBT_EINVAL;
  constexpr int CPR = BKB / 16;
  constexpr int TCS = ((TC * CPR + 255) / 256) * 256 / CPR;
  constexpr int lds_main = NBUF * (TCS + TP) * BKB;
  constexpr int lds_epi = 2 * 4 * 16 * ((TC / WAVES_C) * 4 + 16);
  constexpr int lds = (lds_main > lds_epi ? lds_main : lds_epi) + 2 * TC * 4;
  if constexpr (lds > 160 * 1024) {
    return MTBT_EINVAL;  // this (tile, depth) does not fit the CU's 160 KiB of LDS
  } else {
  if (int rc = mtbt_allow_lds(conv_igemm_kernel<T, TC, TP, WAVES_C, WAVES_P, BKB, NBUF>, lds)) return rc;
  hipLaunchKernelGGL((conv_igemm_kernel<T, TC, TP, WAVES_C, WAVES_P, BKB, NBUF>), dim3((unsigned)blocks), dim3(256), lds, stream, q);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
  }
}

template <typename T, int BKB, int NBUF>
int dispatch_tile(const ConvP& p, int TC, int TP, hipStream_t s) {
  // wave layouts keep each wave's output row >= 128 B (64 bf16 channels) wherever the tile allows: full-line stores.
  // (Round 1 also built 256-pixel tiles, 3- and 4-deep pipelines and alternative wave layouts for the sweep in tools/conv_tune.py; none
  // was ever the best choice, and with one epilogue body per activation they cost minutes of build time: removed.)
  if (TP == 128) {
    if (TC == 128) return launch<T, 128, 128, 2, 2, BKB, NBUF>(p, s);
    if (TC == 96) return launch<T, 96, 128, 1, 4, BKB, NBUF>(p, s);
    if (TC == 64) return launch<T, 64, 128, 1, 4, BKB, NBUF>(p, s);
    if (TC == 32) return launch<T, 32, 128, 1, 4, BKB, NBUF>(p, s);
  } else if (TP == 64) {
    if (TC == 128) return launch<T, 128, 64, 2, 2, BKB, NBUF>(p, s);
    if (TC == 96) return launch<T, 96, 64, 2, 2, BKB, NBUF>(p, s);
    if (TC == 64) return launch<T, 64, 64, 1, 4, BKB, NBUF>(p, s);
    if (TC == 32) return launch<T, 32, 64, 1, 4, BKB, NBUF>(p, s);
  }
  return MTBT_EINVAL;
}

}  // namespace
