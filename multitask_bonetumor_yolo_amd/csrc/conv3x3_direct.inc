#ifndef MTBT_RR_RESPF
#define MTBT_RR_RESPF 2   // residual pieces requested ONE slab ahead (conv_epilogue.h): the whole tile's (mode 1) spills 57 / 33 registers in the
#endif                   // 128-channel kernels, which sit at 256; mode 2 costs ITER x 4
// Direct 3x3 convolution (stride 1, pad 1) on gfx950 MFMA with an LDS-RESIDENT INPUT HALO TILE.
//
// Why: in the implicit-GEMM kernel every (tap, channel-chunk) step refills BOTH operand tiles, and the measured
// limiter is not the MFMA pipe but the CU's 64 B/clk fill path (L1 -> LDS-DMA) plus the LDS port time those fills
// and the fragment reads share: a 128x128 tile is 64 FLOP per filled byte, exactly the machine balance
// (4096 FLOP/clk/CU / 64 B/clk).  A 3x3 conv re-reads each input pixel for 9 taps, so here the workgroup stages
// the (16+2)x(16+2) pixel halo of its 16x16 output tile ONCE per 64-channel chunk and the nine taps are served
// from it by shifted LDS addresses (im2col by address arithmetic, all precomputed).  Per chunk the fill is
// 41 KB (halo) + 9 x 16 KB (weights) for 37.7 MFLOP: ~200 FLOP/B, 3x the balance point.
//
//   GEMM view as in conv_igemm.inc: rows = output channels (MFMA A = weights), columns = pixels (MFMA B).
//   workgroup = 4 waves, TC output channels x 256 pixels; wave w owns tile rows 4w..4w+3 (one MFMA column
//   block = the 16 pixels of one tile row), FC = TC/16 channel fragments x 4 pixel fragments.
//   LDS: halo [324 px][128 B] (chunk slot XOR (pixel & 7): conflict-free b128 reads from ANY 16 consecutive
//   pixels), weight tap tile [TC][128 B] double-buffered; both filled by LDS-DMA with constant per-lane offsets.
//   Schedule per channel chunk: barrier, DMA halo + tap 0; per tap: vmcnt(0), barrier, DMA next tap, 2 x
//   (FC + 4 fragment reads, FC x 4 MFMAs).  Epilogue: the slab scheme of conv_igemm.inc (fp32 through LDS,
//   16-byte coalesced stores, fused scale / shift / activation / residual).
#pragma once
#include "common.h"
#include "conv_dma.h"
#include "conv_epilogue.h"
#include "conv_params.h"
#include "conv_tiles.h"

namespace {

template <typename T, int TC>
__global__ __launch_bounds__(256, 2) void conv3x3_direct_kernel(const ConvP p) {
  constexpr int ES = (int)sizeof(T), EPC = 16 / ES, BKB = 128, BKE = BKB / ES;
  constexpr int HWID = 18, NHP = HWID * HWID;                 // halo edge, halo pixels
  constexpr int FC = TC / 16, FP = 4;
  constexpr int XDMA = (NHP * 8 + 255) / 256;                  // halo DMA instructions per wave (11)
  constexpr int XBYTES = XDMA * 256 * 16;                      // halo region incl. the zero-filled DMA tail
  constexpr int WDMA = TC * 8 / 256;                           // weight-tap DMA instructions per wave
  constexpr int WBYTES = TC * BKB;
  constexpr unsigned OOB = 0x80000000u;
  static_assert(TC % 32 == 0 && WDMA * 256 == TC * 8, "weight tile = whole wave-instructions");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* aff = reinterpret_cast<float*>(smem + XBYTES + 2 * WBYTES);  // scale/shift copy (epilogue slabs fit below it)
  static_assert(4 * 16 * (TC * 4 + 16) <= XBYTES + 2 * WBYTES, "epilogue slabs below the affine copy");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lq = lane >> 4;

  // tile decode (XCD-contiguous ranges of spatial tiles, channel tiles of one spatial tile adjacent)
  const int slot = blockIdx.x >> 3, xcd = blockIdx.x & 7;
  const int ctile = slot % p.ctiles;
  const int ptile = xcd * p.ptiles_per_xcd + slot / p.ctiles;
  const int tiles_x = p.W >> 4, tpi = tiles_x * (p.H >> 4);
  if (ptile >= p.N * tpi) return;
  const int n = ptile / tpi, trem = ptile - n * tpi;
  const int ty0 = (trem / tiles_x) << 4, tx0 = (trem % tiles_x) << 4;
  const int cbase = ctile * TC;
  const int Kdim = 9 * p.C;
  stage_affine<TC>(p, aff, cbase, tid);

  const srd_t xsrd = make_srd(reinterpret_cast<const T*>(p.x) + (long)n * p.xbs);
  const srd_t wsrd = make_srd(reinterpret_cast<const T*>(p.w) + (long)cbase * Kdim);
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;

  // constant per-lane DMA offsets
  unsigned xvoff[XDMA];
#pragma unroll
  for (int i = 0; i < XDMA; ++i) {
    const int c = i * 256 + tid;
    const int hp = c >> 3, sl = c & 7;
    const int hy = hp / HWID, hx = hp - hy * HWID;
    const int iy = ty0 - 1 + hy, ix = tx0 - 1 + hx;
    const bool ok = hp < NHP && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
    xvoff[i] = ok ? (unsigned)((((long)iy * p.W + ix) * p.ldx + (sl ^ (hp & 7)) * EPC) * ES) : OOB;
  }
  unsigned wvoff[WDMA];
#pragma unroll
  for (int i = 0; i < WDMA; ++i) {
    const int c = i * 256 + tid;
    const int row = c >> 3, sl = c & 7;
    const int srow = epi_row_channel(row);          // staged row order of conv_epilogue.h PERM (all four waves share the TC weight rows)
    wvoff[i] = (cbase + srow < p.K) ? (unsigned)(((long)srow * Kdim + (sl ^ ((row >> 1) & 7)) * EPC) * ES) : OOB;
  }

  // fragment read addresses (bytes from smem): B for (tile row 4w + rr, tap column s, K sub-step), A base per sub-step
  int baddr[6][3][2];
#pragma unroll
  for (int rr = 0; rr < 6; ++rr)
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int hp = (4 * wave + rr) * HWID + lr + s;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) baddr[rr][s][ks] = hp * BKB + (((ks * 4 + lq) ^ (hp & 7)) << 4);
    }
  int abase[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) abase[ks] = XBYTES + lr * BKB + (((ks * 4 + lq) ^ ((lr >> 1) & 7)) << 4);

  f32x4 acc[FC][FP];
#pragma unroll
  for (int i = 0; i < FC; ++i)
#pragma unroll
    for (int j = 0; j < FP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nchunks = p.C / BKE;
  for (int cc = 0; cc < nchunks; ++cc) {
    lds_barrier();  // every wave is done with the previous chunk's halo and tap buffers
    const int csoff = cc * BKB;
#pragma unroll
    for (int i = 0; i < XDMA; ++i) lds_dma16(xsrd, xvoff[i], csoff, lds0 + (i * 256 + wave * 64) * 16);
#pragma unroll
    for (int i = 0; i < WDMA; ++i) lds_dma16(wsrd, wvoff[i], csoff, lds0 + XBYTES + (i * 256 + wave * 64) * 16);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      wait_vm<0>();
      lds_barrier();
      if (tap < 8) {
        const int wsoff = ((tap + 1) * p.C) * ES + csoff;
#pragma unroll
        for (int i = 0; i < WDMA; ++i)
          lds_dma16(wsrd, wvoff[i], wsoff, lds0 + XBYTES + ((tap + 1) & 1) * WBYTES + (i * 256 + wave * 64) * 16);
      }
      const int r = tap / 3, s = tap - 3 * r;  // compile-time (tap loop is unrolled)
      const char* wb = smem + (tap & 1) * WBYTES;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        uint4 a[FC], b[FP];
#pragma unroll
        for (int f = 0; f < FC; ++f) a[f] = *reinterpret_cast<const uint4*>(wb + abase[ks] + f * 16 * BKB);
#pragma unroll
        for (int j = 0; j < FP; ++j) b[j] = *reinterpret_cast<const uint4*>(smem + baddr[j + r][s][ks]);
#pragma unroll
        for (int i = 0; i < FC; ++i)
#pragma unroll
          for (int j = 0; j < FP; ++j) {
            if constexpr (sizeof(T) == 2) {
              acc[i][j] = mfma_16x16x32<T>(a[i], b[j], acc[i][j]);
            } else {
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[i].x), __uint_as_float(b[j].x), acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[i].y), __uint_as_float(b[j].y), acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[i].z), __uint_as_float(b[j].z), acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[i].w), __uint_as_float(b[j].w), acc[i][j], 0, 0, 0);
            }
          }
      }
    }
  }
  __syncthreads();  // LDS is free for the epilogue slabs

  // ---- epilogue (conv_epilogue.h): one slab = the 16 pixels of one tile row x TC channels ----
  const EpiSeq seq{(long)(ty0 + 4 * wave) * p.W + tx0, p.W, 0x7fffffffffffffffL, (long)n * p.ybs, (long)n * p.rbs};   // slab j = tile row j
  conv_epilogue<T, TC, FC, FP, false, MTBT_RR_RESPF, false, true>(p, acc, smem + wave * (16 * (TC * 4 + 16)), aff, cbase, 0, lane,
                               [&](int j, int row, int ch, long& yoff, long& roff) -> bool {
    const long pixoff = (long)(ty0 + 4 * wave + j) * p.W + tx0 + row;
    yoff = (long)n * p.ybs + pixoff * p.ldy + ch;
    roff = (long)n * p.rbs + pixoff * p.ldr + ch;
    return true;
  }, seq, true, (long)ptile * DIRECT_CS_ROWS + wave);     // column-sum partial rows: 4 per tile (each wave owns four tile rows)
}

template <typename T, int TC>
int launch_direct3x3(ConvP q, hipStream_t stream) {
  constexpr int XBYTES = ((324 * 8 + 255) / 256) * 256 * 16;
  constexpr int lds_main = XBYTES + 2 * TC * 128;
  constexpr int lds_epi = 4 * 16 * (TC * 4 + 16);
  constexpr int lds = (lds_main > lds_epi ? lds_main : lds_epi) + 2 * TC * 4;
  return conv_launch_tiles(conv3x3_direct_kernel<T, TC>, q, TC, (long)q.N * (q.H >> 4) * (q.W >> 4), 1, lds, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Row-reuse variant.  The kernel above is bound by LDS port time: per (tap, 32-channel step) a wave reads FC weight and 4
// input fragments for FC x 4 MFMAs, and the 4 waves re-read the same weights (SQ counters: MFMA busy 52 %).  Here
//   * waves tile the workgroup 2 (channel halves) x 2 (row halves): a wave owns TC/2 channels x 8 tile rows (FP = 8);
//   * the reduction is walked in steps of ONE 32-channel (64-byte) slab and, inside it, per filter COLUMN s: the 10 input
//     row fragments (tile rows 8 wr .. 8 wr + 9, shifted by s) are read ONCE and serve the three taps (0..2, s), because
//     output row y with filter row r reads input row y + r;
//   * so a column step is 10 + 3 x FC fragment reads for 3 x FC x 8 MFMAs (FC = 4: 22 reads / 96 MFMAs, against 36 / 96);
//   * LDS: halo [324 px][64 B] (slot XOR (pixel >> 2) & 3: conflict-free for any 16 consecutive pixels), weights of one
//     filter column = 3 tap tiles [TC][64 B], double-buffered; 69 KiB at TC = 128 -> two workgroups per CU as before.
//     The next column's weights are requested at the top of a step, the next slab's halo as soon as every wave holds the
//     last column's input fragments in registers.
template <typename T, int TC>
__global__ __launch_bounds__(256, 2) void conv3x3_rr_kernel(const ConvP p) {
  const unsigned bid = blockIdx.x;
#include "conv3x3_rr_body.inc"
}

#ifdef MTBT_CONV_BATCH_UNIT
// Batched form (conv_params.h): grid = (blocks of one member, members), the member's blocks ordered as in a call of its own.
template <typename T, int TC>
__global__ __launch_bounds__(256, 2) void conv3x3_rr_batch_kernel(const ConvBatchP b) {
  const ConvP p = conv_member(b, (int)blockIdx.y);
  const unsigned bid = blockIdx.x;
#include "conv3x3_rr_body.inc"
}
#endif

// One call (q a ConvP, n = 1) or one batch (q a ConvBatchP) of a row-reuse kernel: one workgroup per (16 x 16 tile, TC channels); LDS =
// halo [324 px][64 B] incl. the zero-filled DMA tail, 2 x 3 weight tap tiles, the affine copy.
template <int TC, typename Kernel, typename Params>
int launch_direct3x3_rr(Kernel kernel, Params q, int n, hipStream_t stream) {
  constexpr int XBYTES = ((324 * 4 + 255) / 256) * 256 * 16;
  constexpr int lds = XBYTES + 2 * 3 * TC * 64 + 2 * TC * 4;
  const ConvP& p = conv_of(q);
  return conv_launch_tiles(kernel, q, TC, (long)p.N * (p.H >> 4) * (p.W >> 4), n, lds, stream);
}

// both formulations at 128- and 64-channel tiles
template <typename T>
int dispatch_direct3x3(const ConvP& p, int TC, bool row_reuse, hipStream_t s) {
  if (row_reuse && TC == 128) return launch_direct3x3_rr<128>(conv3x3_rr_kernel<T, 128>, p, 1, s);
  if (row_reuse && TC == 64) return launch_direct3x3_rr<64>(conv3x3_rr_kernel<T, 64>, p, 1, s);
  if (TC == 128) return launch_direct3x3<T, 128>(p, s);
  if (TC == 64) return launch_direct3x3<T, 64>(p, s);
  return MTBT_EINVAL;
}

}  // namespace
