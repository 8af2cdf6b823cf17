// C entry points of the convolution family, host side only: argument validation (conv_validate), the kernel / tile choice (conv_choose;
// the tiles themselves are stated in conv_tiles.h) and the dispatch to the per-dtype translation units (conv_launch; kernels in
// conv_igemm.inc, conv3x3_direct.inc, pw_stream.hip).
#include "common.h"
#include "conv_params.h"
#include "conv_tiles.h"
#include "rowreduce.h"

// per (storage type, K-step width) translation units; two LDS stages (deeper pipelines never paid: residency beats prefetch depth -- re-checked in
// round 3 inside a dependent launch chain with 4 / 6 / 8 stages on 64x64, 128x64, 64x32 and 128x32 tiles: level on the 20x20 maps, 1.5 - 2.5x
// slower wherever the grid needs the residency; profiles/r03_chain_probe_deep_pipelines.txt).  conv_batch_<dtype>.hip: the batched kernels
// (implicit GEMM with 128-byte K-steps on the table's batched tiles, row-reuse direct 3x3 at 64 channels).
struct ConvUnit {
  int (*gemm[2])(const ConvP& p, int TC, int TP, hipStream_t s);      // [0] 64-byte, [1] 128-byte K-steps
  int (*direct3x3)(const ConvP& p, int TC, bool row_reuse, hipStream_t s);
  int (*batch)(const ConvBatchP& b, int n, const ConvChoice& c, hipStream_t s);
};
#define MTBT_DECL(dt)                                                                      \
  int mtbt_conv_dispatch_##dt##_wide(const ConvP& p, int TC, int TP, hipStream_t s);       \
  int mtbt_conv_dispatch_##dt##_narrow(const ConvP& p, int TC, int TP, hipStream_t s);     \
  int mtbt_conv3x3_direct_##dt(const ConvP& p, int TC, bool row_reuse, hipStream_t s);     \
  int mtbt_conv_batch_dispatch_##dt(const ConvBatchP& b, int n, const ConvChoice& c, hipStream_t s); \
  static const ConvUnit conv_unit_##dt = {{mtbt_conv_dispatch_##dt##_narrow, mtbt_conv_dispatch_##dt##_wide}, mtbt_conv3x3_direct_##dt, mtbt_conv_batch_dispatch_##dt};
MTBT_DECL(bf16)
MTBT_DECL(f32)
MTBT_DECL(f16)
#undef MTBT_DECL
static const ConvUnit& conv_unit(int dtype) { return dtype == MTBT_F32 ? conv_unit_f32 : (dtype == MTBT_F16 ? conv_unit_f16 : conv_unit_bf16); }
// pw_stream.hip: the heads' output 1x1 convolutions (few input channels, <= 64 outputs, fp32 strided store) without LDS
bool mtbt_pw_stream_applies(const ConvP& p, int dtype, bool any_width);
int mtbt_pw_stream(const ConvP& p, int dtype, hipStream_t s);
bool mtbt_pw_stream_batch_applies(const ConvP& p, int dtype);
int mtbt_pw_stream_batch(const ConvBatchP& b, int n, int dtype, hipStream_t s);

// Tile heuristics, from the sweep in tools/conv_tune.py on the shapes of the 640x640 batch-16 forward
// (numbers in DESIGN.md):
//   * channel tile = the divisor of K among 128 / 96 (else the smallest tile that covers K);
//   * 1x1 convolutions (streaming GEMMs, HBM-bound): a SMALL 128x64 / 96x128 / 64x128 tile with 64-byte K-steps
//     -> 32 KiB of LDS, three or more workgroups per CU hide the load / epilogue latency of the short K loop;
//   * k x k convolutions (MFMA-bound): 128-pixel tiles with 128-byte K-steps while that still gives >= 2
//     workgroups per CU, else 64x64 (small pyramid levels, 64-channel head convs).
static void pick_tile(int pol, int K, long M, int taps, int C, int es, int* TC, int* TP, int* narrow, bool no96 = false, int act = 0) {
  // pol (mtbt_conv_args.policy, a development A/B knob the host passes per call): bit0 = small 1x1 tiles, bit1 = 64x64 for small k x k
  int tc;
  if (K % 128 == 0) tc = 128;
  else if (K % 96 == 0 && !no96) tc = 96;
  else if (K > 96) tc = (no96 && K % 64 == 0) ? 64 : 128;
  else if (K > 64) tc = no96 ? 128 : 96;
  else if (K > 32) tc = 64;
  else tc = 32;
  const long ct = (K + tc - 1) / tc;
  if (taps == 1 && (pol & 1) && !no96 && K % 96 == 0 && tc == 128 && ((M + 127) / 128) * (K / 96) >= 3000) {
    // large 1x1 GEMMs whose width is a multiple of both: 96-channel tiles (batch-32 sweep, profiles/r02_j_conv_tune_1x1_batch32.txt: fc1 of
    // stages 0-2 3-9 % ahead of 128x128; level at batch 16)
    *TC = 96; *TP = 128; *narrow = (C * es <= 1536) ? 1 : 0;
    return;
  }
  if (taps == 1 && (pol & 1)) {
    // Round 3, re-measured IN A DEPENDENT CHAIN (tools/chain_tune.py, profiles/r03_chain_tune.txt: 32 launches in one captured graph, operands
    // out of the Infinity Cache as behind a producer).  The round-2 rules came from an eager same-buffer loop that is host-bound below ~15 us
    // and L2-warm, and had it backwards on the small maps:
    //   * 128-byte K-steps wherever the row allows (they never lose; 64-byte steps only for rows that are not a multiple of 128 bytes);
    //   * what decides the tile is the ROUND structure on the 512 workgroup slots (256 CUs x 2): 300 - 512 workgroups of the largest tile
    //     that gives that many -- one full round -- beat twice as many half tiles (256 -> 256 @40x40: 128x128 11.3 us, 128x64 14.3;
    //     512 -> 256 @40x40: 15.8 against 21.5) and 513 - 1023 is the worst place to be (a second, mostly empty round: 384 -> 384 @40x40);
    //   * 64-channel outputs (the heads' box convs): 64-pixel tiles at every level; narrower ones run on the streaming kernel (pw_stream.hip).
    const bool can_wide = (C * es) % 128 == 0;
    *narrow = can_wide ? 0 : 1;
    if (tc == 128) {
      const long g = ((M + 127) / 128) * ct, g2 = ((M + 63) / 64) * ct, g4 = ((M + 63) / 64) * ((K + 63) / 64);
      *TC = 128;
      if (g >= 1024) *TP = (act == MTBT_ACT_ELU && g < 4096) ? 64 : 128;      // (the ELU epilogue is long: BiFPN pointwise @80x80 49.9 against 58.7 us)
      else if (g >= 300 && g <= 512) *TP = 128;
      else if (g > 512 || (g2 >= 300 && g2 <= 512)) *TP = 64;
      else if (K % 64 == 0 && g4 <= 1024) { *TC = 64; *TP = 64; }
      else *TP = 64;
      return;
    }
    *TC = tc;
    if (tc <= 64) { *TP = 64; return; }
    *TP = 128;
    *narrow = (C * es <= 1536 || !can_wide) ? 1 : 0;
    return;
  }
  *narrow = 0;
  if (!(pol & 2) || taps == 1) {  // round-1 baseline: largest fitting channel tile, 128 pixels unless the grid is tiny
    *TC = tc;
    *TP = (((M + 127) / 128) * ct >= 512) ? 128 : 64;
    return;
  }
  if (K <= 64) { *TC = K > 32 ? 64 : 32; *TP = 64; return; }
  // (round-2 sweep, profiles/r02_f_conv_tune_3x3.txt: one 128-pixel tile per CU is already enough -- c2f_p4.m 3x3 192->192 @40: 40.3 -> 31.6 us)
  const long gk = ((M + 127) / 128) * ct;
  if (gk > 512 && gk < 1024 && tc == 128) { *TC = tc; *TP = 64; return; }   // (chain sweep: a second, mostly empty round of 128x128 tiles -- stage-2 downsample 38.1 -> 33.9 us)
  if (gk >= 256) { *TC = tc; *TP = 128; return; }
  if (((M + 63) / 64) * ct >= 256) { *TC = tc; *TP = 64; return; }
  *TC = (tc == 96) ? 96 : 64;
  *TP = 64;
  if (no96 && *TC == 96) *TC = 64;
}

extern "C" int64_t mtbt_conv_colsum_workspace_bytes(int64_t pixels, int K, int with_squares) {
  if (pixels <= 0 || K <= 0) return 0;
  return (pixels / 64 + 1) * 4 * (int64_t)K * (with_squares ? 2 : 1) * (int64_t)sizeof(float);   // <= 4 partial rows per 64 pixels
}

// second level of the column sums: `rows` partial rows -> colsum (one wave per channel, fixed order)
static int colsum_finish(const mtbt_conv_args* a, const ConvP& p, long rows, hipStream_t s) {
  if (rows <= 0 || rows > 0x7fffffffL) return MTBT_EINVAL;
  int pitch = p.cs_pitch;
  colsum_prereduce(p.cs_part, rows, pitch, 0, p.cs_pitch, s);       // (tall matrices: in place, see rowreduce.h)
  hipLaunchKernelGGL(channel_sum_final, dim3((unsigned)((a->K + 3) / 4)), dim3(256), 0, s, p.cs_part, (int)rows, pitch, 0, a->K, a->colsum, a->colsum_accumulate);
  if (a->colsum_sq)
    hipLaunchKernelGGL(channel_sum_final, dim3((unsigned)((a->K + 3) / 4)), dim3(256), 0, s, p.cs_part, (int)rows, pitch, a->K, a->K, a->colsum + a->K, a->colsum_accumulate);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}

// Step 1: every argument check, in a fixed order (the first fault of a block answers), and the kernel parameters.
static int conv_validate(const mtbt_conv_args* a, ConvP* pp) {
  if (!a || !a->x || !a->w || !a->y) return MTBT_EINVAL;
  if (a->dtype != MTBT_F32 && a->dtype != MTBT_BF16 && a->dtype != MTBT_F16) return MTBT_EINVAL;
  if (a->out_dtype != a->dtype && a->out_dtype != MTBT_F32) return MTBT_EINVAL;
  if (a->N <= 0 || a->H <= 0 || a->W <= 0 || a->C <= 0 || a->K <= 0 || a->R <= 0 || a->S <= 0 || a->stride <= 0 || a->pad < 0)
    return MTBT_EINVAL;
  const int es = a->dtype == MTBT_F32 ? 4 : 2;
  const int epc = 16 / es;
  if (a->C % (64 / es) != 0) return MTBT_EINVAL;
  if (a->Ho != (a->H + 2 * a->pad - a->R) / a->stride + 1 || a->Wo != (a->W + 2 * a->pad - a->S) / a->stride + 1) return MTBT_EINVAL;
  if (a->out_mode != MTBT_OUT_NHWC && a->out_mode != MTBT_OUT_CONVT2X2) return MTBT_EINVAL;
  if (a->out_mode == MTBT_OUT_CONVT2X2 && (a->K % 4 != 0)) return MTBT_EINVAL;
  if (a->act < 0 || a->act > MTBT_ACT_DGELU_POLY) return MTBT_EINVAL;
  if (a->act >= MTBT_ACT_DSILU && !a->res) return MTBT_EINVAL;  // the derivative epilogues read the pre-activation through res
  if (a->y2 && (a->out_mode != MTBT_OUT_NHWC || !aligned16(a->y2))) return MTBT_EINVAL;
  if (!aligned16(a->x) || !aligned16(a->w) || a->x_pixel_stride % epc != 0 || a->x_batch_stride % epc != 0) return MTBT_EALIGN;
  if (a->x_pixel_stride < a->C) return MTBT_EINVAL;

  ConvP& p = *pp;
  p.x = a->x; p.w = a->w; p.y = a->y; p.scale = a->scale; p.shift = a->shift; p.res = a->res; p.y2 = a->y2;
  p.xbs = a->x_batch_stride; p.ybs = a->y_batch_stride; p.rbs = a->res_batch_stride;
  p.ldx = a->x_pixel_stride; p.ldy = a->y_pixel_stride; p.ldr = a->res_pixel_stride;
  p.N = a->N; p.H = a->H; p.W = a->W; p.C = a->C; p.K = a->K; p.R = a->R; p.S = a->S;
  p.stride = a->stride; p.pad = a->pad; p.Ho = a->Ho; p.Wo = a->Wo;
  p.act = a->act; p.out_mode = a->out_mode; p.out_f32 = (a->out_dtype == MTBT_F32);
  if ((long)a->N * a->Ho * a->Wo > 0x7fffff00L) return MTBT_EINVAL;
  p.M = a->N * a->Ho * a->Wo;
  p.y_linear = (a->out_mode == MTBT_OUT_NHWC) && (a->y_batch_stride == (int64_t)a->Ho * a->Wo * a->y_pixel_stride) &&
               (!a->res || a->res_batch_stride == (int64_t)a->Ho * a->Wo * a->res_pixel_stride);
  p.ctiles = 0;
  p.ptiles_per_xcd = 0;
  p.debug = a->debug;
  // column sums (header): partial rows in the caller's workspace (cs_part set = asked for), second level after the conv
  p.cs_part = nullptr; p.cs_shift = a->colsum_shift; p.cs_sq = a->colsum_sq ? 1 : 0; p.cs_pitch = a->K * (a->colsum_sq ? 2 : 1);
  if (a->colsum && !a->colsum_ws) return MTBT_EINVAL;
  if (a->colsum_ws) {
    if (a->out_mode != MTBT_OUT_NHWC || !aligned16(a->colsum_ws)) return MTBT_EINVAL;
    p.cs_part = reinterpret_cast<float*>(a->colsum_ws);
  }
  // LDS-DMA addressing: 32-bit byte offsets below 2 GiB relative to (first image of a tile, weight tile row 0)
  if ((double)a->R * a->S > 31) return MTBT_EINVAL;
  if (((long)(128 / (a->Ho * a->Wo) + 2) * a->x_batch_stride + 2L * ((long)a->pad * a->W + a->pad) * a->x_pixel_stride) * es >= 0x7fff0000L) return MTBT_EINVAL;
  if ((long)128 * a->R * a->S * a->C * es >= 0x7fff0000L || (long)a->R * a->S * a->C * es >= 0x7fff0000L) return MTBT_EINVAL;
  // vector epilogue: a lane's 8 consecutive output channels must be whole aligned 16-byte accesses
  const int oes = p.out_f32 ? 4 : 2;
  const int kq = a->out_mode == MTBT_OUT_CONVT2X2 ? a->K / 4 : a->K;
  const int ovec = 16 / oes;  // elements per 16-byte store
  bool vec = (kq % 8 == 0 || a->out_mode == MTBT_OUT_NHWC) && (a->y_pixel_stride % ovec == 0) &&
             (a->y_batch_stride % ovec == 0) && aligned16(a->y);
  if (a->out_mode == MTBT_OUT_CONVT2X2) vec = vec && (kq % 8 == 0);
  if (a->res) vec = vec && (a->res_pixel_stride % epc == 0) && (a->res_batch_stride % epc == 0) && aligned16(a->res);
  p.vec_ok = vec ? 1 : 0;
  return MTBT_OK;
}

// Step 2: which kernel and tile a validated call runs and the column-sum partial layout it writes.  Pure: no stream, no launch.
// `nmem` > 0: the call is a member of a batch of nmem equal shapes -- the tile rules count the workgroups of the whole batch.
static int conv_choose(const mtbt_conv_args* a, const ConvP& p, int nmem, ConvChoice* c) {
  const int es = a->dtype == MTBT_F32 ? 4 : 2;
  const int pol = (a->policy & 0x100) ? (a->policy & 0xff) : 7;   // 0 = the default policy
  const bool want_cs = p.cs_part != nullptr;      // partial rows (and, with colsum, the finished sums)
  // narrow 1x1 convolutions into an fp32 map (the heads' output convs): streaming kernel, same arithmetic (a tile hint keeps the call on
  // the implicit-GEMM kernel: tests, A/B)
  if (!a->tile_hint && (pol & 64) == 0 && (long)a->K * a->C * es < 0x7fff0000L &&
      (nmem ? mtbt_pw_stream_batch_applies(p, a->dtype) : mtbt_pw_stream_applies(p, a->dtype, (pol & 128) != 0))) {
    *c = ConvChoice{CONV_PW_STREAM, a->K, 128, false, false, 0, 0};   // (no column sums on this path)
    return MTBT_OK;
  }
  // 3x3 / stride 1 / pad 1 on 16-aligned maps: direct convolution with an LDS-resident halo tile (conv3x3_direct.inc).
  // tile_hint bit 26 (or MTBT_CONV_POLICY bit 2 cleared) keeps such a conv on the implicit-GEMM kernel (tests, A/B).
  if ((pol & 4) && !((a->tile_hint >> 26) & 1) && !a->y2 && a->act < MTBT_ACT_DSILU && a->R == 3 && a->S == 3 && a->stride == 1 && a->pad == 1 && a->H % 16 == 0 &&
      a->W % 16 == 0 && a->out_mode == MTBT_OUT_NHWC && a->C % (128 / es) == 0 && a->K > 32 &&
      (long)a->H * a->W * a->x_pixel_stride * es < 0x7fff0000L && (long)128 * 9 * a->C * es < 0x7fff0000L) {
    // row-reuse variant (conv3x3_rr_kernel): the default (round 1: only for 64-channel tiles; after the epilogue split it is also
    // 9 % faster on the 128-channel C2f convs and 3 % on Proto -- MTBT_CONV_POLICY A/B, 7.20 -> 7.15 ms per step); policy bit 4
    // selects the first formulation, hint bit 25 / policy bit 3 force this one
    const bool rr = (pol & 8) || ((a->tile_hint >> 25) & 1) || !(pol & 16);
    const long rows = (long)a->N * (a->H >> 4) * (a->W >> 4) * (rr ? DIRECT_RR_CS_ROWS : DIRECT_CS_ROWS);
    *c = ConvChoice{CONV_DIRECT3X3, (a->K >= 96 && !(pol & 32)) ? 128 : 64, DIRECT_TP, false, rr, rows, p.cs_pitch};
    return MTBT_OK;
  }
  // tile_hint bits 28..30 once chose the LDS pipeline depth: accepted and ignored (every kernel has two stages)
  int TC = (a->tile_hint >> 16) & 0x1ff, TP = a->tile_hint & 0xffff;
  int narrow = (a->tile_hint >> 27) & 1;  // hint bit 27: force 64-byte K-steps
  if (!a->tile_hint || !TC || !TP) pick_tile(pol, a->K, nmem ? (long)p.M * nmem : (long)p.M, a->R * a->S, a->C, es, &TC, &TP, &narrow, want_cs, a->act);
  if (want_cs && TC == 96) return MTBT_EINVAL;   // (a wave's 48 / 96 channels are not a power-of-two number of 8-channel pieces)
  const int waves_p = conv_tile_waves_p(TC, TP);   // (a hinted tile outside the table: sized for 4 wave rows here, refused by conv_launch)
  *c = ConvChoice{CONV_IGEMM, TC, TP, a->C % (128 / es) == 0 && !narrow, false, (((long)p.M + TP - 1) / TP) * (waves_p ? waves_p : 4), p.cs_pitch};
  return MTBT_OK;
}

// Step 3: the workspace check, the launch and the second level of the column sums.
static int conv_launch(const mtbt_conv_args* a, const ConvP& p, const ConvChoice& c, hipStream_t s) {
  if (c.kind == CONV_PW_STREAM) return mtbt_pw_stream(p, a->dtype, s);
  if (p.cs_part && a->colsum_ws_bytes < c.cs_rows * c.cs_pitch * (int64_t)sizeof(float)) return MTBT_EWORKSPACE;
  const ConvUnit& u = conv_unit(a->dtype);
  const int rc = c.kind == CONV_DIRECT3X3 ? u.direct3x3(p, c.TC, c.row_reuse, s) : u.gemm[c.wide](p, c.TC, c.TP, s);
  if (rc != MTBT_OK || !a->colsum) return rc;
  return colsum_finish(a, p, c.cs_rows, s);
}

// validate + choose: what every entry point starts with
static int conv_plan(const mtbt_conv_args* a, int nmem, ConvP* p, ConvChoice* c) {
  if (const int rc = conv_validate(a, p)) return rc;
  return conv_choose(a, *p, nmem, c);
}

// the public choice[0..3] of a ConvChoice: [3] = 128-byte K-steps (implicit GEMM) / first formulation (direct) / 0 (streaming kernel)
static void conv_report(const ConvChoice& c, int32_t* choice) {
  choice[0] = c.kind; choice[1] = c.TC; choice[2] = c.TP;
  choice[3] = c.kind == CONV_IGEMM ? c.wide : (c.kind == CONV_DIRECT3X3 ? !c.row_reuse : 0);
}

extern "C" int mtbt_conv2d_nhwc(const mtbt_conv_args* a, void* stream) {
  ConvP p;
  ConvChoice c;
  if (const int rc = conv_plan(a, 0, &p, &c)) return rc;
  return conv_launch(a, p, c, reinterpret_cast<hipStream_t>(stream));
}

// The partial rows a call with these arguments writes into colsum_ws: rows x pitch floats, row r = [sum (K) | sum of squares (K, with
// colsum_sq)] of one (pixel tile, wave row); rows that cover no pixel hold zeros.  For a consumer that reduces them itself
// (mtbt_bn_forward_partials_nhwc) instead of asking for the finished sums.
extern "C" int mtbt_conv_colsum_layout(const mtbt_conv_args* a, int64_t* rows, int32_t* pitch) {
  if (!rows || !pitch || !a || !a->colsum_ws) return MTBT_EINVAL;
  ConvP p;
  ConvChoice c;
  if (const int rc = conv_plan(a, 0, &p, &c)) return rc;
  *rows = c.cs_rows; *pitch = c.cs_pitch;
  return MTBT_OK;
}

// Which kernel and tile a call with these arguments runs (nothing is launched, no pointer is dereferenced): choice[0] = 0 implicit GEMM,
// 1 direct 3x3 with an LDS-resident halo, 2 streaming head conv; [1] channel tile; [2] pixel tile (256 = the 16 x 16 halo tile; the
// streaming kernel: 128 pixels per workgroup); [3] = 128-byte K-steps (implicit GEMM) / first formulation (direct).  For tests of the tile
// rules (tests/test_cpu_host_logic.py) and for tools.
extern "C" int mtbt_conv_kernel_choice(const mtbt_conv_args* a, int32_t* choice) {
  if (!a || !choice) return MTBT_EINVAL;
  ConvP p;
  ConvChoice c;
  if (const int rc = conv_plan(a, 0, &p, &c)) return rc;
  conv_report(c, choice);
  return MTBT_OK;
}

// ---- batched form: n convolutions of one shape in one launch ---------------------------------------------------------------------------
// Validation and the ONE kernel choice of the batch: every member passes the single call's checks and choice (conv_validate, conv_choose with the
// batch's total workgroup count in the tile rules), the members agree in everything that selects or shapes the kernel, and the choice is
// one the batched kernels are instantiated for: implicit GEMM 64x64 / 128x128 / 128x64 / 32x64 with 128-byte K-steps, the row-reuse direct
// 3x3 at 64 channels (policy bit 5 asks for it from 96 output channels on), the streaming head conv up to 32 output channels.
static bool batch_same_shape(const mtbt_conv_args& a, const mtbt_conv_args& b) {
  return a.N == b.N && a.H == b.H && a.W == b.W && a.C == b.C && a.K == b.K && a.R == b.R && a.S == b.S && a.stride == b.stride && a.pad == b.pad &&
         a.Ho == b.Ho && a.Wo == b.Wo && a.dtype == b.dtype && a.out_dtype == b.out_dtype && a.act == b.act && a.out_mode == b.out_mode &&
         a.tile_hint == b.tile_hint && a.policy == b.policy && a.debug == b.debug && !a.scale == !b.scale && !a.shift == !b.shift && !a.res == !b.res;
}

// Output regions of two members (equal shapes): disjoint byte ranges, or channel slices of the same rows (equal pitch and batch stride, the
// batch stride a whole number of rows) that do not meet.
static bool batch_outputs_overlap(const mtbt_conv_args& a, const mtbt_conv_args& b) {
  const long oes = a.out_dtype == MTBT_F32 ? 4 : 2;
  const long ext_a = ((long)(a.N - 1) * a.y_batch_stride + ((long)a.Ho * a.Wo - 1) * a.y_pixel_stride + a.K) * oes;
  const long ext_b = ((long)(b.N - 1) * b.y_batch_stride + ((long)b.Ho * b.Wo - 1) * b.y_pixel_stride + b.K) * oes;
  const char* ya = reinterpret_cast<const char*>(a.y);
  const char* yb = reinterpret_cast<const char*>(b.y);
  if (ya + ext_a <= yb || yb + ext_b <= ya) return false;
  const long ld = a.y_pixel_stride;
  if (ld != b.y_pixel_stride || a.y_batch_stride != b.y_batch_stride || ld <= 0 || a.y_batch_stride % ld != 0) return true;
  const long db = yb - ya;
  if (db % oes != 0) return true;
  const long r = ((db / oes) % ld + ld) % ld;      // member b's first channel inside member a's rows
  return !(r >= a.K && r + a.K <= ld);
}


static int conv_batch_impl(const mtbt_conv_args* calls, int n, void* stream, int32_t* choice) {
  if (!calls || n < 1 || n > MTBT_CONV_BATCH_MAX) return MTBT_EINVAL;
  ConvBatchP b;
  ConvChoice c0;
  for (int i = 0; i < n; ++i) {
    const mtbt_conv_args& a = calls[i];
    if (a.y2 || a.colsum || a.colsum_ws || a.out_mode != MTBT_OUT_NHWC) return MTBT_EINVAL;     // training forms and the ConvT scatter: single calls only
    if (i && !batch_same_shape(calls[0], a)) return MTBT_EINVAL;
    ConvP p;
    ConvChoice c;
    if (const int rc = conv_plan(&a, n, &p, &c)) return rc;
    if (i == 0) { b.p = p; c0 = c; }
    else if (c.kind != c0.kind || c.TC != c0.TC || c.TP != c0.TP || c.wide != c0.wide || c.row_reuse != c0.row_reuse) return MTBT_EINVAL;
    ConvMember& m = b.m[i];
    m.x = p.x; m.w = p.w; m.y = p.y; m.scale = p.scale; m.shift = p.shift; m.res = p.res;
    m.xbs = p.xbs; m.ybs = p.ybs; m.rbs = p.rbs; m.ldx = p.ldx; m.ldy = p.ldy; m.ldr = p.ldr;
    m.vec_ok = p.vec_ok; m.y_linear = p.y_linear; m.pad_ = 0;
    for (int j = 0; j < i; ++j)
      if (batch_outputs_overlap(calls[j], a)) return MTBT_EINVAL;
  }
  for (int i = n; i < MTBT_CONV_BATCH_MAX; ++i) b.m[i] = b.m[0];
  if (c0.kind == CONV_IGEMM && !(c0.wide && conv_tile_batched(c0.TC, c0.TP))) return MTBT_EINVAL;
  if (c0.kind == CONV_DIRECT3X3 && !(c0.TC == 64 && c0.row_reuse)) return MTBT_EINVAL;
  if (choice) { conv_report(c0, choice); return MTBT_OK; }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (c0.kind == CONV_PW_STREAM) return mtbt_pw_stream_batch(b, n, calls[0].dtype, s);
  return conv_unit(calls[0].dtype).batch(b, n, c0, s);
}

extern "C" int mtbt_conv2d_nhwc_batch(const mtbt_conv_args* calls, int n, void* stream) { return conv_batch_impl(calls, n, stream, nullptr); }

extern "C" int mtbt_conv_batch_kernel_choice(const mtbt_conv_args* calls, int n, int32_t* choice) {
  if (!choice) return MTBT_EINVAL;
  return conv_batch_impl(calls, n, nullptr, choice);
}
