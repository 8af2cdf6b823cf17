// Depthwise KS x KS convolution (stride 1, pad KS/2), NHWC, fp32 arithmetic on the VALU.
//
// Depthwise has no cross-channel reduction, so there is no MFMA shape for it; the roof is the packed
// fp32 FMA rate (v_pk_fma_f32).  What the first versions of this kernel ran into instead was the
// vector-memory ISSUE rate: a 4-byte-per-lane global load costs the CU's address unit as much as a
// 16-byte one, and a 7x7 window needs ~7 input vectors per output pixel.  So:
//
//   * a workgroup owns a TH x TW output tile and walks the channels in chunks of CC = 128;
//   * per chunk the (TH+KS-1) x (TW+KS-1) input halo tile and the chunk's KS*KS taps are staged in LDS
//     with 16-byte global loads (the only global reads), 256 B (bf16) per pixel;
//   * wave w owns the 2 x 8 output sub-tile w; lane l owns channel pair (2l, 2l+1) of the chunk: every
//     LDS read is a conflict-free 4-byte (bf16x2) / 8-byte (f32x2) access, every FMA a packed pair;
//     a sub-tile row of 8+KS-1 inputs is read once and feeds both output rows and all KS horizontal taps;
//   * all chunks' accumulators stay in registers; the LayerNorm statistics (ConvNeXt conv_dw + norm)
//     are per-thread partial sums + one LDS transpose-reduce per wave (a wave holds ALL channels of its
//     16 pixels), two-pass mean/variance, then the normalised pairs are stored straight from registers.
#include "common.h"
#include "conv_dma.h"
#include "dwconv_args.h"

namespace {

// A channel pair as a 2-vector: `fma2` on it is ONE v_pk_fma_f32 (left as separate .x/.y fmaf calls the SLP
// vectoriser pairs values across pixels instead and pays ~0.6 shuffle moves per packed FMA).
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

template <typename T> struct Pair;
template <> struct Pair<float> {
  typedef f32x2 raw_t;                                   // a pair as it lies in memory (kept in registers until it is needed)
  static __device__ __forceinline__ raw_t ld_raw(const void* p) { return *reinterpret_cast<const f32x2*>(p); }
  static __device__ __forceinline__ f32x2 cvt(raw_t r) { return r; }
  static __device__ __forceinline__ raw_t zero() { return f32x2{0.f, 0.f}; }
  static __device__ __forceinline__ f32x2 ld(const void* p) { return *reinterpret_cast<const f32x2*>(p); }
  static __device__ __forceinline__ void st(float* p, f32x2 v) { *reinterpret_cast<f32x2*>(p) = v; }
};
template <> struct Pair<bf16_t> {
  typedef uint32_t raw_t;
  static __device__ __forceinline__ raw_t ld_raw(const void* p) { return *reinterpret_cast<const uint32_t*>(p); }
  static __device__ __forceinline__ f32x2 cvt(raw_t u) { return f32x2{__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)}; }
  static __device__ __forceinline__ raw_t zero() { return 0u; }
  static __device__ __forceinline__ f32x2 ld(const void* p) {
    const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
    return f32x2{__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)};
  }
  static __device__ __forceinline__ void st(bf16_t* p, f32x2 v) {
    *reinterpret_cast<uint32_t*>(p) = (uint32_t)f2bf(v.x) | ((uint32_t)f2bf(v.y) << 16);
  }
};

// Sum each of 16 per-lane values over the 64 lanes of a wave and give every lane all 16 totals.
// LDS transpose instead of 96 ds_bpermute: red[p][lane] (16 conflict-free b32 writes), lane L then sums
// a quarter row (4 x b128) of pixel L/4, two quad-DPP adds finish the row, one b32 write per pixel and
// four broadcast b128 reads return the totals.  `red` = this wave's private 4 KiB + 64 B region.
__device__ __forceinline__ void wave_sum16(float (&v)[16], float* red, int lane) {
#pragma unroll
  for (int p = 0; p < 16; ++p) red[p * 64 + lane] = v[p];
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // cross-lane hand-off inside the wave: order writes before reads
  const float4* row = reinterpret_cast<const float4*>(red + (lane >> 2) * 64 + (lane & 3) * 16);
  const float4 a = row[0], b = row[1], c = row[2], d = row[3];
  float t = ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w)) + ((c.x + c.y) + (c.z + c.w)) + ((d.x + d.y) + (d.z + d.w));
  t += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, t), 0xB1, 0xf, 0xf, true));  // quad xor 1
  t += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, t), 0x4E, 0xf, 0xf, true));  // quad xor 2
  float* tot = red + 16 * 64;
  if ((lane & 3) == 0) tot[lane >> 2] = t;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const float4* tv = reinterpret_cast<const float4*>(tot);
#pragma unroll
  for (int p4 = 0; p4 < 4; ++p4) {
    const float4 r = tv[p4];
    v[p4 * 4 + 0] = r.x; v[p4 * 4 + 1] = r.y; v[p4 * 4 + 2] = r.z; v[p4 * 4 + 3] = r.w;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // totals read before the region is written again
}

template <> struct Pair<f16_t> {
  typedef uint32_t raw_t;
  static __device__ __forceinline__ raw_t ld_raw(const void* p) { return *reinterpret_cast<const uint32_t*>(p); }
  static __device__ __forceinline__ f32x2 cvt(raw_t u) { return f32x2{h_lo(u), h_hi(u)}; }
  static __device__ __forceinline__ raw_t zero() { return 0u; }
  static __device__ __forceinline__ f32x2 ld(const void* p) {
    const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
    return f32x2{h_lo(u), h_hi(u)};
  }
  static __device__ __forceinline__ void st(f16_t* p, f32x2 v) { *reinterpret_cast<uint32_t*>(p) = pk_h2(v.x, v.y); }
};

constexpr int CC = 128;  // channels per chunk = 64 lanes x 2

// mtbt_dwconv_kernel_choice: what the launch functions below are about to launch, written where they would launch it (DwArgs::choice)
inline int dw_report(int32_t* choice, int th, int tw, int xb, int maxch, bool full, int act, long tiles, long blocks, int ygrid) {
  const int32_t v[9] = {th, tw, xb, maxch, full ? 1 : 0, act, (int32_t)tiles, (int32_t)blocks, ygrid};
  for (int i = 0; i < 9; ++i) choice[i] = v[i];
  return MTBT_OK;
}


// MAXCH = ceil(C / 128) chunks held in registers.  Workgroups are PERSISTENT: each walks a strided list of tiles
// (XCD-contiguous ranges, so neighbouring tiles' halos meet in one L2); with a single chunk (C <= 128) the taps stay
// in registers across tiles.
// ACT: the activation of the scale / shift form as a compile-time constant (-1 = the runtime `act` argument): with the switch inside
// the per-element epilogue the non-LayerNorm kernels were twice the code size of the LayerNorm ones and 65 % slower (instruction fetch).
// FULL: H % TH == 0 and W % TW == 0 -- no per-pixel bounds branches around the stores.
template <typename T, int KS, bool LN, int TH, int TW, int MAXCH, int XB, int OCC = 2, bool REGT = (MAXCH == 1), int ACT = -1, bool FULL = false>
__global__ __launch_bounds__((TH / 2) * (TW / XB) * 64, OCC) void dwconv_kernel(
    const T* __restrict__ x_, const T* __restrict__ w_ /* [KS*KS][C] */, const float* __restrict__ bias_,
    const float* __restrict__ lnw_, const float* __restrict__ lnb_, float eps, const float* __restrict__ scale_,
    const float* __restrict__ shift_, int act, T* __restrict__ y_, T* __restrict__ raw_, const T* res_, int N, int H, int W,
    int C, int dbg) {
  // One-chunk kernels take the 128-channel chunk from blockIdx.y: the scale / shift form has no cross-channel step, so a wider tensor
  // (depthwise dgrad of stages 1-3, the 256-channel 3x3 head convs) runs as independent chunks with the taps in registers instead of the
  // multi-chunk kernel's chunk loop.  C stays the pixel pitch; Cn = the channels from this chunk's first one on.
  const int cg = (MAXCH == 1) ? (int)blockIdx.y * CC : 0;
  const int Cx = C, cgx = cg;
#include "dwconv_body.inc"
}

// Depth multiplier (mtbt_dwconv3x3_mult_nhwc): output [N,H,W,C] with C = M * Cx, output channel j reads input channel j mod Cx.  The
// one-chunk scale / shift kernel with the input chunk and pitch separated from the output's; per channel the arithmetic is the plain form's.
template <typename T, int TH, int TW, int ACT, bool FULL>
__global__ __launch_bounds__((TH / 2) * (TW / 8) * 64, 2) void dwconv_mult_kernel(
    const T* __restrict__ x_, const T* __restrict__ w_ /* [9][C] */, const float* __restrict__ scale_, const float* __restrict__ shift_, int act,
    T* __restrict__ y_, int N, int H, int W, int C, int Cx) {
  constexpr int KS = 3, MAXCH = 1, XB = 8;
  constexpr bool LN = false, REGT = true;
  const float* __restrict__ bias_ = nullptr;
  const float* __restrict__ lnw_ = nullptr;
  const float* __restrict__ lnb_ = nullptr;
  T* __restrict__ raw_ = nullptr;
  const T* res_ = nullptr;
  const float eps = 0.f;
  const int dbg = 0;
  const int cg = (int)blockIdx.y * CC, cgx = ((int)blockIdx.y % (Cx / CC)) * CC;
#include "dwconv_body.inc"
}

template <typename T, int TH, int TW, int ACT, bool FULL>
int launch_dw_mult(const void* x, const void* w, const float* scale, const float* shift, int act, void* y, int N, int H, int W, int C, int Cx, int32_t* choice,
                   hipStream_t s) {
  constexpr int NT = (TH / 2) * (TW / 8) * 64;
  constexpr int PARTS = CC * (int)sizeof(T) / 16, PXI = 64 / PARTS, IWP = ((TW + 2 + PXI - 1) / PXI) * PXI;
  constexpr int lds = (TH + 2) * IWP * CC * (int)sizeof(T);
  const long tiles = (long)N * ((H + TH - 1) / TH) * ((W + TW - 1) / TW);
  if (tiles > 0x7fffffffL) return MTBT_EINVAL;
  // the grid of launch_dw for the same output width: persistent workgroups per 128-channel chunk, the chunks as grid rows
  constexpr int by_waves = (4 * 2) / (NT / 64) > 0 ? (4 * 2) / (NT / 64) : 1;
  constexpr int cap = by_waves < 4 ? by_waves : 4;
  const long resident = 256L * (160 * 1024 / lds > cap ? cap : 160 * 1024 / lds);
  long blocks = tiles < resident ? tiles : resident;
  blocks = (blocks + 7) / 8 * 8;
  const int ygrid = C / CC;
  if (ygrid > 1) { blocks = (blocks / ygrid + 7) / 8 * 8; if (blocks < 8) blocks = 8; }
  if (choice) return dw_report(choice, TH, TW, 8, 1, FULL, ACT, tiles, blocks, ygrid);
  auto kern = dwconv_mult_kernel<T, TH, TW, ACT, FULL>;
  if (int rc = mtbt_allow_lds(kern, lds)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)ygrid), dim3(NT), lds, s, (const T*)x, (const T*)w, scale, shift, act, (T*)y, N, H, W, C, Cx);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}

// the variant choice of dw_run's 3x3 scale / shift branch (activation constant, full-tile form), so that a channel block of the multiplier
// form runs the code a plain call on that block runs
template <typename T, int TW, bool VARIANTS>
int dw_run_mult(const DwArgs& a, int Cx, hipStream_t s) {
#define DW_M(ACTV, FULLV) launch_dw_mult<T, 4, TW, ACTV, FULLV>(a.x, a.w, a.scale, a.shift, a.act, a.y, a.N, a.H, a.W, a.C, Cx, a.choice, s)
  if constexpr (VARIANTS) {
    const bool full = a.H % 4 == 0 && a.W % TW == 0;
    if (a.act == MTBT_ACT_NONE) return full ? DW_M(MTBT_ACT_NONE, true) : DW_M(MTBT_ACT_NONE, false);
    if (a.act == MTBT_ACT_SILU) return full ? DW_M(MTBT_ACT_SILU, true) : DW_M(MTBT_ACT_SILU, false);
    return full ? DW_M(-1, true) : DW_M(-1, false);
  } else {
    return DW_M(-1, false);
  }
#undef DW_M
}

template <typename T, int KS, bool LN, int TH, int TW, int MAXCH, int XB = 8, int ACT = -1, bool FULL = false, int OCC = 2, bool REGT = (MAXCH == 1)>
int launch_dw(const void* x, const void* w, const float* bias, const float* lnw, const float* lnb, float eps,
              const float* scale, const float* shift, int act, void* y, void* raw, const void* res, int N, int H, int W, int C, int32_t* choice,
              hipStream_t s) {
  constexpr int NT = (TH / 2) * (TW / XB) * 64;
  constexpr int PARTS = CC * (int)sizeof(T) / 16, PXI = 64 / PARTS, IWP = ((TW + KS - 1 + PXI - 1) / PXI) * PXI;
  constexpr int lds_tile = (TH + KS - 1) * IWP * CC * (int)sizeof(T), lds_red = LN ? (NT / 64) * (16 * 64 + 16) * 4 : 0;
  constexpr int lds_taps = REGT ? 0 : ((KS * KS + PXI - 1) / PXI) * 1024;
  constexpr int lds = MAXCH == 1 ? lds_tile + lds_taps + lds_red : (lds_tile + lds_taps > lds_red ? lds_tile + lds_taps : lds_red);
  static_assert(lds <= 160 * 1024, "LDS");
  const long tiles = (long)N * ((H + TH - 1) / TH) * ((W + TW - 1) / TW);
  if (tiles > 0x7fffffffL) return MTBT_EINVAL;
  // persistent workgroups: as many as stay resident (LDS-limited, at most 4 per CU), a multiple of the 8 XCDs
  // (also wave-limited: __launch_bounds__(NT, OCC) promises OCC waves per SIMD = 4 * OCC per CU, i.e. 4 * OCC / (NT / 64) workgroups; a
  // workgroup that had to queue behind the resident ones would start its tile list late)
  constexpr int by_waves = (4 * OCC) / (NT / 64) > 0 ? (4 * OCC) / (NT / 64) : 1;
  constexpr int cap = by_waves < 4 ? by_waves : 4;
  const long resident = 256L * (160 * 1024 / lds > cap ? cap : 160 * 1024 / lds);
  long blocks = tiles < resident ? tiles : resident;
  blocks = (blocks + 7) / 8 * 8;
  const int ygrid = MAXCH == 1 ? (C + CC - 1) / CC : 1;      // one-chunk kernel on a wider tensor: the chunks are grid rows
  if (ygrid > 1) { blocks = (blocks / ygrid + 7) / 8 * 8; if (blocks < 8) blocks = 8; }
  if (choice) return dw_report(choice, TH, TW, XB, MAXCH, FULL, ACT, tiles, blocks, ygrid);
  auto kern = dwconv_kernel<T, KS, LN, TH, TW, MAXCH, XB, OCC, REGT, ACT, FULL>;
  if (int rc = mtbt_allow_lds(kern, lds)) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)ygrid), dim3(NT), lds, s, (const T*)x, (const T*)w, bias, lnw, lnb, eps, scale, shift,
                     act, (T*)y, (T*)raw, (const T*)res, N, H, W, C, 0 /* ablation bits: development builds only */);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}

template <typename T, int KS, bool LN, int TH, int TW, int ACT, bool FULL>
int dispatch_chunks(const void* x, const void* w, const float* bias, const float* lnw, const float* lnb, float eps,
                    const float* scale, const float* shift, int act, void* y, void* raw, const void* res, int N, int H, int W, int C, bool half,
                    int32_t* choice, hipStream_t s) {
  // (An earlier separate kernel for two / three chunks -- taps of a chunk in registers, one tile per workgroup -- was
  // 10-25 % faster on those layers but restaged its LDS tile behind a plain __syncthreads(): DESIGN.md 4 has the root cause.)
  // `half` = the TH x TW/2 tile with 4 outputs per lane row (twice the waves per tile, half the accumulators): see dw_run.
  const int nch = (C + CC - 1) / CC;
  if constexpr (!LN) {   // no cross-channel step: the one-chunk kernel, chunks as grid rows
    if constexpr (KS == 7) {
      if (half) return launch_dw<T, KS, LN, TH, TW / 2, 1, 4, ACT, FULL>(x, w, bias, lnw, lnb, eps, scale, shift, act, y, raw, res, N, H, W, C, choice, s);
    }
    return launch_dw<T, KS, LN, TH, TW, 1, 8, ACT, FULL>(x, w, bias, lnw, lnb, eps, scale, shift, act, y, raw, res, N, H, W, C, choice, s);
  } else {
  if (nch <= 1) return launch_dw<T, KS, LN, TH, TW, 1, 8, ACT, FULL>(x, w, bias, lnw, lnb, eps, scale, shift, act, y, raw, res, N, H, W, C, choice, s);
  if (nch <= 2) return launch_dw<T, KS, LN, TH, TW, 2, 8, ACT, FULL>(x, w, bias, lnw, lnb, eps, scale, shift, act, y, raw, res, N, H, W, C, choice, s);
  if (nch <= 3) return launch_dw<T, KS, LN, TH, TW / 2, 3, 4, ACT, FULL>(x, w, bias, lnw, lnb, eps, scale, shift, act, y, raw, res, N, H, W, C, choice, s);
  // (six chunks: ONE wave per SIMD -- at two the 48 accumulator pairs + taps + LayerNorm vectors spilled 344 bytes per lane; 40 -> 25 us on stage 3)
  if (nch <= 6) return launch_dw<T, KS, LN, TH, TW / 2, 6, 4, ACT, FULL, 1>(x, w, bias, lnw, lnb, eps, scale, shift, act, y, raw, res, N, H, W, C, choice, s);
  return MTBT_EINVAL;
  }
}

// one storage type: LayerNorm / scale-shift form, 7x7 / 3x3, activation constant, full-tile variant.  VARIANTS = false (fp32, a test
// path) builds only the runtime-activation bounds-checked kernels.
template <typename T, int TW, bool VARIANTS>
int dw_run(const DwArgs& a, hipStream_t s) {
#define DW_ARGS a.x, a.w, a.bias, a.ln_w, a.ln_b, a.ln_eps, a.scale, a.shift, a.act, a.y, a.raw, a.res, a.N, a.H, a.W, a.C, half, a.choice, s
  const bool ln = a.ln_w != nullptr;
  // the half-width tile (4 x TW/2, 4 outputs per lane row): LayerNorm form from three chunks on (stage 2 of the 640x640 forward, 40x40 maps:
  // 48.5 -> 33 us; twice the waves per tile hide what the 96-register accumulator tile of three chunks could not), scale / shift 7x7 form
  // when the width is not a whole number of full tiles (depthwise dgrad at 40x40 / 20x20: 68 -> 46 us at batch 32) --
  // tools/dw_tile_probe.py, profiles/r02_h_dw_tile_probe.txt
  const bool half = ln ? (a.C + CC - 1) / CC > 2 : (a.ksize == 7 && a.W % TW != 0);
  const int tw = half ? TW / 2 : TW;
  const bool full = VARIANTS && a.H % 4 == 0 && a.W % tw == 0;
#define DW_BY_FULL(KSV, LNV, ACTV) (full ? dispatch_chunks<T, KSV, LNV, 4, TW, ACTV, VARIANTS>(DW_ARGS) : dispatch_chunks<T, KSV, LNV, 4, TW, ACTV, false>(DW_ARGS))
  if (ln) return a.ksize == 7 ? DW_BY_FULL(7, true, 0) : DW_BY_FULL(3, true, 0);
  if (VARIANTS && a.act == MTBT_ACT_NONE) return a.ksize == 7 ? DW_BY_FULL(7, false, (VARIANTS ? MTBT_ACT_NONE : -1)) : DW_BY_FULL(3, false, (VARIANTS ? MTBT_ACT_NONE : -1));
  if (VARIANTS && a.act == MTBT_ACT_SILU) return a.ksize == 7 ? DW_BY_FULL(7, false, (VARIANTS ? MTBT_ACT_SILU : -1)) : DW_BY_FULL(3, false, (VARIANTS ? MTBT_ACT_SILU : -1));
  return a.ksize == 7 ? DW_BY_FULL(7, false, -1) : DW_BY_FULL(3, false, -1);
#undef DW_BY_FULL
#undef DW_ARGS
}

}  // namespace
