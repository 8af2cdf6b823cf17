// Two back-to-back 1x1 convolutions on the same pixels as ONE launch (include/mtbt_hip.h, mtbt_pw_chain_nhwc):
//
//   t[p][m] = round16( act1( (sum_c W1[m][c] * x[p][c]) * scale1[m] + shift1[m] ) )        C = M = 256
//   y[p][k] =          act2( (sum_m W2[k][m] * t[p][m]) * scale2[k] + shift2[k] )          K = 256 (16-bit y)  or  K <= 32 (fp32 y, bias only)
//
// The sites: every BiFPN node lowers as fuse -> X_conv (1x1 + BN + ELU) -> X_cf.cv1 (1x1 + BN + SiLU), and every class branch of the heads
// ends cv3[i][1][1] (1x1 + BN + SiLU) -> cv3[i][2] (1x1 256 -> nc + bias into the fp32 head map).  As two launches the 256-channel tensor
// between them makes an HBM round trip (2 x 52 MB at P3, batch 16) for ONE reader, and on P4 / P5 the pair is two launch floors.
//
// A workgroup owns 64 consecutive pixels (two such tiles on large maps: NT below); their x rows are an XOR-swizzled [64 px][256] image in LDS (node_gemm.hip's B image).  Each wave
// owns a quarter of the 256 intermediate channels x all 64 pixels with its W1 fragments in registers (no weight tiles in LDS, no barrier per
// reduction step).  After the first GEMM the epilogue's rounded values go back into THE SAME image -- a lane's accumulators of a fragment pair
// are 8 consecutive channels of one pixel (conv_epilogue.h PERM), i.e. one 16-byte slot -- and the second GEMM runs from it; W2's fragments
// are requested right behind the first GEMM's last MFMA and land while its epilogue runs.
//
// BIT-IDENTICAL to the two mtbt_conv2d_nhwc launches: for every element the reduction is the standalone kernels' -- v_mfma_f32_16x16x32
// with the weights as A and the pixels as B, lane quarter lq holding channels 32 g + 8 lq .. + 7 of k-block g (conv_igemm_body.inc: 16-byte
// chunk ks * 4 + lq of a K-step; pw_stream.hip: g * 32 + lq * 8), k-blocks ascending into ONE fp32 accumulator that starts at zero -- and so is
// the epilogue: fmaf(acc, scale, shift) -> activation -> round to the storage type (conv_epilogue_direct / conv_epilogue_fast; scale = 1
// where there is none) for 16-bit outputs, acc + bias for the fp32 map (pw_stream.hip).  tests/test_gpu_pw_chain.py holds both to torch.equal.
#include "common.h"
#include "conv_epilogue.h"
#include "conv_params.h"

namespace {

struct ChainP {
  const void* x;
  const void* w1;
  const void* w2;
  const float* scale1;
  const float* shift1;
  const float* scale2;
  const float* shift2;
  void* y;
  long M;        // pixels (< 2^31)
  int ldy, K, vec_ok;
};

constexpr int CH = 256;                      // C = M = 256: 8 k-blocks of 32 channels
constexpr int TPX = 64;                      // pixels per workgroup
constexpr int NST = CH / 32;
constexpr int ROWB = CH * 2;                 // bytes per image row

// byte offset of 16-byte slot `slot` of pixel row q in the image (the low four slot bits are XORed with the row: conflict-free b128 accesses)
__device__ __forceinline__ int img_off(int q, int slot) { return q * ROWB + ((((slot & 15) ^ (q & 15)) | (slot & ~15)) << 4); }

// F32OUT = false: K = 256, 16-bit y, FC2 = 4 (a wave owns 64 output channels x 64 pixels, as in the first GEMM).
// F32OUT = true:  K <= 16 * FC2, fp32 y: a wave owns ALL output channels of 16 pixels (pw_stream.hip's fragments: row i * 16 + lr, no permutation).
// NT: 64-pixel tiles per workgroup.  The weight fragments come out of the L2 once per workgroup -- 2 x 128 KB for 64 pixels is FOUR times the
// activation traffic -- so on large maps a workgroup runs both GEMM phases over TWO tiles with each matrix loaded once (NT = 2: two images).
template <typename T, int A1, int A2, bool F32OUT, int FC2, int NT>
__global__ __launch_bounds__(256, 2) void pw_chain_kernel(const ChainP p) {
  constexpr int WCH = CH / 4, FC = WCH / 16, FP = 4;
  static_assert(FC % 2 == 0, "fragment pairs (PERM epilogue)");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int IMG = TPX * ROWB;                                      // one image: [64][256] T, x and then t of a tile
  float* aff1 = reinterpret_cast<float*>(smem + NT * IMG);             // scale1 [256] | shift1 [256]
  float* aff2 = aff1 + 2 * CH;                                         // scale2 [256] | shift2 [256]   (16-bit family)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lq = lane >> 4;
  const long pix0 = (long)blockIdx.x * (NT * TPX);
  {
    aff1[tid] = p.scale1 ? p.scale1[tid] : 1.f;
    aff1[CH + tid] = p.shift1 ? p.shift1[tid] : 0.f;
    if constexpr (!F32OUT) {
      aff2[tid] = p.scale2 ? p.scale2[tid] : 1.f;
      aff2[CH + tid] = p.shift2 ? p.shift2[tid] : 0.f;
    }
  }

  // ---- x rows of this workgroup's pixels -> image (ragged last tile: rows past the end fetch the last pixel; they are never stored) ----
#pragma unroll
  for (int tb = 0; tb < NT; ++tb) {
    constexpr int PCS = TPX * (CH / 8) / 256;
    const T* xb = reinterpret_cast<const T*>(p.x);
    char* bimg = smem + tb * IMG;
    uint4 v[PCS];
#pragma unroll
    for (int k = 0; k < PCS; ++k) {
      const int idx = tid + k * 256;
      const int q = idx >> 5, c8 = idx & 31;
      const long pix = pix0 + tb * TPX + q;
      const long pc = pix < p.M ? pix : p.M - 1;
      v[k] = *reinterpret_cast<const uint4*>(xb + pc * CH + c8 * 8);
    }
#pragma unroll
    for (int k = 0; k < PCS; ++k) {
      const int idx = tid + k * 256;
      *reinterpret_cast<uint4*>(bimg + img_off(idx >> 5, idx & 31)) = v[k];
    }
  }

  // ---- this wave's W1 fragments for the whole reduction (node_gemm.hip): fragment row f * 16 + lr holds weight row wave * 64 + epi_row_channel(f * 16 + lr) ----
  uint4 a[NST][FC];
  {
    const T* wbase = reinterpret_cast<const T*>(p.w1) + (long)(wave * WCH) * CH + lq * 8;
#pragma unroll
    for (int g = 0; g < NST; ++g)
#pragma unroll
      for (int f = 0; f < FC; ++f) a[g][f] = *reinterpret_cast<const uint4*>(wbase + (long)epi_row_channel(f * 16 + lr) * CH + g * 32);
  }
  __syncthreads();   // the x images and the affine vectors are written

  f32x4 acc[FC][FP];
  uint4 a2[NST][FC2];
#pragma unroll
  for (int tb = 0; tb < NT; ++tb) {
  char* bimg = smem + tb * IMG;
#pragma unroll
  for (int i = 0; i < FC; ++i)
#pragma unroll
    for (int j = 0; j < FP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < NST; ++g) {
    uint4 b[FP];
#pragma unroll
    for (int j = 0; j < FP; ++j) b[j] = *reinterpret_cast<const uint4*>(bimg + img_off(j * 16 + lr, g * 4 + lq));
#pragma unroll
    for (int i = 0; i < FC; ++i)
#pragma unroll
      for (int j = 0; j < FP; ++j) acc[i][j] = mfma_16x16x32<T>(a[g][i], b[j], acc[i][j]);
  }

  // ---- W2 fragments: requested behind the LAST first-stage GEMM (W1's registers are free), needed after the first epilogue ----
  if (tb == NT - 1) {
    const T* w2 = reinterpret_cast<const T*>(p.w2);
#pragma unroll
    for (int g = 0; g < NST; ++g)
#pragma unroll
      for (int f = 0; f < FC2; ++f) {
        if constexpr (F32OUT) {
          const int row = f * 16 + lr;
          a2[g][f] = row < p.K ? *reinterpret_cast<const uint4*>(w2 + (long)row * CH + g * 32 + lq * 8) : uint4{0u, 0u, 0u, 0u};
        } else {
          a2[g][f] = *reinterpret_cast<const uint4*>(w2 + (long)(wave * WCH + epi_row_channel(f * 16 + lr)) * CH + g * 32 + lq * 8);
        }
      }
  }
  __syncthreads();   // every wave is done with this tile's x image

  // ---- first epilogue (conv_epilogue_direct's arithmetic) -> t, rounded to T, into the image: channels wave * 64 + 32 m + 8 lq .. + 7 = slot wave * 8 + 4 m + lq ----
#pragma unroll
  for (int m = 0; m < FC / 2; ++m) {
    const int cl = wave * WCH + m * 32 + lq * 8;
    const float4 s0 = *reinterpret_cast<const float4*>(aff1 + cl), s1 = *reinterpret_cast<const float4*>(aff1 + cl + 4);
    const float4 h0 = *reinterpret_cast<const float4*>(aff1 + CH + cl), h1 = *reinterpret_cast<const float4*>(aff1 + CH + cl + 4);
#pragma unroll
    for (int j = 0; j < FP; ++j) {
      float v[8];
      v[0] = act_apply(fmaf(acc[2 * m][j][0], s0.x, h0.x), A1); v[1] = act_apply(fmaf(acc[2 * m][j][1], s0.y, h0.y), A1);
      v[2] = act_apply(fmaf(acc[2 * m][j][2], s0.z, h0.z), A1); v[3] = act_apply(fmaf(acc[2 * m][j][3], s0.w, h0.w), A1);
      v[4] = act_apply(fmaf(acc[2 * m + 1][j][0], s1.x, h1.x), A1); v[5] = act_apply(fmaf(acc[2 * m + 1][j][1], s1.y, h1.y), A1);
      v[6] = act_apply(fmaf(acc[2 * m + 1][j][2], s1.z, h1.z), A1); v[7] = act_apply(fmaf(acc[2 * m + 1][j][3], s1.w, h1.w), A1);
      st8<T>(reinterpret_cast<T*>(bimg + img_off(j * 16 + lr, wave * 8 + m * 4 + lq)), v);
    }
  }
  }
  __syncthreads();   // the t images are complete

#pragma unroll
  for (int tb = 0; tb < NT; ++tb) {
  const char* bimg = smem + tb * IMG;
  const long tpix0 = pix0 + tb * TPX;
  if constexpr (!F32OUT) {
#pragma unroll
    for (int i = 0; i < FC; ++i)
#pragma unroll
      for (int j = 0; j < FP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < NST; ++g) {
      uint4 b[FP];
#pragma unroll
      for (int j = 0; j < FP; ++j) b[j] = *reinterpret_cast<const uint4*>(bimg + img_off(j * 16 + lr, g * 4 + lq));
#pragma unroll
      for (int i = 0; i < FC; ++i)
#pragma unroll
        for (int j = 0; j < FP; ++j) acc[i][j] = mfma_16x16x32<T>(a2[g][i], b[j], acc[i][j]);
    }
    ConvP ep{};
    ep.y = p.y; ep.res = nullptr; ep.ldy = p.ldy; ep.ldr = 0; ep.K = CH;
    const EpiSeq seq{tpix0, 16, p.M, 0L, 0L};
    conv_epilogue_direct<T, CH, FC, FP, A2>(ep, acc, aff2, 0, wave * WCH, lane, seq);
  } else {
    // the streaming kernel's second stage (pw_stream.hip): this wave's 16 pixels x all K channels, bias only, fp32 stores
    f32x4 o[FC2];
#pragma unroll
    for (int i = 0; i < FC2; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int q = wave * 16 + lr;
#pragma unroll
    for (int g = 0; g < NST; ++g) {
      const uint4 b = *reinterpret_cast<const uint4*>(bimg + img_off(q, g * 4 + lq));
#pragma unroll
      for (int i = 0; i < FC2; ++i) o[i] = mfma_16x16x32<T>(a2[g][i], b, o[i]);
    }
    const long pix = tpix0 + q;
    float* const yrow = reinterpret_cast<float*>(p.y) + pix * p.ldy;
#pragma unroll
    for (int i = 0; i < FC2; ++i) {
      const int ch = i * 16 + lq * 4;
      if (ch >= p.K || pix >= p.M) continue;
      float sh[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) sh[e] = (p.shift2 && ch + e < p.K) ? p.shift2[ch + e] : 0.f;
      const f32x4 v = f32x4{o[i][0] + sh[0], o[i][1] + sh[1], o[i][2] + sh[2], o[i][3] + sh[3]};
      if (p.vec_ok && ch + 4 <= p.K) *reinterpret_cast<f32x4*>(yrow + ch) = v;
      else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (ch + e < p.K) yrow[ch + e] = v[e];
      }
    }
  }
  }
}

template <typename T, int A1, int A2, bool F32OUT, int FC2, int NT>
int launch_chain_nt(const ChainP& p, hipStream_t s) {
  const long blocks = (p.M + NT * TPX - 1) / (NT * TPX);
  if (blocks <= 0 || blocks > 0x7fffffffL) return MTBT_EINVAL;
  constexpr int lds = NT * TPX * ROWB + (F32OUT ? 2 : 4) * CH * 4;
  if (int rc = mtbt_allow_lds(pw_chain_kernel<T, A1, A2, F32OUT, FC2, NT>, lds)) return rc;
  hipLaunchKernelGGL((pw_chain_kernel<T, A1, A2, F32OUT, FC2, NT>), dim3((unsigned)blocks), dim3(256), lds, s, p);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}

// two tiles per workgroup where that still leaves every CU its two workgroups (256 CUs x 2 x 128 pixels)
constexpr long TWO_TILE_PIXELS = 65536;
template <typename T, int A1, int A2, bool F32OUT, int FC2>
int launch_chain(const ChainP& p, hipStream_t s) {
  return p.M >= TWO_TILE_PIXELS ? launch_chain_nt<T, A1, A2, F32OUT, FC2, 2>(p, s) : launch_chain_nt<T, A1, A2, F32OUT, FC2, 1>(p, s);
}

template <typename T, int A1>
int launch_a1(const ChainP& p, bool f32out, int act2, hipStream_t s) {
  if (f32out) return p.K <= 16 ? launch_chain<T, A1, MTBT_ACT_NONE, true, 1>(p, s) : launch_chain<T, A1, MTBT_ACT_NONE, true, 2>(p, s);
  switch (act2) {
    case MTBT_ACT_NONE: return launch_chain<T, A1, MTBT_ACT_NONE, false, 4>(p, s);
    case MTBT_ACT_SILU: return launch_chain<T, A1, MTBT_ACT_SILU, false, 4>(p, s);
    case MTBT_ACT_ELU: return launch_chain<T, A1, MTBT_ACT_ELU, false, 4>(p, s);
    default: return MTBT_EINVAL;
  }
}

template <typename T>
int launch_t(const ChainP& p, bool f32out, int act1, int act2, hipStream_t s) {
  if (act1 == MTBT_ACT_SILU) return launch_a1<T, MTBT_ACT_SILU>(p, f32out, act2, s);
  if (act1 == MTBT_ACT_ELU) return launch_a1<T, MTBT_ACT_ELU>(p, f32out, act2, s);
  return MTBT_EINVAL;
}

// every argument check, in a fixed order, and the kernel parameters: the shapes launch_t has a kernel for and nothing else
int chain_validate(const mtbt_pw_chain_args* a, ChainP* pp) {
  if (!a || !a->x || !a->w1 || !a->w2 || !a->y) return MTBT_EINVAL;
  if (a->dtype != MTBT_BF16 && a->dtype != MTBT_F16) return MTBT_EINVAL;        // (fp32 parity mode: two mtbt_conv2d_nhwc launches)
  if (a->out_dtype != a->dtype && a->out_dtype != MTBT_F32) return MTBT_EINVAL;
  if (a->C != CH || a->M != CH) return MTBT_EINVAL;
  if (a->pixels <= 0 || a->pixels > 0x7fffff00L) return MTBT_EINVAL;
  if (a->act1 != MTBT_ACT_SILU && a->act1 != MTBT_ACT_ELU) return MTBT_EINVAL;
  const bool f32out = a->out_dtype == MTBT_F32;
  if (f32out) {
    if (a->K < 1 || a->K > 32 || a->act2 != MTBT_ACT_NONE || a->scale2) return MTBT_EINVAL;
    if (a->y_pixel_stride < a->K) return MTBT_EINVAL;
    if (reinterpret_cast<uintptr_t>(a->y) & 3) return MTBT_EALIGN;
  } else {
    if (a->K != CH) return MTBT_EINVAL;
    if (a->act2 != MTBT_ACT_NONE && a->act2 != MTBT_ACT_SILU && a->act2 != MTBT_ACT_ELU) return MTBT_EINVAL;
    if (a->y_pixel_stride < a->K) return MTBT_EINVAL;
    if (a->y_pixel_stride % 8 || !aligned16(a->y)) return MTBT_EALIGN;          // a lane's 8 output channels are one aligned 16-byte store
  }
  if (!aligned16(a->x) || !aligned16(a->w1) || !aligned16(a->w2)) return MTBT_EALIGN;
  ChainP& p = *pp;
  p.x = a->x; p.w1 = a->w1; p.w2 = a->w2;
  p.scale1 = a->scale1; p.shift1 = a->shift1; p.scale2 = a->scale2; p.shift2 = a->shift2;
  p.y = a->y; p.M = a->pixels; p.ldy = a->y_pixel_stride; p.K = a->K;
  p.vec_ok = (f32out && a->y_pixel_stride % 4 == 0 && aligned16(a->y)) ? 1 : 0;  // whole aligned 16-byte fp32 stores (pw_stream.hip)
  return MTBT_OK;
}

}  // namespace

extern "C" int mtbt_sizeof_pw_chain_args(void) { return (int)sizeof(mtbt_pw_chain_args); }

// The pixel-count rule (profiles/pw_chain_sites.txt, batch 16 x 640^2): the 256 -> 256 -> 256 form on the 20 x 20 map (6 400 pixels = 100
// workgroups on 256 CUs) measured 14.8 us against 13.5 us for the two launches, whose smaller tiles fill the machine; from one workgroup per CU
// upwards it wins.  The fp32-output form wins at every size measured.
constexpr long MIN_PIXELS_K256 = 256 * TPX;
extern "C" int mtbt_pw_chain_supported(const mtbt_pw_chain_args* a) {
  ChainP p;
  if (chain_validate(a, &p) != MTBT_OK) return 0;
  return (a->out_dtype == MTBT_F32 || a->pixels >= MIN_PIXELS_K256) ? 1 : 2;
}

extern "C" int mtbt_pw_chain_nhwc(const mtbt_pw_chain_args* a, void* stream) {
  ChainP p;
  if (const int rc = chain_validate(a, &p)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool f32out = a->out_dtype == MTBT_F32;
  return a->dtype == MTBT_F16 ? launch_t<f16_t>(p, f32out, a->act1, a->act2, s) : launch_t<bf16_t>(p, f32out, a->act1, a->act2, s);
}
