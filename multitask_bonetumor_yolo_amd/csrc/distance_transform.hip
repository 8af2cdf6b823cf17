// Exact Euclidean distance transform of bit-packed planes, mtbt_distance_transform, and the two region terms of the segmentation
// loss that read it, mtbt_seg_region_loss (soft Dice and Kervadec's boundary loss).  Contracts in include/mtbt_hip.h.
//
// Packed layout as in surface_dist.hip: a plane is H rows of pitch = 8 * ceil(W / 64) bytes, pixel X is bit X & 7 of byte X >> 3,
// planes are 8-byte aligned and every access to one is an 8-byte load.  Bits X >= W are masked off where a row word is read.
// The transform is integer arithmetic throughout: d2 < 2^29 (H, W <= 16384).
//
// The transform is separable, d2(x, y) = min over y' of (y - y')^2 + g(x, y')^2 with g(x, y') the distance ALONG ROW y' from x to
// the nearest target pixel, and it is taken in that order (rows first, then columns) because of what each pass costs here:
//
// edt_rows_kernel   one wave per (plane, row, 64-bit word), lane = pixel.  g needs no sweep along a packed row: inside the word it
//                   is a clz / ctz of the masked word, beyond it the nearest non-zero word on each side, found by a wave-uniform
//                   walk that stops at the first hit.  Both maps come from one read (targets: the word, and its complement inside
//                   the image).  g is uint16 (0xFFFF: the row has no target), stored 128 contiguous bytes per wave.
// edt_cols_kernel   one wave per (plane, map, column of 64 pixels), lane = pixel column: the LOWER ENVELOPE of the parabolas
//                   (y - y')^2 + g(y')^2 (Meijster, Roerdink, Hesselink 2000; Felzenszwalb, Huttenlocher 2012), a forward sweep
//                   that keeps a stack of (apex s, first row t where it wins) and a backward sweep that reads the stack out.
//                   O(H) per column whatever the plane holds.  With the lanes across x every access is coalesced: g[y][x..x+63]
//                   is 128 contiguous bytes, the output row 256.  The stack needs no memory of its own: entry q of column x lives
//                   in out[q][x] (s in the low, t in the high 16 bits).  q <= t[q] <= y holds in both sweeps (t[0] = 0 and t grows
//                   strictly), so the forward sweep at row y writes rows <= y only, and the backward sweep, which writes row y
//                   while the live entries are q <= y with entry q in registers, never overwrites an entry it still has to read.
//                   A row without a target enters as g = 2^15: g^2 = 2^30 exceeds every true d2 (< 2^29), the sums stay below
//                   2^31, and a result >= 2^30 means the plane has no target at all: the sentinel.
//                   Bound: the latency of the 2 H dependent steps of a column (a division and, on a pop, two dependent loads); the
//                   parallelism is n * maps * ceil(W / 64) waves.
//
// region_sums_kernel   one workgroup per (image, slice of 16384 pixels): sigmoid, target bit, phi; I = sum p t, P = sum p,
//                      F = sum phi p, T = sum t in fp64: thread t adds items t, t + 256, ... of the slice in order, then a fixed
//                      tree (as surface_select_kernel does).
// region_final_kernel  one workgroup: the slices of an image in order, the images in order; dice, boundary, the weighted sum, and
//                      per image the two Dice gradient factors (t = 0, t = 1), formed in fp64 and cast once.
// region_grad_kernel   d_logits (+)= p (1 - p) (factor[t] + k_boundary phi).
#include <cmath>

#include "bitplane.h"

namespace {

constexpr unsigned NONE16 = 0xFFFFu;
constexpr int INF_G = 1 << 15;                  // g of a row without a target, as the envelope takes it
constexpr unsigned D2_NONE = 0xFFFFFFFFu;
constexpr unsigned D2_LIMIT = 1u << 30;         // INF_G^2: no true d2 reaches it
constexpr int RT = 256;                         // threads of the loss workgroups
constexpr int SLICE = RT * 64;                  // pixels per workgroup of the loss kernels

int64_t g_bytes(int64_t c, int64_t H, int64_t W) { return up16(c * 2 * H * (plane_words(W) * 64) * 2); }

int chunk_of(int n, int H, int W) { return ::chunk_of(n, g_bytes(1, H, W)); }   // planes per launch group

struct EdtP {
  const u64* packed;
  uint16_t* g;            // [c][2][H][Wp]
  unsigned* out[2];       // d2_set, d2_unset: [n][H][W] or NULL
  int plane0, H, W, words_x;
};

// ---------------------------------------------------------------------------------------------------------------- rows
__global__ __launch_bounds__(256) void edt_rows_kernel(const EdtP p) {
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const int y = blockIdx.y, pr = blockIdx.z, nw = p.words_x, Wp = nw * 64;
  if (w >= nw) return;
  const u64* row = p.packed + ((size_t)(p.plane0 + pr) * p.H + y) * nw;
  const int x = w * 64 + lane;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    if (!p.out[m]) continue;
    const u64 flip = m ? ~0ull : 0ull;          // the targets of map 1 are the unset pixels inside the image
    const u64 cur = (row[w] ^ flip) & valid_bits(w, p.W);
    int left = -1, right = -1;                  // pixel index of the nearest target in a word before / after this one
    for (int v = w - 1; v >= 0; --v) {
      const u64 b = (row[v] ^ flip) & valid_bits(v, p.W);
      if (b) { left = v * 64 + 63 - __clzll((long long)b); break; }
    }
    for (int v = w + 1; v < nw; ++v) {
      const u64 b = (row[v] ^ flip) & valid_bits(v, p.W);
      if (b) { right = v * 64 + __ffsll((long long)b) - 1; break; }
    }
    const u64 lo = cur & (lane == 63 ? ~0ull : (2ull << lane) - 1ull), hi = cur >> lane;
    const unsigned dl = lo ? (unsigned)(lane - (63 - __clzll((long long)lo))) : (left >= 0 ? (unsigned)(x - left) : NONE16);
    const unsigned dr = hi ? (unsigned)(__ffsll((long long)hi) - 1) : (right >= 0 ? (unsigned)(right - x) : NONE16);
    p.g[((size_t)(pr * 2 + m) * p.H + y) * Wp + x] = (uint16_t)min(dl, dr);
  }
}

// ---------------------------------------------------------------------------------------------------------------- columns
__device__ __forceinline__ int g2_of(const uint16_t* g, size_t Wp, int y) {
  const int v = g[(size_t)y * Wp];
  const int c = v == (int)NONE16 ? INF_G : v;
  return c * c;
}

__global__ __launch_bounds__(64) void edt_cols_kernel(const EdtP p) {
  const int m = blockIdx.y, pr = blockIdx.z, x = blockIdx.x * 64 + threadIdx.x;
  const int H = p.H, W = p.W;
  if (!p.out[m] || x >= W) return;
  const size_t Wp = (size_t)p.words_x * 64;
  const uint16_t* g = p.g + (size_t)(pr * 2 + m) * H * Wp + x;
  unsigned* out = p.out[m] + (size_t)(p.plane0 + pr) * H * W + x;   // out[y * W]: the result, and until then the stack

  int q = 0, s = 0, t = 0, gs2 = g2_of(g, Wp, 0);                   // the top of the stack, in registers
  out[0] = 0u;
  int gn2 = H > 1 ? g2_of(g, Wp, 1) : 0;
  for (int u = 1; u < H; ++u) {
    const int gu2 = gn2;
    if (u + 1 < H) gn2 = g2_of(g, Wp, u + 1);                       // one row ahead of its use
    for (;;) {                                                      // drop the apexes that u beats where they start to win
      const int a = t - s, b = t - u;
      if (a * a + gs2 <= b * b + gu2) break;
      if (q == 0) { q = -1; break; }
      --q;
      const unsigned e = out[(size_t)q * W];
      s = (int)(e & 0xFFFFu);
      t = (int)(e >> 16);
      gs2 = g2_of(g, Wp, s);
    }
    if (q < 0) {
      q = 0; s = u; t = 0; gs2 = gu2;
      out[0] = (unsigned)u;
    } else {                                                        // first row where u wins over s: the numerator is >= 0 here
      const int w = 1 + (int)((unsigned)(u * u - s * s + gu2 - gs2) / (unsigned)(2 * (u - s)));
      if (w < H) {
        ++q; s = u; t = w; gs2 = gu2;
        out[(size_t)q * W] = (unsigned)u | ((unsigned)w << 16);
      }
    }
  }
  for (int u = H - 1; u >= 0; --u) {
    const int d = u - s;
    const unsigned v = (unsigned)(d * d + gs2);
    const bool pop = u == t && q > 0;
    unsigned e = 0u;
    if (pop) e = out[(size_t)(q - 1) * W];                          // row q - 1 < u: not yet overwritten
    out[(size_t)u * W] = v >= D2_LIMIT ? D2_NONE : v;
    if (pop) {
      --q;
      s = (int)(e & 0xFFFFu);
      t = (int)(e >> 16);
      gs2 = g2_of(g, Wp, s);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- region loss
struct RegP {
  const float* logits;      // [B][H][W]
  const float* bias;        // 1 value or NULL
  const u64* targets;       // [B][H][words_x]
  const unsigned* d2_set;   // [B][H][W] or NULL
  const unsigned* d2_unset;
  float* d_logits;          // [B][H][W] or NULL
  double* partial;          // [B][slices][4]
  float* factor;            // [B][2]
  float* out;               // [3]
  int B, H, W, words_x, slices, accumulate;
  double smooth, w_dice, w_boundary;
  float k_boundary;         // w_boundary / (B N)
};

struct Pixel { float p, phi; unsigned t; };

__device__ __forceinline__ Pixel pixel_of(const RegP& r, int b, unsigned i, float bias) {
  const unsigned y = i / (unsigned)r.W, x = i - y * (unsigned)r.W;
  const size_t at = (size_t)b * r.H * r.W + i;
  Pixel px;
  px.t = (unsigned)((r.targets[((size_t)b * r.H + y) * r.words_x + (x >> 6)] >> (x & 63u)) & 1ull);
  px.p = 1.0f / (1.0f + expf(-(r.logits[at] + bias)));
  px.phi = 0.0f;
  if (r.d2_set) {                                                   // both maps or neither: the entry point sees to it
    const unsigned d2 = px.t ? r.d2_unset[at] : r.d2_set[at];
    if (d2 != D2_NONE) {
      const float d = (float)sqrt((double)d2);                      // above 2^24 a uint32 -> float conversion is no longer exact
      px.phi = px.t ? -(d - 1.0f) : d;
    }
  }
  return px;
}

__global__ __launch_bounds__(RT) void region_sums_kernel(const RegP r) {
  __shared__ double red[4][RT];
  const int sl = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const unsigned N = (unsigned)r.H * (unsigned)r.W, i0 = (unsigned)sl * SLICE, i1 = min(N, i0 + (unsigned)SLICE);
  const float bias = r.bias ? *r.bias : 0.f;
  double sI = 0.0, sP = 0.0, sF = 0.0, sT = 0.0;
  for (unsigned i = i0 + tid; i < i1; i += RT) {
    const Pixel px = pixel_of(r, b, i, bias);
    sP += (double)px.p;
    sF += (double)px.phi * (double)px.p;
    if (px.t) { sI += (double)px.p; sT += 1.0; }
  }
  red[0][tid] = sI; red[1][tid] = sP; red[2][tid] = sF; red[3][tid] = sT;
  __syncthreads();
  for (int s = RT / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + s];
    }
    __syncthreads();
  }
  if (tid < 4) r.partial[((size_t)b * r.slices + sl) * 4 + tid] = red[tid][0];
}

__global__ __launch_bounds__(RT) void region_final_kernel(const RegP r) {
  // per image: dice_b and sum phi p go to the first two words of its partials (read by thread 0 once all are there)
  const double N = (double)r.H * (double)r.W;
  for (int b = threadIdx.x; b < r.B; b += RT) {
    double* part = r.partial + (size_t)b * r.slices * 4;
    double I = 0.0, P = 0.0, F = 0.0, T = 0.0;
    for (int sl = 0; sl < r.slices; ++sl) {
      I += part[sl * 4]; P += part[sl * 4 + 1]; F += part[sl * 4 + 2]; T += part[sl * 4 + 3];
    }
    const double num = 2.0 * I + r.smooth, den = P + T + r.smooth;
    // d dice / d p = -[2 t den - num] / den^2 per image, over B for the mean, times w_dice: in fp64, cast once
    const double k = -r.w_dice / ((double)r.B * den * den);
    r.factor[b * 2] = (float)(k * (-num));
    r.factor[b * 2 + 1] = (float)(k * (2.0 * den - num));
    part[0] = 1.0 - num / den;
    part[1] = F;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double dice = 0.0, bnd = 0.0;
    for (int b = 0; b < r.B; ++b) {
      dice += r.partial[(size_t)b * r.slices * 4];
      bnd += r.partial[(size_t)b * r.slices * 4 + 1];
    }
    dice /= (double)r.B;
    bnd /= (double)r.B * N;
    r.out[0] = (float)dice;
    r.out[1] = (float)bnd;
    r.out[2] = (float)(r.w_dice * dice + r.w_boundary * bnd);
  }
}

__global__ __launch_bounds__(RT) void region_grad_kernel(const RegP r) {
  const int sl = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const unsigned N = (unsigned)r.H * (unsigned)r.W, i0 = (unsigned)sl * SLICE, i1 = min(N, i0 + (unsigned)SLICE);
  const float bias = r.bias ? *r.bias : 0.f, f0 = r.factor[b * 2], f1 = r.factor[b * 2 + 1];
  float* d = r.d_logits + (size_t)b * N;
  for (unsigned i = i0 + tid; i < i1; i += RT) {
    const Pixel px = pixel_of(r, b, i, bias);
    const float gz = px.p * (1.0f - px.p) * ((px.t ? f1 : f0) + r.k_boundary * px.phi);
    d[i] = r.accumulate ? d[i] + gz : gz;
  }
}

int slices_of(int H, int W) { return (int)(((int64_t)H * W + SLICE - 1) / SLICE); }

}  // namespace

extern "C" int mtbt_sizeof_distance_args(int which) {
  return which == 0 ? (int)sizeof(mtbt_distance_transform_args) : (which == 1 ? (int)sizeof(mtbt_seg_region_args) : -1);
}

extern "C" int64_t mtbt_distance_transform_workspace_bytes(int n, int H, int W) {
  if (n < 0 || !plane_dims_ok(H, W)) return MTBT_EINVAL;
  if (n == 0) return 0;
  return g_bytes(chunk_of(n, H, W), H, W);
}

extern "C" int mtbt_distance_transform(const mtbt_distance_transform_args* args, void* stream) {
  if (!args) return MTBT_EINVAL;
  const mtbt_distance_transform_args& a = *args;
  if (a.n < 0 || !plane_dims_ok(a.H, a.W) || !plane_pitch_ok(a.W, a.pitch)) return MTBT_EINVAL;
  if (!a.packed || (!a.d2_set && !a.d2_unset)) return MTBT_EINVAL;
  const int64_t need = mtbt_distance_transform_workspace_bytes(a.n, a.H, a.W);
  if (a.workspace_bytes < need || (need > 0 && !a.workspace)) return MTBT_EINVAL;
  if (!aligned_n(a.packed, 8) || !aligned_n(a.workspace, 16) || !aligned_n(a.d2_set, 4) || !aligned_n(a.d2_unset, 4)) return MTBT_EALIGN;
  if (a.n == 0) return MTBT_OK;

  const int chunk = chunk_of(a.n, a.H, a.W);
  EdtP p;
  p.packed = reinterpret_cast<const u64*>(a.packed);
  p.g = reinterpret_cast<uint16_t*>(a.workspace);
  p.out[0] = a.d2_set; p.out[1] = a.d2_unset;
  p.H = a.H; p.W = a.W; p.words_x = a.pitch >> 3;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for (int p0 = 0; p0 < a.n; p0 += chunk) {              // the chunks share the workspace: stream order keeps them apart
    const unsigned c = (unsigned)(a.n - p0 < chunk ? a.n - p0 : chunk);
    p.plane0 = p0;
    hipLaunchKernelGGL(edt_rows_kernel, dim3((unsigned)(p.words_x + 3) / 4, (unsigned)p.H, c), dim3(256), 0, s, p);
    MTBT_LAUNCH_CHECK();
    hipLaunchKernelGGL(edt_cols_kernel, dim3((unsigned)p.words_x, 2, c), dim3(64), 0, s, p);
    MTBT_LAUNCH_CHECK();
  }
  return MTBT_OK;
}

extern "C" int64_t mtbt_seg_region_loss_workspace_bytes(int B, int H, int W) {
  if (B < 1 || B > 65535 || !plane_dims_ok(H, W)) return MTBT_EINVAL;
  return up16((int64_t)B * slices_of(H, W) * 4 * 8) + up16((int64_t)B * 2 * 4);
}

extern "C" int mtbt_seg_region_loss(const mtbt_seg_region_args* args, void* stream) {
  if (!args) return MTBT_EINVAL;
  const mtbt_seg_region_args& a = *args;
  if (a.B < 1 || a.B > 65535 || !plane_dims_ok(a.H, a.W) || !plane_pitch_ok(a.W, a.pitch)) return MTBT_EINVAL;
  if (!a.logits || !a.targets || !a.out || !a.workspace) return MTBT_EINVAL;
  if (!(a.smooth >= 0.f) || !(a.w_dice >= 0.f) || !(a.w_boundary >= 0.f) || std::isinf(a.smooth) || std::isinf(a.w_dice) || std::isinf(a.w_boundary))
    return MTBT_EINVAL;                                  // NaN fails the comparisons
  if ((a.d2_set == nullptr) != (a.d2_unset == nullptr) || (a.w_boundary != 0.f && !a.d2_set)) return MTBT_EINVAL;
  if (a.accumulate != 0 && a.accumulate != 1) return MTBT_EINVAL;
  if (a.workspace_bytes < mtbt_seg_region_loss_workspace_bytes(a.B, a.H, a.W)) return MTBT_EINVAL;
  if (!aligned_n(a.targets, 8) || !aligned_n(a.workspace, 16) || !aligned_n(a.logits, 4) || !aligned_n(a.bias, 4) || !aligned_n(a.d2_set, 4) ||
      !aligned_n(a.d2_unset, 4) || !aligned_n(a.d_logits, 4) || !aligned_n(a.out, 4))
    return MTBT_EALIGN;

  RegP r;
  r.logits = a.logits; r.bias = a.bias; r.targets = reinterpret_cast<const u64*>(a.targets);
  r.d2_set = a.d2_set; r.d2_unset = a.d2_unset; r.d_logits = a.d_logits; r.out = a.out;
  r.B = a.B; r.H = a.H; r.W = a.W; r.words_x = a.pitch >> 3; r.slices = slices_of(a.H, a.W); r.accumulate = a.accumulate;
  r.partial = reinterpret_cast<double*>(a.workspace);
  r.factor = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(a.workspace) + up16((int64_t)a.B * r.slices * 4 * 8));
  r.smooth = (double)a.smooth; r.w_dice = (double)a.w_dice; r.w_boundary = (double)a.w_boundary;
  r.k_boundary = (float)((double)a.w_boundary / ((double)a.B * (double)a.H * (double)a.W));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(region_sums_kernel, dim3((unsigned)r.slices, (unsigned)r.B), dim3(RT), 0, s, r);
  MTBT_LAUNCH_CHECK();
  hipLaunchKernelGGL(region_final_kernel, dim3(1), dim3(RT), 0, s, r);
  MTBT_LAUNCH_CHECK();
  if (a.d_logits) {
    hipLaunchKernelGGL(region_grad_kernel, dim3((unsigned)r.slices, (unsigned)r.B), dim3(RT), 0, s, r);
    MTBT_LAUNCH_CHECK();
  }
  return MTBT_OK;
}
