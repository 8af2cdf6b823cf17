// Affine augmentation of a batch on the device (include/mtbt_hip.h mtbt_warp_batch): rotation, shear, any 2 x 3 map.  The reference has
// no augmentation and cv2 is absent, so the rule is the project's own, modelled on cv2 warpAffine(INTER_LINEAR): an inverse map in fixed
// point (1/65536 px, int64), the position reduced to 1/32 px, 2 x 2 taps with weights that sum to 1024.  Everything is integer work up to
// the one correctly rounded /255, so tests/warp_reference.py reproduces the kernel bit for bit.
//
// This is NOT a mode of preprocess.hip's quad_pixels: that body rests on separable taps (a canvas row is a row or a column of the source,
// so one tap is shared by the four pixels of a thread); under a rotation a canvas row is a slanted line through the source and every
// pixel has its own four taps.
//
// One thread produces 4 horizontally adjacent canvas pixels: three float4 plane stores + one mask float4 store, 16 B of output per pixel
// as in augment_kernel.  The <= 13 source bytes per pixel are gathered through L2 as byte loads, and under a turn THEY bound the kernel, not
// the output: a wave's load instruction touches one cache line per source row its 64 lanes reach.  So the shape of the canvas patch a
// wave covers decides the time (MI355X, 32 canvases of 640^2 from 1024 x 768 sources, us per call at 0 / 33 / 90 degrees):
//   workgroup 32 x 32, wave 32 px x 8 rows     134 / 187 / 134   <- this kernel: the same at 0 and 90, best at every angle but exactly 0
//   workgroup 64 x 16, wave 64 px x 4 rows     100 / 212 / 231   (169 at 5 degrees already: only the exact identity shares its rows)
//   workgroup 16 x 64, wave 16 px x 16 rows    240 / 209 / 133
//   workgroup 128 x 8, wave 128 px x 2 rows    107 / 282 / 246
//   1024 px of one row (augment_kernel's walk) 101 / 535 / 360
// (augment_batch with the letterbox geometry on the same sources: 101.)  blockIdx.y is the canvas, so the descriptor and the six
// coefficients are scalar.  No LDS, no atomics; the tiles partition the canvas, so every output byte is written exactly once.
#include "common.h"

namespace {

constexpr int MAX_CANVASES = 32;   // canvases per launch: 32 * (40 + 32) = 2304 bytes of kernel arguments, below augment_kernel's 2560
constexpr int TILE_W = 32, TILE_H = 32;   // canvas pixels per workgroup: 8 quads x 32 rows = 256 threads; a wave is 32 px x 8 rows
constexpr long LIN_MAX = 1L << 26, OFF_MAX = 1L << 47;   // |a|, |b|, |d|, |e| and |c|, |f|: with img_size <= 32768, |X| < 2^48

struct Source {
  const uint8_t* bgr;    // [H0][row_stride] bytes, 3 per pixel
  const uint8_t* mask;   // [H0][mask_stride] or null
  long row_stride, mask_stride;
  int H0, W0;
};
struct Map { int a, b, d, e; long c, f; };   // X = a dx + b dy + c, Y = d dx + e dy + f, in 1/65536 source px
struct Batch { Source im[MAX_CANVASES]; Map map[MAX_CANVASES]; };

__global__ __launch_bounds__(256) void warp_kernel(const Batch b, int S, const uint8_t* __restrict__ lut, float* __restrict__ out_img,
                                                   float* __restrict__ out_mask) {
  const int tiles_x = (S + TILE_W - 1) / TILE_W;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int dx0 = tx * TILE_W + ((threadIdx.x & 7) << 2), dy = ty * TILE_H + (threadIdx.x >> 3);
  if (dx0 >= S || dy >= S) return;   // S % 4 == 0: the four pixels of a thread are inside together
  const int canvas = blockIdx.y;
  const Source& im = b.im[canvas];
  const Map& m = b.map[canvas];
  const uint8_t* table = lut ? lut + (long)canvas * 768 : nullptr;
  const int H0 = im.H0, W0 = im.W0;
  const long x_hi = 32L * W0 - 17, y_hi = 32L * H0 - 17;
  const float pad = __fdiv_rn(114.f, 255.f);
  long X = (long)m.a * dx0 + (long)m.b * dy + m.c, Y = (long)m.d * dx0 + (long)m.e * dy + m.f;   // the row start, once per thread
  float r[4], g[4], bl[4], mk[4];
#pragma unroll
  for (int i = 0; i < 4; ++i, X += m.a, Y += m.d) {
    r[i] = g[i] = bl[i] = pad;
    mk[i] = 0.f;
    const long Xs = (X + 1024) >> 11, Ys = (Y + 1024) >> 11;   // arithmetic shift = floor; 1/32 px
    if (Xs < -16 || Xs > x_hi || Ys < -16 || Ys > y_hi) continue;   // compared in 64 bits, before anything is narrowed
    const int sx = (int)(Xs >> 5), sy = (int)(Ys >> 5), fx = (int)Xs & 31, fy = (int)Ys & 31;   // sx in [-1, W0 - 1]
    const int x0 = max(sx, 0), x1 = min(sx + 1, W0 - 1), y0 = max(sy, 0), y1 = min(sy + 1, H0 - 1);
    const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
    const uint8_t* row0 = im.bgr + y0 * im.row_stride;
    const uint8_t* row1 = im.bgr + y1 * im.row_stride;
    int o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      o[c] = (w00 * row0[x0 * 3L + c] + w01 * row0[x1 * 3L + c] + w10 * row1[x0 * 3L + c] + w11 * row1[x1 * 3L + c] + 512) >> 10;
      if (table) o[c] = table[c * 256 + o[c]];
    }
    bl[i] = __fdiv_rn((float)o[0], 255.f);
    g[i] = __fdiv_rn((float)o[1], 255.f);
    r[i] = __fdiv_rn((float)o[2], 255.f);
    if (im.mask) {
      const int mx = min((int)((Xs + 16) >> 5), W0 - 1), my = min((int)((Ys + 16) >> 5), H0 - 1);   // >= 0 since Xs >= -16
      mk[i] = im.mask[my * im.mask_stride + mx] >= 128 ? 1.f : 0.f;
    }
  }
  const long plane = (long)S * S;
  float* o = out_img + (long)canvas * 3 * plane + (long)dy * S + dx0;
  *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
  *reinterpret_cast<float4*>(o + plane) = make_float4(g[0], g[1], g[2], g[3]);
  *reinterpret_cast<float4*>(o + 2 * plane) = make_float4(bl[0], bl[1], bl[2], bl[3]);
  if (out_mask) *reinterpret_cast<float4*>(out_mask + (long)canvas * plane + (long)dy * S + dx0) = make_float4(mk[0], mk[1], mk[2], mk[3]);
}

// One source and its coefficient row (a, b, c, d, e, f, 0, 0) -> what the kernel reads; false = MTBT_EINVAL.  The descriptor rules are
// mtbt_letterbox_batch's.
bool describe(const mtbt_raw_image& s, const int64_t* k, Source& d, Map& m) {
  if (!s.bgr || s.height <= 0 || s.width <= 0 || s.row_stride < (int64_t)s.width * 3 || (s.mask && s.mask_row_stride < s.width) ||
      (long)s.height * s.row_stride >= 0x7fffffffL)
    return false;
  for (int j : {0, 1, 3, 4})
    if (k[j] < -LIN_MAX || k[j] > LIN_MAX) return false;
  if (k[2] < -OFF_MAX || k[2] > OFF_MAX || k[5] < -OFF_MAX || k[5] > OFF_MAX || k[6] || k[7]) return false;
  d.bgr = s.bgr; d.mask = s.mask; d.row_stride = s.row_stride; d.mask_stride = s.mask_row_stride;
  d.H0 = s.height; d.W0 = s.width;
  m.a = (int)k[0]; m.b = (int)k[1]; m.c = k[2]; m.d = (int)k[3]; m.e = (int)k[4]; m.f = k[5];
  return true;
}

}  // namespace

extern "C" int mtbt_warp_batch(const mtbt_raw_image* images, int count, int img_size, const int64_t* coef, int coef_stride,
                               const uint8_t* lut, float* out_images, float* out_masks, void* stream) {
  if (!images || !coef || !out_images || coef_stride != 8 || count < 0 || img_size <= 0 || img_size % 4 || img_size > 32768) return MTBT_EINVAL;
  Source probe;
  Map unused;
  for (int i = 0; i < count; ++i)   // every canvas is checked before the first launch
    if (!describe(images[i], coef + 8L * i, probe, unused)) return MTBT_EINVAL;
  if (!aligned16(out_images) || (out_masks && !aligned16(out_masks))) return MTBT_EALIGN;
  const long plane = (long)img_size * img_size;
  const unsigned tiles = (unsigned)(((img_size + TILE_W - 1) / TILE_W) * ((img_size + TILE_H - 1) / TILE_H));
  for (int first = 0; first < count; first += MAX_CANVASES) {
    const int nb = count - first < MAX_CANVASES ? count - first : MAX_CANVASES;
    Batch b;
    for (int i = 0; i < nb; ++i) describe(images[first + i], coef + 8L * (first + i), b.im[i], b.map[i]);
    hipLaunchKernelGGL(warp_kernel, dim3(tiles, (unsigned)nb), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), b, img_size,
                       lut ? lut + (long)first * 768 : nullptr, out_images + (long)first * 3 * plane,
                       out_masks ? out_masks + (long)first * plane : nullptr);
    MTBT_LAUNCH_CHECK();
  }
  return MTBT_OK;
}
