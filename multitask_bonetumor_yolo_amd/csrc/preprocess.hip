// Input pipeline on the device: the per-sample image work of `BTXRDDataset.__getitem__`
// (/root/reference/src/dataset_btxrdv2.py:109-166) for a whole batch in one launch:
//
//   _letterbox (:109-134)   scale = S / max(H0, W0); new = max(1, int(dim * scale));
//                           image  cv2.resize(INTER_LINEAR), mask  cv2.resize(INTER_NEAREST);
//                           copyMakeBorder top-left aligned: image pad (114,114,114), mask pad 0
//   :157-166                BGR -> RGB, float32 / 255, HWC -> CHW;  mask / 255 > 0.5 -> {0,1} float32, [1,S,S]
//
// cv2 is a third-party dependency that is absent here; the arithmetic restated below is OpenCV's published 8-bit
// path (modules/imgproc/src/resize.cpp; IPP is not used for 8-bit linear unless "not exact" IPP is enabled):
//   linear   fx = (float)((dx + 0.5) * scale_x - 0.5), sx = floor(fx), fx -= sx; sx < 0 -> (0, 0); sx >= W-1 -> (W-1, 0);
//            coefficients short(round_half_even((1-fx) * 2048)), short(round_half_even(fx * 2048));
//            horizontal pass in int:  r = S[sx] * a0 + S[sx+1] * a1;
//            vertical pass:           dst = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
//   nearest  sx = min(floor(dx * scale_x), W-1), same for y
// with scale_x = 1.0 / ((double)new_w / W0).  All of it is integer work except the coefficient set-up, which is done in
// the same double/float steps (this file is compiled with -ffp-contract=off so that (dx+0.5)*scale-0.5 is not fused).
//
// One thread produces 4 horizontally adjacent output pixels of one image: three float4 plane stores + one mask
// float4 store (the output, 16 B per pixel, is the HBM traffic that bounds the kernel); the <= 12 source bytes per pixel
// are gathered through L2.
//
// That pixel is written once, in quad_pixels, for a source under a placement (the reference has NO augmentation: the placement
// is the project's own definition, include/mtbt_hip.h mtbt_augment_batch).  R = the source resized to new_w x new_h by the
// arithmetic above (never materialised); Q = R under one of the eight dihedral orientations; the canvas shows Q at (off_x, off_y),
// pad elsewhere; an optional 256-entry table per channel remaps the resized byte before the /255.  The three kernels only say
// which (canvas, dy, dx0, source, placement, table) a thread has, then call quad_pixels and store_quad:
//   letterbox_kernel  blockIdx.y = image = canvas; offsets 0, orient 0 and no table as compile-time constants (PLACED = false)
//   augment_kernel    blockIdx.y = image = canvas; the caller's placement and table
//   mosaic_kernel     blockIdx.y = canvas * 4 + tile, the source picked per canvas region (include/mtbt_hip.h mtbt_mosaic_batch)
#include "common.h"

namespace {

constexpr int MAX_IMAGES = 32;   // images per launch (descriptors travel as kernel arguments)

struct RawImage {
  const uint8_t* bgr;    // [H0][row_stride] bytes, 3 per pixel
  const uint8_t* mask;   // [H0][mask_stride] or null
  long row_stride, mask_stride;
  int H0, W0, new_h, new_w;
  double scale_x, scale_y;   // source step per output pixel (cv2's 1 / inv_scale)
};
struct Batch { RawImage im[MAX_IMAGES]; };
struct Placement { int off_x, off_y, orient, reserved; };   // of the oriented image Q on the canvas
struct Placements { Placement p[MAX_IMAGES]; };              // 2048 + 512 bytes of kernel arguments with Batch
constexpr int MAX_CANVASES = MAX_IMAGES / 4;                 // mosaic canvases per launch: four descriptors each
struct Centres { int cx[MAX_CANVASES], cy[MAX_CANVASES]; };
struct Quad { float r[4], g[4], b[4], m[4]; };               // four adjacent canvas pixels: RGB in [0,1] and the mask

__device__ __forceinline__ void linear_tap(int d, double scale, int size, int& s0, int& s1, int& c0, int& c1) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= size - 1) { f = 0.f; s = size - 1; }
  s0 = s;
  s1 = min(s + 1, size - 1);
  c0 = __float2int_rn((1.f - f) * 2048.f);
  c1 = __float2int_rn(f * 2048.f);
}

// The canvas pixels (dy, dx0 .. dx0+3) of source im under placement g and an optional table.  They lie on one row of Q, which is
// one row of R (a shared vertical tap) or, transposed, one column of R (a shared horizontal tap); the other tap is per pixel.
// Every source index comes out of linear_tap / the clamped nearest index, so it lies in [0, size-1] whatever the geometry is.
// PLACED = false is the letterbox: g and table are not read, the orientation selects fold away at compile time.
template <bool PLACED>
__device__ __forceinline__ void quad_pixels(const RawImage& im, const Placement& g, const uint8_t* table, int dy, int dx0, Quad& out) {
  const int off_x = PLACED ? g.off_x : 0, off_y = PLACED ? g.off_y : 0, orient = PLACED ? g.orient : 0;
  if (!PLACED) table = nullptr;
  const bool flip_x = orient & 1, flip_y = orient & 2, transposed = orient & 4;
  const int qw = transposed ? im.new_h : im.new_w, qh = transposed ? im.new_w : im.new_h;
  // the axis of R that runs along a row of Q (per pixel) and the one across it (shared)
  const double scale_p = transposed ? im.scale_y : im.scale_x, scale_s = transposed ? im.scale_x : im.scale_y;
  const int size_p = transposed ? im.H0 : im.W0, size_s = transposed ? im.W0 : im.H0;
  const float pad = __fdiv_rn(114.f, 255.f);
  const int qy = dy - off_y;
  const bool row_in = qy >= 0 && qy < qh;
  int s0 = 0, s1 = 0, cs0 = 0, cs1 = 0, ms = 0;
  if (row_in) {
    const int u = flip_y ? qh - 1 - qy : qy;
    linear_tap(u, scale_s, size_s, s0, s1, cs0, cs1);
    ms = max(min((int)floor(u * scale_s), size_s - 1), 0);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int qx = dx0 + i - off_x;
    out.r[i] = out.g[i] = out.b[i] = pad;
    out.m[i] = 0.f;
    if (row_in && qx >= 0 && qx < qw) {
      const int v = flip_x ? qw - 1 - qx : qx;
      int p0, p1, cp0, cp1;
      linear_tap(v, scale_p, size_p, p0, p1, cp0, cp1);
      const int sx0 = transposed ? s0 : p0, sx1 = transposed ? s1 : p1, a0 = transposed ? cs0 : cp0, a1 = transposed ? cs1 : cp1;
      const int sy0 = transposed ? p0 : s0, sy1 = transposed ? p1 : s1, b0 = transposed ? cp0 : cs0, b1 = transposed ? cp1 : cs1;
      const uint8_t* row0 = im.bgr + sy0 * im.row_stride;
      const uint8_t* row1 = im.bgr + sy1 * im.row_stride;
      int o[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int r0 = row0[sx0 * 3 + c] * a0 + row0[sx1 * 3 + c] * a1;
        const int r1 = row1[sx0 * 3 + c] * a0 + row1[sx1 * 3 + c] * a1;
        const int t = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
        o[c] = min(max(t, 0), 255);
        if (table) o[c] = table[c * 256 + o[c]];
      }
      out.b[i] = __fdiv_rn((float)o[0], 255.f);
      out.g[i] = __fdiv_rn((float)o[1], 255.f);
      out.r[i] = __fdiv_rn((float)o[2], 255.f);
      if (im.mask) {
        const int mp = max(min((int)floor(v * scale_p), size_p - 1), 0);
        const int mx = transposed ? ms : mp, my = transposed ? mp : ms;
        out.m[i] = im.mask[my * im.mask_stride + mx] >= 128 ? 1.f : 0.f;   // v / 255 > 0.5  <=>  v >= 128
      }
    }
  }
}

__device__ __forceinline__ void store_quad(const Quad& q, int S, int canvas, int dy, int dx0, float* __restrict__ out_img, float* __restrict__ out_mask) {
  const long plane = (long)S * S;
  float* o = out_img + (long)canvas * 3 * plane + (long)dy * S + dx0;
  *reinterpret_cast<float4*>(o) = make_float4(q.r[0], q.r[1], q.r[2], q.r[3]);
  *reinterpret_cast<float4*>(o + plane) = make_float4(q.g[0], q.g[1], q.g[2], q.g[3]);
  *reinterpret_cast<float4*>(o + 2 * plane) = make_float4(q.b[0], q.b[1], q.b[2], q.b[3]);
  if (out_mask) *reinterpret_cast<float4*>(out_mask + (long)canvas * plane + (long)dy * S + dx0) = make_float4(q.m[0], q.m[1], q.m[2], q.m[3]);
}

__global__ __launch_bounds__(256) void letterbox_kernel(const Batch b, int S, float* __restrict__ out_img, float* __restrict__ out_mask) {
  const int quads = S >> 2;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= S * quads) return;
  const int dy = q / quads, dx0 = (q - dy * quads) << 2;
  Quad px;
  quad_pixels<false>(b.im[blockIdx.y], Placement{}, nullptr, dy, dx0, px);
  store_quad(px, S, blockIdx.y, dy, dx0, out_img, out_mask);
}

__global__ __launch_bounds__(256) void augment_kernel(const Batch b, const Placements pl, int S, const uint8_t* __restrict__ lut,
                                                      float* __restrict__ out_img, float* __restrict__ out_mask) {
  const int quads = S >> 2;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= S * quads) return;
  const int dy = q / quads, dx0 = (q - dy * quads) << 2;
  Quad px;
  quad_pixels<true>(b.im[blockIdx.y], pl.p[blockIdx.y], lut ? lut + (long)blockIdx.y * 768 : nullptr, dy, dx0, px);
  store_quad(px, S, blockIdx.y, dy, dx0, out_img, out_mask);
}

// blockIdx.y = canvas * 4 + tile; blockIdx.x runs over the quads of that tile's rectangle [x0, x1) x [y0, y1) of the canvas (x0, x1 are
// multiples of 4, so the four pixels of a thread share a rectangle) and workgroups beyond it leave at once.  The four rectangles partition
// the canvas, so every output byte is written by exactly one thread.  One blockIdx.y per (canvas, rectangle) keeps descriptor and placement
// scalar; the offsets are in canvas coordinates and the table is the canvas's.
__global__ __launch_bounds__(256) void mosaic_kernel(const Batch b, const Placements pl, const Centres ce, int S, const uint8_t* __restrict__ lut,
                                                     float* __restrict__ out_img, float* __restrict__ out_mask) {
  const int canvas = blockIdx.y >> 2, tile = blockIdx.y & 3;
  const int cx = ce.cx[canvas], cy = ce.cy[canvas];
  const int x0 = (tile & 1) ? cx : 0, x1 = (tile & 1) ? S : cx, y0 = (tile & 2) ? cy : 0, y1 = (tile & 2) ? S : cy;
  const int quads = (x1 - x0) >> 2;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= (y1 - y0) * quads) return;   // also the empty rectangle
  const int ty = q / quads;
  const int dy = y0 + ty, dx0 = x0 + ((q - ty * quads) << 2);
  Quad px;
  quad_pixels<true>(b.im[blockIdx.y], pl.p[blockIdx.y], lut ? lut + (long)canvas * 768 : nullptr, dy, dx0, px);
  store_quad(px, S, canvas, dy, dx0, out_img, out_mask);
}

// ---- host: every entry point checks all of its items, then the alignment, then launches ----------------------------------------
// One source and its geometry row (new_w, new_h, off_x, off_y, orient, 0, 0, 0) -> what the kernel reads; false = MTBT_EINVAL.
bool describe(const mtbt_raw_image& s, const int32_t* g, int img_size, RawImage& d, Placement& p) {
  if (!s.bgr || s.height <= 0 || s.width <= 0 || s.row_stride < (int64_t)s.width * 3 || (s.mask && s.mask_row_stride < s.width) ||
      (long)s.height * s.row_stride >= 0x7fffffffL)
    return false;
  if (g[0] < 1 || g[0] > 32768 || g[1] < 1 || g[1] > 32768 || g[4] < 0 || g[4] > 7 || g[5] || g[6] || g[7]) return false;
  d.bgr = s.bgr; d.mask = s.mask; d.row_stride = s.row_stride; d.mask_stride = s.mask_row_stride;
  d.H0 = s.height; d.W0 = s.width; d.new_w = g[0]; d.new_h = g[1];
  d.scale_x = 1.0 / ((double)d.new_w / (double)d.W0);
  d.scale_y = 1.0 / ((double)d.new_h / (double)d.H0);
  // an offset beyond [-q, S] shows nothing of Q, exactly like the bound itself: clamped so that the kernel's int arithmetic cannot wrap
  const int qw = (g[4] & 4) ? g[1] : g[0], qh = (g[4] & 4) ? g[0] : g[1];
  p.off_x = g[2] < -qw ? -qw : (g[2] > img_size ? img_size : g[2]);
  p.off_y = g[3] < -qh ? -qh : (g[3] > img_size ? img_size : g[3]);
  p.orient = g[4];
  p.reserved = 0;
  return true;
}

// the row of the plain letterbox, dataset_btxrdv2.py:114-117 in the same double arithmetic as Python's floats; returns its scale
// (a descriptor without a positive size gets scale 0: describe refuses it, and no out-of-range double is converted to int)
double letterbox_row(const mtbt_raw_image& s, int img_size, int32_t* g) {
  const double scale = s.height > 0 && s.width > 0 ? (double)img_size / (double)(s.height > s.width ? s.height : s.width) : 0.0;
  const int nw = (int)((double)s.width * scale), nh = (int)((double)s.height * scale);
  g[0] = nw < 1 ? 1 : nw; g[1] = nh < 1 ? 1 : nh;
  g[2] = g[3] = g[4] = g[5] = g[6] = g[7] = 0;
  return scale;
}

bool call_ok(const void* items, const void* out_images, int count, int img_size) {
  return items && out_images && count >= 0 && img_size > 0 && img_size % 4 == 0;
}
bool outputs_aligned(const float* out_images, const float* out_masks) { return aligned16(out_images) && (!out_masks || aligned16(out_masks)); }
unsigned blocks_of(long quads) { return (unsigned)((quads + 255) / 256); }

}  // namespace

extern "C" int mtbt_letterbox_batch(const mtbt_raw_image* images, int count, int img_size, float* out_images, float* out_masks,
                                    double* out_scales, void* stream) {
  if (!call_ok(images, out_images, count, img_size)) return MTBT_EINVAL;
  RawImage probe;
  Placement unused;
  int32_t row[8];
  for (int i = 0; i < count; ++i) {   // every image is checked before the first launch
    letterbox_row(images[i], img_size, row);
    if (!describe(images[i], row, img_size, probe, unused)) return MTBT_EINVAL;
  }
  if (!outputs_aligned(out_images, out_masks)) return MTBT_EALIGN;
  const long plane = (long)img_size * img_size;
  for (int first = 0; first < count; first += MAX_IMAGES) {
    const int nb = count - first < MAX_IMAGES ? count - first : MAX_IMAGES;
    Batch b;
    for (int i = 0; i < nb; ++i) {
      const double scale = letterbox_row(images[first + i], img_size, row);
      describe(images[first + i], row, img_size, b.im[i], unused);
      if (out_scales) out_scales[first + i] = scale;
    }
    hipLaunchKernelGGL(letterbox_kernel, dim3(blocks_of(plane / 4), (unsigned)nb), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), b, img_size,
                       out_images + (long)first * 3 * plane, out_masks ? out_masks + (long)first * plane : nullptr);
    MTBT_LAUNCH_CHECK();
  }
  return MTBT_OK;
}

extern "C" int mtbt_augment_batch(const mtbt_raw_image* images, int count, int img_size, const int32_t* geom, int geom_stride,
                                  const uint8_t* lut, float* out_images, float* out_masks, void* stream) {
  if (!call_ok(images, out_images, count, img_size) || !geom || geom_stride != 8) return MTBT_EINVAL;
  RawImage probe;
  Placement unused;
  for (int i = 0; i < count; ++i)   // every image is checked before the first launch
    if (!describe(images[i], geom + 8L * i, img_size, probe, unused)) return MTBT_EINVAL;
  if (!outputs_aligned(out_images, out_masks)) return MTBT_EALIGN;
  const long plane = (long)img_size * img_size;
  for (int first = 0; first < count; first += MAX_IMAGES) {
    const int nb = count - first < MAX_IMAGES ? count - first : MAX_IMAGES;
    Batch b;
    Placements pl;
    for (int i = 0; i < nb; ++i) describe(images[first + i], geom + 8L * (first + i), img_size, b.im[i], pl.p[i]);
    hipLaunchKernelGGL(augment_kernel, dim3(blocks_of(plane / 4), (unsigned)nb), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), b, pl, img_size,
                       lut ? lut + (long)first * 768 : nullptr, out_images + (long)first * 3 * plane,
                       out_masks ? out_masks + (long)first * plane : nullptr);
    MTBT_LAUNCH_CHECK();
  }
  return MTBT_OK;
}

extern "C" int mtbt_mosaic_batch(const mtbt_raw_image* tiles, int count, int img_size, const int32_t* geom, int geom_stride,
                                 const int32_t* centres, const uint8_t* lut, float* out_images, float* out_masks, void* stream) {
  if (!call_ok(tiles, out_images, count, img_size) || !geom || !centres || geom_stride != 8) return MTBT_EINVAL;
  RawImage probe;
  Placement unused;
  for (int i = 0; i < count; ++i) {   // every canvas is checked before the first launch, empty tiles included
    const int cx = centres[2 * i], cy = centres[2 * i + 1];
    if (cx < 0 || cx > img_size || cx % 4 || cy < 0 || cy > img_size) return MTBT_EINVAL;
    for (long k = 4L * i; k < 4L * i + 4; ++k)
      if (!describe(tiles[k], geom + 8 * k, img_size, probe, unused)) return MTBT_EINVAL;
  }
  if (!outputs_aligned(out_images, out_masks)) return MTBT_EALIGN;
  const long plane = (long)img_size * img_size;
  for (int first = 0; first < count; first += MAX_CANVASES) {
    const int nb = count - first < MAX_CANVASES ? count - first : MAX_CANVASES;
    Batch b;
    Placements pl;
    Centres ce;
    long most = 0;   // quads of the largest rectangle of this chunk: the grid's x extent
    for (int i = 0; i < nb; ++i) {
      const int cx = ce.cx[i] = centres[2 * (first + i)], cy = ce.cy[i] = centres[2 * (first + i) + 1];
      for (int t = 0; t < 4; ++t) {
        const long k = 4L * (first + i) + t;
        describe(tiles[k], geom + 8 * k, img_size, b.im[4 * i + t], pl.p[4 * i + t]);
        const long quads = (long)(((t & 1) ? img_size - cx : cx) >> 2) * ((t & 2) ? img_size - cy : cy);
        if (quads > most) most = quads;
      }
    }
    hipLaunchKernelGGL(mosaic_kernel, dim3(blocks_of(most), (unsigned)(4 * nb)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), b, pl, ce, img_size,
                       lut ? lut + (long)first * 768 : nullptr, out_images + (long)first * 3 * plane,
                       out_masks ? out_masks + (long)first * plane : nullptr);
    MTBT_LAUNCH_CHECK();
  }
  return MTBT_OK;
}
