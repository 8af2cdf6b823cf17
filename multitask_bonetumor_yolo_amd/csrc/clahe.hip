// Contrast-limited adaptive histogram equalisation of raw uint8 images (mtbt_clahe_batch; THE RULE and the contract are in
// include/mtbt_hip.h, tests/clahe_reference.py restates the rule in numpy), feeding `preprocess.clahe_batch` and the `clahe=` option of the
// `*_samples` functions.  Integer arithmetic and integer atomics only: the output is a pure function of the input.
//
// Workspace of a call with T = count * gx * gy tiles: int32 hist [T][256] (cleared on the stream by the entry point), then uint8 lut [T][256].
// Three launches per <= 32 images (descriptors travel as kernel arguments):
//
// clahe_hist_kernel    grid (row segments, tiles, images).  A tile is split into segments of whole rows of about SEG_PIXELS pixels, so a
//                      3000 x 3000 image at 8 x 8 (tiles of 140 000 pixels) is 576 workgroups instead of 64 (measured: 97 us a call
//                      against 275 us with one workgroup per tile, no difference at 16 images); a segment beyond its tile
//                      leaves at once.  A row of the segment is cut by the ADDRESS of its first byte into a head (up to 15 pixels, until
//                      a 16-byte boundary), groups of 16 pixels (one or three 16-byte loads) and a tail; the reflected columns of the last
//                      tile column are a fourth piece (each of the three at most 15 pixels, loaded together, then added).  The pieces of
//                      all rows are dealt to the 256 threads in one flat index.  A thread merges equal neighbouring keys of its group
//                      before the LDS atomic, a wave whose active groups all hold ONE key (radiograph background) adds them with a
//                      single atomic, and each wave has its own sub-histogram: one bin taking most pixels does not serialise on one LDS
//                      word.  The four sub-histograms are summed and the non-zero bins go to the workspace with one int32 global atomic
//                      each.
// clahe_curve_kernel   grid (tiles, images), 256 threads = 256 bins: clip, block sum of the excess, the closed form of the remainder,
//                      inclusive scan, the rounded curve; one byte per thread into the workspace.
// clahe_apply_kernel   grid (row chunks, cells, images).  A cell is the set of pixels between the same four tile centres ((gx + 1) x
//                      (gy + 1) cells, the outer ones half a tile wide); its four curves are staged in LDS as ONE 32-bit word per grey
//                      level, so a value costs one LDS read.  The kernel works on BYTES of a row (pixel = byte / channels), in the 16-byte
//                      windows of the DESTINATION's alignment: a window inside the cell is one 16-byte store, and one 16-byte load when
//                      source and destination rows are congruent mod 16 (else 16 byte loads); the first and last window of a row are
//                      bytewise under a mask, the loads all issued before the arithmetic.  A thread reads its bytes before it writes
//                      them and no other thread touches them: dst == src is safe.  The division by 4 * area is a float estimate corrected
//                      exactly in integers.
#include "common.h"

#ifndef MTBT_CLAHE_SEG_PIXELS
#define MTBT_CLAHE_SEG_PIXELS 16384   // pixels of a histogram workgroup; a development build with 1 << 30 is one workgroup per tile
#endif

namespace {

constexpr int MAX_IMAGES = 32;    // images per launch
constexpr int PT = 256;           // threads of a block = bins
constexpr int SEG_PIXELS = MTBT_CLAHE_SEG_PIXELS;
constexpr int CHUNK_BYTES = 16384;   // bytes of an apply workgroup

struct Image {
  const uint8_t* src;
  uint8_t* dst;
  long sstride, dstride;
  int H, W, ch, clip;
  int tw, th;          // tile size
  int seg_rows;        // rows of a histogram segment
  int tile0;           // first tile of this image in the workspace
};
struct Batch { Image im[MAX_IMAGES]; };   // 64 bytes each: 2 KiB of kernel arguments

__device__ __forceinline__ int reflect(int i, int n) { return i < n ? i : 2 * (n - 1) - i; }
__device__ __forceinline__ int byte_of(const uint4& q, int i) {   // i is a compile-time constant after unrolling
  const unsigned w = i < 4 ? q.x : i < 8 ? q.y : i < 12 ? q.z : q.w;
  return (int)((w >> (8 * (i & 3))) & 255u);
}
// pixels until the address a + ch * h is a multiple of 16 (ch = 1 or 3; 3 * 11 = 33 = 1 mod 16)
__device__ __forceinline__ int head_pixels(uintptr_t a, int ch) {
  const int m = (int)((16 - (a & 15)) & 15);
  return ch == 1 ? m : (m * 11) & 15;
}
__device__ __forceinline__ int key_at(const uint8_t* p, int ch) { return ch == 1 ? p[0] : (p[0] + 2 * p[1] + p[2] + 2) >> 2; }

// n <= 15 pixels one by one (heads, tails, reflected columns): all the loads are issued before the first add waits for one
template <typename F>
__device__ __forceinline__ void add_few(int* my, int n, F key_of) {
  int key[15];
#pragma unroll
  for (int i = 0; i < 15; ++i) key[i] = i < n ? key_of(i) : -1;
#pragma unroll
  for (int i = 0; i < 15; ++i)
    if (key[i] >= 0) atomicAdd(&my[key[i]], 1);
}

__global__ __launch_bounds__(PT) void clahe_hist_kernel(const Batch b, const int gx, int* __restrict__ hist) {
  __shared__ int s_h[4][256];
  const Image& im = b.im[blockIdx.z];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int ti = blockIdx.y % gx, tj = blockIdx.y / gx;
  const int r0 = blockIdx.x * im.seg_rows, r1 = min(r0 + im.seg_rows, im.th);   // rows of the tile, [r0, r1)
  if (r0 >= r1) return;                                                           // block-uniform
  for (int i = tid; i < 4 * 256; i += PT) (&s_h[0][0])[i] = 0;
  __syncthreads();

  const int x0 = ti * im.tw, xe = x0 + im.tw;          // columns of the extended image
  const int x1 = max(min(xe, im.W), x0);               // [x0, x1) are real, [x1, xe) reflected: a tile may lie wholly in the extension
  const int npx = x1 - x0, ch = im.ch;
  const int ipr = npx / 16 + 3;                        // pieces of a row: head, <= npx / 16 groups, tail, reflected columns
  const int rows = r1 - r0;
  int* my = s_h[wave];
  for (int w = tid; w < rows * ipr; w += PT) {
    const int row = w / ipr, piece = w - row * ipr;
    const int ry = reflect(tj * im.th + r0 + row, im.H);
    const uint8_t* line = im.src + (long)ry * im.sstride;
    const uint8_t* p = line + (long)x0 * ch;
    const int h = min(head_pixels(reinterpret_cast<uintptr_t>(p), ch), npx);
    const int nb = (npx - h) >> 4;
    if (piece >= 1 && piece <= ipr - 3) {
      if (piece <= nb) {
        const uint8_t* q = p + (long)(h + 16 * (piece - 1)) * ch;       // 16-byte aligned by the choice of h
        int key[16];
        if (ch == 1) {
          const uint4 v = *reinterpret_cast<const uint4*>(q);
#pragma unroll
          for (int i = 0; i < 16; ++i) key[i] = byte_of(v, i);
        } else {
          const uint4 v0 = reinterpret_cast<const uint4*>(q)[0], v1 = reinterpret_cast<const uint4*>(q)[1], v2 = reinterpret_cast<const uint4*>(q)[2];
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            int c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              const int at = 3 * i + k;
              c[k] = at < 16 ? byte_of(v0, at) : at < 32 ? byte_of(v1, at - 16) : byte_of(v2, at - 32);
            }
            key[i] = (c[0] + 2 * c[1] + c[2] + 2) >> 2;
          }
        }
        bool one = true;
#pragma unroll
        for (int i = 1; i < 16; ++i) one = one && key[i] == key[0];
        // the lanes here are the wave's active ones: all of them on one key is one atomic for the wave
        const int first = __builtin_amdgcn_readfirstlane(key[0]);
        if (__all(one && key[0] == first)) {
          const unsigned long long active = __ballot(1);
          if ((int)__lane_id() == __ffsll((long long)active) - 1) atomicAdd(&my[first], 16 * __popcll(active));
        } else {
          int cur = key[0], n = 1;
#pragma unroll
          for (int i = 1; i < 16; ++i) {
            if (key[i] == cur) {
              ++n;
            } else {
              atomicAdd(&my[cur], n);
              cur = key[i];
              n = 1;
            }
          }
          atomicAdd(&my[cur], n);
        }
      }
    } else if (piece == 0) {
      add_few(my, h, [&](int i) { return key_at(p + (long)i * ch, ch); });
    } else if (piece == ipr - 2) {
      add_few(my, npx - h - 16 * nb, [&](int i) { return key_at(p + (long)(h + 16 * nb + i) * ch, ch); });
    } else {
      for (int e = x1; e < xe; e += 15)                // fewer than 16 columns in all
        add_few(my, min(xe - e, 15), [&](int i) { return key_at(line + (long)reflect(e + i, im.W) * ch, ch); });
    }
  }
  __syncthreads();
  const int total = s_h[0][tid] + s_h[1][tid] + s_h[2][tid] + s_h[3][tid];
  if (total) atomicAdd(hist + ((long)im.tile0 + blockIdx.y) * 256 + tid, total);
}

__global__ __launch_bounds__(PT) void clahe_curve_kernel(const Batch b, const int* __restrict__ hist, uint8_t* __restrict__ lut) {
  __shared__ int s_part[4];
  __shared__ int s_scan[4];
  const Image& im = b.im[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long at = ((long)im.tile0 + blockIdx.x) * 256 + tid;
  const unsigned area = (unsigned)im.tw * (unsigned)im.th;
  int h = hist[at];
  if (im.clip > 0) {                                     // block-uniform
    int ex = max(h - im.clip, 0);
    h = min(h, im.clip);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) ex += __shfl_xor(ex, d);
    if (lane == 0) s_part[wave] = ex;
    __syncthreads();
    const int excess = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    h += excess >> 8;
    const int r = excess & 255;
    if (r > 0) {
      const int step = 256 / r;                          // >= 1
      if (tid % step == 0 && tid / step < r) h += 1;
    }
  }
  int c = h;                                             // inclusive scan over the 256 bins
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(c, d);
    if (lane >= d) c += up;
  }
  if (lane == 63) s_scan[wave] = c;
  __syncthreads();
  for (int k = 0; k < wave; ++k) c += s_scan[k];
  lut[at] = (uint8_t)min((510u * (unsigned)c + area) / (2u * area), 255u);   // c <= area <= 2^22: below 2^32
}

// lower edge of cell c along an axis of tile size t: the first x with floor((2 x + 1 - t) / (2 t)) == c - 1
__device__ __forceinline__ int cell_lo(int c, int t) { return c <= 0 ? 0 : ((2 * c - 1) * t) >> 1; }

// One output value from the four curves packed in `packed` and the four weights w = wy * wx.  Every multiply is a 24-bit one (full rate):
// a weight is at most 4 area <= 2^24, and equals 2^24 only if area = 2^22 with a = 0 on both axes, which needs tw and th odd -- so it is
// below 2^24; a curve value is a byte; half = 2 area <= 2^23.  n < 2^32 (the weights sum to den = 4 area, the values are <= 255).
__device__ __forceinline__ unsigned blend(unsigned packed, unsigned w00, unsigned w01, unsigned w10, unsigned w11, unsigned half, float rden) {
  const unsigned n = __umul24(w00, packed & 255u) + __umul24(w01, (packed >> 8) & 255u) + __umul24(w10, (packed >> 16) & 255u) +
                     __umul24(w11, packed >> 24) + half;
  unsigned q = min((unsigned)((float)n * rden), 255u);   // within one of n / den: the quotient is <= 255, the estimate's error far below 1
  const int r = (int)(n - (__umul24(q, half) << 1));     // n - q den, in (-den, 2 den): fits
  if (r < 0) --q;
  else if (r >= (int)(half << 1)) ++q;
  return q & 255u;                                       // a byte outside the cell (meaningless weights) must not spill into its neighbour
}

__global__ __launch_bounds__(PT) void clahe_apply_kernel(const Batch b, const int gx, const int gy, const uint8_t* __restrict__ lut) {
  __shared__ unsigned s_lut[256];
  const Image& im = b.im[blockIdx.z];
  const int tid = threadIdx.x, ch = im.ch, tw = im.tw, th = im.th;
  const int cx = blockIdx.y % (gx + 1), cy = blockIdx.y / (gx + 1);
  const int xa = cell_lo(cx, tw), xb = min(cell_lo(cx + 1, tw), im.W);
  const int ya = cell_lo(cy, th), yb = min(cell_lo(cy + 1, th), im.H);
  if (xa >= xb || ya >= yb) return;                      // block-uniform: a cell beyond the image
  const int span = (xb - xa) * ch;                       // bytes of a row of the cell
  const int chunk_rows = max(1, CHUNK_BYTES / span);
  const int r0 = ya + blockIdx.x * chunk_rows, r1 = min(r0 + chunk_rows, yb);
  if (r0 >= r1) return;                                  // block-uniform

  {
    const int tx0 = min(max(cx - 1, 0), gx - 1), tx1 = min(cx, gx - 1), ty0 = min(max(cy - 1, 0), gy - 1), ty1 = min(cy, gy - 1);
    const uint8_t* base = lut + (long)im.tile0 * 256 + tid;
    s_lut[tid] = (unsigned)base[(long)(ty0 * gx + tx0) * 256] | (unsigned)base[(long)(ty0 * gx + tx1) * 256] << 8 |
                 (unsigned)base[(long)(ty1 * gx + tx0) * 256] << 16 | (unsigned)base[(long)(ty1 * gx + tx1) * 256] << 24;
  }
  __syncthreads();

  const unsigned den = 4u * (unsigned)tw * (unsigned)th, half = den >> 1;   // half = 2 area
  const float rden = 1.0f / (float)den;
  const int ux0 = 1 - tw - (cx - 1) * 2 * tw, uy0 = 1 - th - (cy - 1) * 2 * th;   // a = 2 x + ux0 in [0, 2 tw), the same for rows
  const int ipr = (span + 15) / 16 + 1;                  // 16-byte windows of the destination that a row of the cell can touch
  const int rows = r1 - r0;
  for (int w = tid; w < rows * ipr; w += PT) {
    const int row = w / ipr, piece = w - row * ipr;
    const int y = r0 + row;
    const unsigned ay = (unsigned)(2 * y + uy0), wy0 = 2u * th - ay, wy1 = ay;
    const uint8_t* s = im.src + (long)y * im.sstride + (long)xa * ch;
    uint8_t* d = im.dst + (long)y * im.dstride + (long)xa * ch;
    const bool wide = ((reinterpret_cast<uintptr_t>(s) ^ reinterpret_cast<uintptr_t>(d)) & 15) == 0;
    const int k0 = 16 * piece - (int)(reinterpret_cast<uintptr_t>(d) & 15);   // the window holds bytes k0 .. k0 + 15 of the row of the cell
    if (k0 >= span) continue;
    const bool full = k0 >= 0 && k0 + 16 <= span;        // else only the bytes inside [0, span) are read and written
    uint4 v;
    if (full && wide) {
      v = *reinterpret_cast<const uint4*>(s + k0);
    } else {                                             // every load is issued before the first result is needed
      unsigned in[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = k0 + i;
        if (k >= 0 && k < span) in[i >> 2] |= (unsigned)s[k] << (8 * (i & 3));
      }
      v = make_uint4(in[0], in[1], in[2], in[3]);
    }
    unsigned o[4] = {0u, 0u, 0u, 0u};
    // pixel of byte k0 + i: k0 + i itself, or (k0 + i) / 3 = q3 - 16 + (r3 + i) / 3 with r3 + i < 18, where v / 3 == (11 v) >> 5
    const int q3 = (k0 + 48) / 3, r3 = k0 + 48 - 3 * q3;
#pragma unroll
    for (int i = 0; i < 16; ++i) {                       // a byte outside the cell gets weights that mean nothing and is not stored
      const int x = xa + (ch == 1 ? k0 + i : q3 - 16 + ((11 * (r3 + i)) >> 5));
      const unsigned ax = (unsigned)(2 * x + ux0) & 0xffffffu, wx0 = (2u * tw - ax) & 0xffffffu;
      o[i >> 2] |= blend(s_lut[byte_of(v, i)], __umul24(wy0, wx0), __umul24(wy0, ax), __umul24(wy1, wx0), __umul24(wy1, ax), half, rden) << (8 * (i & 3));
    }
    if (full) {
      *reinterpret_cast<uint4*>(d + k0) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = k0 + i;
        if (k >= 0 && k < span) d[k] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
      }
    }
  }
}

bool grid_ok(int gx, int gy) { return gx >= 1 && gx <= 16 && gy >= 1 && gy <= 16; }

// One item -> what the kernels read; false = MTBT_EINVAL.
bool describe(const mtbt_clahe_image& s, int gx, int gy, int tile0, Image& d) {
  if (!s.src || !s.dst || (s.channels != 1 && s.channels != 3) || s.height < gy || s.width < gx || s.clip < 0) return false;
  const int64_t row = (int64_t)s.width * s.channels;
  if (s.src_row_stride < row || s.dst_row_stride < row) return false;
  if ((int64_t)s.height * s.src_row_stride >= 0x7fffffffLL || (int64_t)s.height * s.dst_row_stride >= 0x7fffffffLL) return false;
  const int tw = (s.width + gx - 1) / gx, th = (s.height + gy - 1) / gy;
  if ((int64_t)tw * th > (1LL << 22)) return false;
  d.src = s.src; d.dst = s.dst; d.sstride = s.src_row_stride; d.dstride = s.dst_row_stride;
  d.H = s.height; d.W = s.width; d.ch = s.channels; d.clip = s.clip;
  d.tw = tw; d.th = th;
  d.seg_rows = (SEG_PIXELS + tw - 1) / tw;
  d.tile0 = tile0;
  return true;
}

// the bytes an image's rows span: [lo, hi)
void extent(const uint8_t* p, const mtbt_clahe_image& s, int64_t stride, uintptr_t& lo, uintptr_t& hi) {
  lo = reinterpret_cast<uintptr_t>(p);
  hi = lo + (uintptr_t)((int64_t)(s.height - 1) * stride + (int64_t)s.width * s.channels);
}

}  // namespace

extern "C" int mtbt_sizeof_clahe_args(int which) { return which == 0 ? (int)sizeof(mtbt_clahe_image) : -1; }

extern "C" int64_t mtbt_clahe_workspace_bytes(const mtbt_clahe_image* images, int count, int grid_x, int grid_y) {
  if (count < 0 || !grid_ok(grid_x, grid_y) || (count > 0 && !images)) return MTBT_EINVAL;
  return (int64_t)count * grid_x * grid_y * (256 * (int64_t)sizeof(int32_t) + 256);
}

extern "C" int mtbt_clahe_batch(const mtbt_clahe_image* images, int count, int grid_x, int grid_y, void* workspace, int64_t workspace_bytes,
                                void* stream) {
  if (!images || count < 0 || !grid_ok(grid_x, grid_y)) return MTBT_EINVAL;
  const int tiles = grid_x * grid_y;
  Image probe;
  for (int i = 0; i < count; ++i) {   // every item is checked before the first launch
    if (!describe(images[i], grid_x, grid_y, 0, probe)) return MTBT_EINVAL;
    uintptr_t d0, d1, s0, s1;
    extent(images[i].dst, images[i], images[i].dst_row_stride, d0, d1);
    for (int j = 0; j < count; ++j) {   // a destination may meet a source only as its own item's, exactly
      extent(images[j].src, images[j], images[j].src_row_stride, s0, s1);
      if (d0 < s1 && s0 < d1 && !(i == j && images[i].dst == images[i].src && images[i].dst_row_stride == images[i].src_row_stride)) return MTBT_EINVAL;
    }
  }
  const int64_t need = mtbt_clahe_workspace_bytes(images, count, grid_x, grid_y);
  if (need > 0 && (!workspace || workspace_bytes < need)) return MTBT_EINVAL;
  if (need > 0 && !aligned16(workspace)) return MTBT_EALIGN;
  if (count == 0) return MTBT_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int* hist = reinterpret_cast<int*>(workspace);
  uint8_t* lut = reinterpret_cast<uint8_t*>(workspace) + (int64_t)count * tiles * 256 * (int64_t)sizeof(int32_t);
  if (hipMemsetAsync(hist, 0, (size_t)count * tiles * 256 * sizeof(int32_t), s) != hipSuccess) return MTBT_ELAUNCH;
  for (int first = 0; first < count; first += MAX_IMAGES) {
    const int nb = count - first < MAX_IMAGES ? count - first : MAX_IMAGES;
    Batch b;
    int segs = 1, chunks = 1;   // the grids' x extents: the most any image of this launch needs
    for (int i = 0; i < nb; ++i) {
      Image& d = b.im[i];
      describe(images[first + i], grid_x, grid_y, (first + i) * tiles, d);
      const int sg = (d.th + d.seg_rows - 1) / d.seg_rows;
      // a cell is at most tw x th pixels and the kernel takes max(1, CHUNK_BYTES / span) rows per workgroup: the widest cell needs the most
      const int64_t span = (int64_t)d.tw * d.ch;
      const int chunk_rows = span >= CHUNK_BYTES ? 1 : (int)(CHUNK_BYTES / span);
      const int ck = (d.th + chunk_rows - 1) / chunk_rows;
      if (sg > segs) segs = sg;
      if (ck > chunks) chunks = ck;
    }
    hipLaunchKernelGGL(clahe_hist_kernel, dim3((unsigned)segs, (unsigned)tiles, (unsigned)nb), dim3(PT), 0, s, b, grid_x, hist);
    MTBT_LAUNCH_CHECK();
    hipLaunchKernelGGL(clahe_curve_kernel, dim3((unsigned)tiles, (unsigned)nb), dim3(PT), 0, s, b, hist, lut);
    MTBT_LAUNCH_CHECK();
    hipLaunchKernelGGL(clahe_apply_kernel, dim3((unsigned)chunks, (unsigned)((grid_x + 1) * (grid_y + 1)), (unsigned)nb), dim3(PT), 0, s, b, grid_x,
                       grid_y, lut);
    MTBT_LAUNCH_CHECK();
  }
  return MTBT_OK;
}
