// The body of the frame-mask family: bit-packed instance masks in the ORIGINAL image frame, written by mask_frame.hip
// (mtbt_masks_to_frames), mask_vote.hip (mtbt_vote_masks) and mask_tiles.hip (mtbt_vote_tile_masks).  Those files keep their parameter
// struct, how a group's `low` is produced and the entry point; the tile walk, the tap rule, the sampler, the stores and the host's share
// are here, once.
//
//   low[k][y][x] = sum_c coeff[k][c] * protos[y][x][c]                   -- MFMA, exact fp32 (v_mfma_f32_16x16x4_f32), as mask_mfma.hip
//   bit(k, Y, X) = bilinear(low[k])(X, Y) > 0  (&& inside the frame box when cropping)
//
// The bilinear taps are taken at the ORIGINAL pixel positions in one step (torch's align_corners=False rule with
// step = scale / up prototype pixels per frame pixel): no letterboxed S x S plane exists in between.  All coordinate
// and box arithmetic is separate fp32 multiplies and adds so that it rounds like the CPU restatements in tests/frame_reference.py,
// tests/vote_reference.py and tests/slice_reference.py.  INCLUDE THIS HEADER ONLY FROM FILES BUILT WITH -ffp-contract=off (build.py
// EXTRA_FLAGS: the three files above and seg_frame.hip, which walks the same tiles for the semantic mask): contracted into FMAs the taps and the bilinear value round differently.
//
// A workgroup owns one tile of one image: 2^wl 64-pixel words wide and th rows tall, both picked per image on the host
// (frame_pick_tile) so that the prototype patch under the tile (first tap of the first pixel .. second tap of the last) fits
// the LDS patch buffer.  Tiles are whole words wide and every word of a plane belongs to exactly one tile, so no two
// workgroups write the same byte and every byte of every plane is written: no pre-zero pass, no atomics.
//   1. the patch is staged in LDS (stage_patch; lazily: with cropping only when a box group touches the tile, group_hit);
//   2. boxes are processed 16 at a time: coefficients [16 x 32] x patch [32 x NPX] on the fp32 MFMA -> low in LDS
//      (coef_fragment, mfma_columns, spill_low);
//   3. the tile is cut into (row, word) units; a wave takes a run of consecutive units (tile_context).  A lane owns pixel
//      64 * word + lane of the row, evaluates the four taps for each of the 16 boxes (taps_at, bilinear) and the wave's ballot is the
//      row's 8-byte word.  The ballot of the wave's unit j is kept by lane j (sample_words), and one store per box writes the whole run
//      (store_words: consecutive words of a row are consecutive in memory).
// With cropping a (unit, box) pair whose word lies wholly outside the box costs nothing but the zero it stores, and a
// group of 16 boxes that all miss the tile skips the MFMA phase too.  Planes k >= counts[n] are zero-filled (zero_tail).
#pragma once
#include "bitplane.h"

namespace frame_tile {

constexpr int MAX_FRAMES = 32;   // images per launch (descriptors travel as kernel arguments)
constexpr int NM = 32;           // prototype channels
constexpr int PPITCH = NM + 1;   // patch row pitch (floats): conflict-free column reads
constexpr int NPX_CAP = 384;     // prototype pixels of a tile's patch: 2 workgroups per CU (77 KiB of LDS each)
constexpr int LPITCH = NPX_CAP + 4;   // row pitch of `low` (floats).  Compile-time: a box's row is an immediate offset of the tap reads
constexpr int MAX_UNITS = 256;   // (row, word) units per tile: 4 waves x 64 lanes
constexpr size_t FRAME_LDS = (size_t)(NPX_CAP * PPITCH + 16 * PPITCH + 16 * LPITCH + 64) * sizeof(float);

struct FrameD {
  long offset;          // byte offset of the image's planes in `out`
  float step, scale;
  int H0, W0, pitch;
  int wl, th;           // tile: 2^wl words x th rows
  int tiles_x, blk0;    // tiles per row of tiles; first workgroup of this image
  int pad_;
};

// torch's align_corners=False source index for destination index d: taps i0, i1 and the weight of i1.  `po`: the grid starts that many
// prototype pixels into the pass (a tile of sliced inference; 0 otherwise, and subtracting 0.f is exact)
__host__ __device__ __forceinline__ void frame_tap(int d, float step, int po, int size, int& i0, int& i1, float& l) {
  float s = ((float)d + 0.5f) * step - 0.5f - (float)po;
  s = s > 0.f ? s : 0.f;
  const int i = (int)s;
  i0 = i < size - 1 ? i : size - 1;
  i1 = i0 + 1 < size - 1 ? i0 + 1 : size - 1;
  float w = s - (float)i0;
  w = w > 0.f ? w : 0.f;
  l = w < 1.f ? w : 1.f;
}

// boxes[k] / scale clamped to the frame: component c of an xyxy box
__device__ __forceinline__ float frame_box(float v, float scale, int c, int H0, int W0) {
  const float hi = (float)((c & 1) ? H0 : W0);
  const float q = __fdiv_rn(v, scale);
  return fminf(fmaxf(q, 0.f), hi);
}

// ---- host: the tile of every image --------------------------------------------------------------------------------------------------

// prototype pixels spanned along one axis by any run of `len` frame pixels that starts at a multiple of `len`, cut to the window [w0, w1)
inline int frame_span(int len, int w0, int w1, float step, int po, int size) {
  int best = 0;
  for (int a = (w0 / len) * len; a < w1; a += len) {
    const int lo = a > w0 ? a : w0, hi = (a + len < w1 ? a + len : w1) - 1;
    int i0, i1, t0, t1;
    float l;
    frame_tap(lo, step, po, size, i0, t0, l);
    frame_tap(hi, step, po, size, t1, i1, l);
    if (i1 - i0 + 1 > best) best = i1 - i0 + 1;
  }
  return best;
}

// the largest tile (2^wl words x th rows, at most max_units units and 2^max_hl rows) under which the patch of every one of the T windows
// (each with its own step and prototype offset) fits NPX_CAP; wider wins a tie (longer contiguous stores).  False when not even a
// 64 x 1 tile fits, which cannot happen for step <= 1 (at most 66 x 2 prototype pixels); wl = 0, th = 1 then.
// `cap`: the patch buffer in prototype pixels (NPX_CAP for the instance kernels; seg_frame.hip keeps one float per pixel and passes its own).
// `snug`: among the largest tiles the one that pads the plane least wins instead (units of tiles that hang over the right or bottom
// edge are idle lanes: a 10-word row under 8-word tiles runs at 10 / 16), wider only among equals.
inline bool frame_pick_tile(const mtbt_frame& fr, const mtbt_tile* win, int T, int hp, int wp, int max_units, int max_hl, int& wl, int& th,
                            int cap = NPX_CAP, bool snug = false) {
  const int words_x = fr.pitch >> 3;
  wl = 0; th = 1;
  long best = 0, best_padded = 0;
  for (int l = 3; l >= 0; --l)
    for (int h = max_hl; h >= 0; --h) {
      if (((1 << l) << h) > max_units || (l > 0 && (1 << (l - 1)) >= words_x) || (h > 0 && (1 << (h - 1)) >= fr.height)) continue;
      const long area = 1L << (l + h);
      const long padded = (long)(((words_x + (1 << l) - 1) >> l) << l) * (((fr.height + (1 << h) - 1) >> h) << h);
      if (area < best || (area == best && !(snug && padded < best_padded))) continue;
      bool fits = true;
      for (int t = 0; t < T && fits; ++t) {
        const mtbt_tile& d = win[t];
        const int n = frame_span(64 << l, d.wx0, d.wx1, d.step, d.pox, wp) * frame_span(1 << h, d.wy0, d.wy1, d.step, d.poy, hp);
        fits = ((n + 15) & ~15) <= cap;
      }
      if (fits) { best = area; best_padded = padded; wl = l; th = 1 << h; }
    }
  return best > 0;
}

// The host's share of a launch over `frames` with K planes per image: the descriptor checks (MTBT_EINVAL), the tile of every image and the
// number of workgroups.  Without `tiles` an image is one window, the frame at its own step; with them (sliced inference: image i's windows
// are tiles[first[i] .. first[i + 1])) the frame's own step and scale are not used, every tile carries its own.
inline int frame_layout(const mtbt_frame* frames, int n_frames, int K, int hp, int wp, bool with_boxes, int64_t out_bytes,
                        const mtbt_tile* tiles, const int32_t* first, int max_units, int max_hl, FrameD* f, long& blocks, int cap = NPX_CAP,
                        bool snug = false) {
  blocks = 0;
  for (int i = 0; i < n_frames; ++i) {
    const mtbt_frame& fr = frames[i];
    if (fr.height < 1 || fr.width < 1 || (!tiles && !(fr.step > 0.f && fr.step <= 1.f))) return MTBT_EINVAL;
    if (with_boxes && !(fr.scale > 0.f)) return MTBT_EINVAL;
    if (!plane_pitch_ok(fr.width, fr.pitch)) return MTBT_EINVAL;
    if (fr.offset < 0 || fr.offset % 16) return MTBT_EINVAL;
    const int64_t bytes = (int64_t)K * fr.height * fr.pitch;
    if (fr.offset > out_bytes || bytes > out_bytes - fr.offset) return MTBT_EINVAL;
    FrameD& d = f[i];
    mtbt_tile own = {};
    own.wx1 = fr.width; own.wy1 = fr.height; own.step = fr.step;
    const bool fits = tiles ? frame_pick_tile(fr, tiles + first[i], first[i + 1] - first[i], hp, wp, max_units, max_hl, d.wl, d.th, cap, snug)
                            : frame_pick_tile(fr, &own, 1, hp, wp, max_units, max_hl, d.wl, d.th, cap, snug);
    if (!fits && !tiles) return MTBT_EINVAL;   // (the tile kernel never reads a patch that did not fit)
    d.offset = fr.offset; d.step = fr.step; d.scale = fr.scale;
    d.H0 = fr.height; d.W0 = fr.width; d.pitch = fr.pitch; d.pad_ = 0;
    const int words_x = fr.pitch >> 3;
    d.tiles_x = (words_x + (1 << d.wl) - 1) >> d.wl;
    d.blk0 = (int)blocks;
    blocks += (long)d.tiles_x * ((fr.height + d.th - 1) / d.th);
    if (blocks > 0x7fffffffL) return MTBT_EINVAL;
  }
  return MTBT_OK;
}

// the argument checks the three entry points share (`planes` per image; MTBT_EINVAL when false)
inline bool frame_args_ok(int n_frames, int N, int nm, int planes, int hp, int wp, int64_t out_bytes) {
  return n_frames >= 1 && n_frames <= MAX_FRAMES && n_frames == N && nm == NM && planes >= 1 && planes <= 65535 && hp >= 1 && wp >= 1 &&
         out_bytes >= 0;
}

// one launch of a mask kernel (the caller picks the CROP instantiation): 256 threads per tile, FRAME_LDS of dynamic LDS
template <class P>
inline int launch_mask_kernel(void (*kernel)(const P), long blocks, const P& p, hipStream_t s) {
  if (int rc = mtbt_allow_lds(kernel, (int)FRAME_LDS)) return rc;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), FRAME_LDS, s, p);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}

// ---- device: the pieces of a mask kernel --------------------------------------------------------------------------------------------

// the LDS of a workgroup
struct Lds {
  float* patch;   // [NPX_CAP][PPITCH]
  float* coef;    // [16][PPITCH]
  float* low;     // [16][LPITCH]
  float* boxs;    // [16][4] frame boxes of the group
};
__device__ __forceinline__ Lds lds_layout(char* smem) {
  Lds s;
  s.patch = reinterpret_cast<float*>(smem);
  s.coef = s.patch + NPX_CAP * PPITCH;
  s.low = s.coef + 16 * PPITCH;
  s.boxs = s.low + 16 * LPITCH;
  return s;
}

// a workgroup's tile and a wave's share of it
struct TileCtx {
  int n, t, tx;                         // image; tile of the image, its column of tiles
  int H0, W0, wl, wt;
  int X0, Y0, Xl, Yl;                   // first and last pixel of the tile
  int nwx, nrows;                       // words and rows of the tile inside the frame
  int u0, un;                           // units of this wave: u = row * wt + word, a run of un consecutive ones from u0
  bool my_store;                        // lane j keeps (and stores) unit u0 + j
  unsigned char* my_out;
  long plane;
};

// `unit_cap`: at most that many units per wave by the host's choice of the tile (0: the 64 a wave can keep)
__device__ __forceinline__ TileCtx tile_context(const FrameD* fs, int n_frames, unsigned char* out, int unit_cap) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  TileCtx c;
  c.n = 0;
  for (int i = 1; i < n_frames; ++i)
    if ((int)blockIdx.x >= fs[i].blk0) c.n = i;
  const FrameD& f = fs[c.n];
  c.H0 = f.H0; c.W0 = f.W0; c.wl = f.wl; c.wt = 1 << f.wl;
  c.t = (int)blockIdx.x - f.blk0;
  const int ty = c.t / f.tiles_x;
  c.tx = c.t - ty * f.tiles_x;
  c.X0 = c.tx * 64 * c.wt; c.Y0 = ty * f.th;
  c.Xl = min(c.X0 + 64 * c.wt, c.W0) - 1; c.Yl = min(c.Y0 + f.th, c.H0) - 1;
  const int words_x = f.pitch >> 3;
  c.nwx = min(c.wt, words_x - c.tx * c.wt); c.nrows = c.Yl - c.Y0 + 1;
  const int U = c.nrows << c.wl;
  int upw = (U + 3) >> 2;
  if (unit_cap) upw = min(upw, unit_cap);
  c.u0 = wave * upw;
  c.un = max(min(upw, U - c.u0), 0);
  const int my_u = c.u0 + lane, my_row = my_u >> c.wl, my_word = my_u & (c.wt - 1);
  c.my_store = lane < c.un && my_word < c.nwx;
  c.my_out = out + f.offset + (long)(c.Y0 + my_row) * f.pitch + (long)(c.tx * c.wt + my_word) * 8;
  c.plane = (long)c.H0 * f.pitch;
  return c;
}

// boxes in the frame: written once per image, by its first tile
__device__ __forceinline__ void write_frame_boxes(const TileCtx& c, const FrameD& f, const float* boxes, float* boxes_frame, int K, int cnt) {
  if (c.t == 0 && boxes_frame) {
    for (int i = threadIdx.x; i < K * 4; i += 256) {
      const long at = (long)c.n * K * 4 + i;
      boxes_frame[at] = (i >> 2) < cnt ? frame_box(boxes[at], f.scale, i & 3, c.H0, c.W0) : 0.f;
    }
  }
}

// the crop rule: does the xyxy box touch the pixels [xa, xe] x [ya, ye] ...
__device__ __forceinline__ bool box_touches(const float* box, float xa, float xe, float ya, float ye) {
  const float x1 = box[0], y1 = box[1], x2 = box[2], y2 = box[3];
  return (x1 <= xe) & (xa < x2) & (y1 <= ye) & (ya < y2);   // (&, not &&: four compares and no branch)
}
// ... and is pixel column x inside it
__device__ __forceinline__ bool box_holds_x(const float* box, float x) {
  const float x1 = box[0], x2 = box[2];
  return (x1 <= x) & (x < x2);
}

// With cropping: thread tid < 64 stages component tid & 3 of box tid >> 2 of the group (`v`), a barrier publishes the boxes (and whatever
// else the caller wrote to LDS), and the result is whether any of the nb boxes touches the tile (workgroup-uniform).  Without: true,
// and no barrier.
template <bool CROP>
__device__ __forceinline__ bool group_hit(const TileCtx& c, float* boxs, float v, int nb) {
  if (!CROP) return true;
  if (threadIdx.x < 64) boxs[threadIdx.x] = v;
  __syncthreads();
  bool ghit = false;
  for (int b = 0; b < nb; ++b) ghit = ghit || box_touches(boxs + b * 4, (float)c.X0, (float)c.Xl, (float)c.Y0, (float)c.Yl);
  return ghit;
}

// the prototype pixels under a rectangle of frame pixels: first tap of the first pixel .. second tap of the last
struct Patch {
  int pxa, pya, PW;
  int NPX, NPXP;   // pixels; rounded up to the MFMA's 16 and cut to NPX_CAP (NPX <= NPX_CAP by the host's choice of the tile)
};
__device__ __forceinline__ Patch patch_under(int xa, int xe, int ya, int ye, float step, int pox, int poy, int hp, int wp) {
  Patch pt;
  int pxb, pyb, tmp;
  float ftmp;
  frame_tap(xa, step, pox, wp, pt.pxa, tmp, ftmp);
  frame_tap(xe, step, pox, wp, tmp, pxb, ftmp);
  frame_tap(ya, step, poy, hp, pt.pya, tmp, ftmp);
  frame_tap(ye, step, poy, hp, tmp, pyb, ftmp);
  pt.PW = pxb - pt.pxa + 1;
  pt.NPX = pt.PW * (pyb - pt.pya + 1);
  pt.NPXP = min((pt.NPX + 15) & ~15, NPX_CAP);
  return pt;
}

// patch[px][32] <- the image's prototypes `pr` ([.][32] floats); at(y, x) is the pixel index in `pr` of upright prototype pixel (y, x)
template <class At>
__device__ __forceinline__ void stage_patch(float* patch, const float* pr, const Patch& pt, At at) {
  for (int i = threadIdx.x; i < pt.NPXP * (NM / 4); i += 256) {
    const int px = i >> 3, c4 = i & 7;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (px < pt.NPX) {
      const int py = px / pt.PW, pxx = px - py * pt.PW;
      v = *reinterpret_cast<const float4*>(pr + at(pt.pya + py, pt.pxa + pxx) * NM + c4 * 4);
    }
    float* d = patch + px * PPITCH + c4 * 4;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
}

// the same walk for a plane that holds ONE float per prototype pixel (seg_frame.hip: the projector's logits): patch[px] <- lo[at(y, x)]
template <class At>
__device__ __forceinline__ void stage_patch1(float* patch, const float* lo, const Patch& pt, At at) {
  for (int px = threadIdx.x; px < pt.NPX; px += 256) {
    const int py = px / pt.PW, pxx = px - py * pt.PW;
    patch[px] = lo[at(pt.pya + py, pt.pxa + pxx)];
  }
}

// low[16][NPXP] = coef[16][32] x patch^T on the fp32 MFMA, in column groups of 16 prototype pixels; wave w takes groups w, w + 4, ...
__device__ __forceinline__ void coef_fragment(const float* coef, float (&a)[8]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) a[ks] = coef[(lane & 15) * PPITCH + ks * 4 + (lane >> 4)];
}
__device__ __forceinline__ void mfma_columns(const float* patch, const float (&a)[8], int pg, f32x4& acc) {
  const int lane = threadIdx.x & 63;
  const float* bp = patch + (pg * 16 + (lane & 15)) * PPITCH + (lane >> 4);
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks], bp[ks * 4], acc, 0, 0, 0);
}
__device__ __forceinline__ void spill_low(float* low, int pg, const f32x4& acc) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int r = 0; r < 4; ++r) low[(4 * (lane >> 4) + r) * LPITCH + pg * 16 + (lane & 15)] = acc[r];
}
// one source: a dynamic loop over the wave's column groups (unrolled it would hold every group's accumulators)
__device__ __forceinline__ void mfma_to_low(const Lds& s, int NPXP) {
  float a[8];
  coef_fragment(s.coef, a);
  for (int pg = threadIdx.x >> 6; pg < NPXP / 16; pg += 4) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    mfma_columns(s.patch, a, pg, acc);
    spill_low(s.low, pg, acc);
  }
}

// the four taps of frame pixel (X, Y), as indices into a row of `low` over the patch, and their weights
struct Taps {
  int i00, i01, i10, i11;
  float lx, ly, wx0, wy0;
};
__device__ __forceinline__ Taps taps_at(int X, int Y, float step, int pox, int poy, int hp, int wp, const Patch& pt) {
  Taps t;
  int x0, x1, y0, y1;
  frame_tap(X, step, pox, wp, x0, x1, t.lx);
  frame_tap(Y, step, poy, hp, y0, y1, t.ly);
  t.wx0 = 1.f - t.lx; t.wy0 = 1.f - t.ly;
  t.i00 = (y0 - pt.pya) * pt.PW + (x0 - pt.pxa); t.i01 = (y0 - pt.pya) * pt.PW + (x1 - pt.pxa);
  t.i10 = (y1 - pt.pya) * pt.PW + (x0 - pt.pxa); t.i11 = (y1 - pt.pya) * pt.PW + (x1 - pt.pxa);
  return t;
}
__device__ __forceinline__ float bilinear(const float* l, const Taps& t) {
  return t.wy0 * (t.wx0 * l[t.i00] + t.lx * l[t.i01]) + t.ly * (t.wx0 * l[t.i10] + t.lx * l[t.i11]);
}

// Is box b of the group sampled for the word [Xw, Xw + 63] of row Y (wave-uniform)?  Without cropping all 16 are (a slot past nb has zero
// coefficients: v = 0, no bit), so the 64 tap reads of a unit are independent and issue together; with it a word wholly outside the box
// stays zero.
template <bool CROP>
__device__ __forceinline__ bool word_hit(const float* boxs, int b, int nb, int Xw, int Y, int W0) {
  if (!CROP) return true;
  const bool touches = box_touches(boxs + b * 4, (float)Xw, (float)min(Xw + 63, W0 - 1), (float)Y, (float)Y);
  return (b < nb) & touches;
}

// sampling of one `low`: one ballot per (unit, box); the ballot of the wave's unit j is kept by lane j
template <bool CROP>
__device__ __forceinline__ void sample_words(const TileCtx& c, const Lds& s, const Patch& pt, float step, int hp, int wp, int nb,
                                             unsigned long long (&word)[16]) {
  const int lane = threadIdx.x & 63;
  for (int j = 0; j < c.un; ++j) {
    const int u = c.u0 + j, row = u >> c.wl, wd = u & (c.wt - 1);
    if (wd >= c.nwx) continue;
    const int Y = c.Y0 + row, Xw = c.X0 + wd * 64, X = Xw + lane;
    const bool valid = X < c.W0;
    const Taps t = taps_at(min(X, c.W0 - 1), Y, step, 0, 0, hp, wp, pt);
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const bool hit = word_hit<CROP>(s.boxs, b, nb, Xw, Y, c.W0);
      bool in = valid;
      if (CROP) in = in && box_holds_x(s.boxs + b * 4, (float)X);
      if (hit) {
        const float v = bilinear(s.low + b * LPITCH, t);   // before the test of `in`: the tap reads are unconditional
        const unsigned long long m = __ballot(in && v > 0.f);
        if (lane == j) word[b] = m;
      }
    }
  }
}

// the group's words: one 8-byte store per box writes the wave's whole run ...
__device__ __forceinline__ void store_words(const TileCtx& c, const unsigned long long (&word)[16], int g0, int nb) {
  if (c.my_store) {
#pragma unroll
    for (int b = 0; b < 16; ++b)
      if (b < nb) *reinterpret_cast<unsigned long long*>(c.my_out + (long)(g0 + b) * c.plane) = word[b];
  }
}
// ... and planes k >= cnt: zeros
__device__ __forceinline__ void zero_tail(const TileCtx& c, int cnt, int K) {
  if (c.my_store)
    for (int k = cnt; k < K; ++k) *reinterpret_cast<unsigned long long*>(c.my_out + (long)k * c.plane) = 0ull;
}

}  // namespace frame_tile
