// What the frame-mask kernels share (mask_frame.hip: mtbt_masks_to_frames, mask_vote.hip: mtbt_vote_masks): the LDS geometry, the
// per-image descriptor that travels in the kernel arguments, the bilinear tap rule and the host's choice of the tile.
#pragma once
#include "common.h"

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

// torch's align_corners=False source index for destination index d: taps i0, i1 and the weight of i1
__host__ __device__ __forceinline__ void frame_tap(int d, float step, int size, int& i0, int& i1, float& l) {
  float s = ((float)d + 0.5f) * step - 0.5f;
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

// prototype pixels spanned by any run of `len` frame pixels that starts at a multiple of `len`
inline int frame_span(int extent, int len, float step, int size) {
  int best = 0;
  for (int a = 0; a < extent; a += len) {
    const int last = (a + len < extent ? a + len : extent) - 1;
    int i0, i1, t0, t1;
    float l;
    frame_tap(a, step, size, i0, t0, l);
    frame_tap(last, step, size, t1, i1, l);
    if (i1 - i0 + 1 > best) best = i1 - i0 + 1;
  }
  return best;
}

// the largest tile (2^wl words x th rows, at most MAX_UNITS units) whose patch fits NPX_CAP; wider wins a tie (longer contiguous stores)
inline void frame_pick_tile(const mtbt_frame& fr, int hp, int wp, int& wl, int& th, int& npxp) {
  const int words_x = fr.pitch >> 3;
  int pw[4], ph[9];
  for (int l = 0; l < 4; ++l) pw[l] = (l == 0 || (1 << (l - 1)) < words_x) ? frame_span(fr.width, 64 << l, fr.step, wp) : 0;
  for (int l = 0; l < 9; ++l) ph[l] = (l == 0 || (1 << (l - 1)) < fr.height) ? frame_span(fr.height, 1 << l, fr.step, hp) : 0;
  wl = 0; th = 1; npxp = (pw[0] * ph[0] + 15) & ~15;   // a 64 x 1 tile at step <= 1: at most 66 x 2 prototype pixels
  long best = 0;
  for (int l = 3; l >= 0; --l)
    for (int h = 8; h >= 0; --h) {
      if (!pw[l] || !ph[h] || ((1 << l) << h) > MAX_UNITS) continue;
      const int n = (pw[l] * ph[h] + 15) & ~15;
      const long area = 1L << (l + h);
      if (n <= NPX_CAP && area > best) { best = area; wl = l; th = 1 << h; npxp = n; }
    }
}

// The host's share of a launch over `frames` with K planes per image: the descriptor checks of mtbt_masks_to_frames (MTBT_EINVAL), the
// tile of every image and the number of workgroups.
inline int frame_layout(const mtbt_frame* frames, int n_frames, int K, int hp, int wp, bool with_boxes, int64_t out_bytes, FrameD* f, long& blocks) {
  blocks = 0;
  for (int i = 0; i < n_frames; ++i) {
    const mtbt_frame& fr = frames[i];
    if (fr.height < 1 || fr.width < 1 || !(fr.step > 0.f && fr.step <= 1.f)) return MTBT_EINVAL;
    if (with_boxes && !(fr.scale > 0.f)) return MTBT_EINVAL;
    if ((int64_t)fr.pitch != 8 * (((int64_t)fr.width + 63) / 64)) return MTBT_EINVAL;
    if (fr.offset < 0 || fr.offset % 16) return MTBT_EINVAL;
    const int64_t bytes = (int64_t)K * fr.height * fr.pitch;
    if (fr.offset > out_bytes || bytes > out_bytes - fr.offset) return MTBT_EINVAL;
    FrameD& d = f[i];
    int npxp;
    frame_pick_tile(fr, hp, wp, d.wl, d.th, npxp);
    if (npxp > NPX_CAP) return MTBT_EINVAL;   // cannot happen for step <= 1
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

}  // namespace frame_tile
