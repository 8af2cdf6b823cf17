// The semantic mask in the original image frame: the projector's logit averaged over the sources of an image (views, models, tiles) and
// sampled at the frame's own pixels, bit-packed and optionally dense (mtbt_seg_to_frames; the definition is in include/mtbt_hip.h,
// tests/seg_frame_reference.py restates it).
//
//   L_s[y,x] = serial fp32 sum over c of q[proj_s][c] * P_s[y,x,c], then + bias                    -- seg_project_kernel, [NS, G, G] workspace
//   num, den = sums over the sources whose window holds (X, Y), ascending, of w * tap_s and w      -- seg_blend_kernel
//   v = num / den, bit = v > threshold                                                             -- packed as frame_tile.h packs
//
// seg_project_kernel streams the prototypes once: a thread owns one prototype pixel, its 128 bytes come in as eight float4 loads that are
// all in flight before the serial sum starts.  One row per source leaves the MFMA nothing to do, and the serial order can be restated
// bit for bit.
// seg_blend_kernel is the tile walk of frame_tile.h (frame tile of whole words, tile_context, patch_under, taps_at, bilinear, 8-byte word
// stores) over a patch of ONE float per prototype pixel, so the patch cap is SEG_LDS / RES pixels instead of 384: a frame tile is up to
// 4 x UW (row, word) units and up to RES sources' patches are resident between two barriers.  The host picks the tile and RES
// (seg_pick).  The sources whose window meets the frame tile are listed once per workgroup; a lane keeps num / den of its UW pixels in
// registers and walks the list ascending, which is the order the rule fixes.  The orientation of a source enters only where its patch
// is staged (stage_patch1's at(y, x)): everything after works on the upright grid.
#include "common.h"
#include "frame_tile.h"
#include "tile_check.h"

// No FMA contraction in this file (built with -ffp-contract=off, see build.py), as in mask_tiles.hip.

namespace {

using namespace frame_tile;

constexpr int UW = 8;                      // (row, word) units per wave: 2 x UW accumulators per lane
constexpr int MAX_SEG_UNITS = 4 * UW;
constexpr int SEG_LDS = 8192;              // floats of patch buffer (32 KiB: two workgroups per CU leave room to spare)
constexpr int MAX_RES = 4;                 // sources resident at once
constexpr int PROJ_NT = 256;

struct ProjectP {
  const float* protos[MTBT_SEG_MAX_PASSES];
  const float* q;
  const mtbt_seg_source* src;
  float* L;
  int s0, GG;
};

__global__ __launch_bounds__(PROJ_NT) void seg_project_kernel(const ProjectP p) {
  const int s = p.s0 + (int)blockIdx.y;
  const int px = (int)blockIdx.x * PROJ_NT + (int)threadIdx.x;
  if (px >= p.GG) return;
  const mtbt_seg_source d = p.src[s];
  const float4* in = reinterpret_cast<const float4*>(p.protos[d.pass] + ((long)d.slot * p.GG + px) * NM);
  float4 v[NM / 4];
#pragma unroll
  for (int i = 0; i < NM / 4; ++i) v[i] = in[i];
  const float* q = p.q + (long)d.proj * (NM + 1);
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < NM / 4; ++i) {
    acc = acc + q[4 * i + 0] * v[i].x;
    acc = acc + q[4 * i + 1] * v[i].y;
    acc = acc + q[4 * i + 2] * v[i].z;
    acc = acc + q[4 * i + 3] * v[i].w;
  }
  p.L[(long)s * p.GG + px] = acc + q[NM];
}

struct BlendP {
  const float* L;
  const mtbt_seg_source* src;
  const mtbt_tile* tiles;
  const float* tab;
  unsigned char* out;
  float* logits;
  float threshold;
  int n_frames, G, res, cap;   // res patches of cap floats each are resident
  int first[MAX_FRAMES + 1];
  long loff[MAX_FRAMES];
  FrameD f[MAX_FRAMES];
};

__global__ __launch_bounds__(256) void seg_blend_kernel(const BlendP p) {
  __shared__ float s_patch[SEG_LDS];
  __shared__ int s_list[MTBT_TILE_MAX_PER_IMAGE], s_nlist;
  const int tid = threadIdx.x, lane = tid & 63;
  const TileCtx c = tile_context(p.f, p.n_frames, p.out, UW);   // a run of at most UW units per wave (the host's choice of the tile)
  const int n = c.n, G = p.G;
  const int t0 = p.first[n], T = min(p.first[n + 1] - t0, MTBT_TILE_MAX_PER_IMAGE);

  // the sources whose window meets the frame tile, ascending
  if (tid == 0) {
    int m = 0;
    for (int tl = 0; tl < T; ++tl) {
      const mtbt_tile& d = p.tiles[t0 + tl];
      if (d.wx0 <= c.Xl && c.X0 < d.wx1 && d.wy0 <= c.Yl && c.Y0 < d.wy1) s_list[m++] = tl;
    }
    s_nlist = m;
  }
  __syncthreads();
  const int nlist = s_nlist;

  float num[UW], den[UW];
#pragma unroll
  for (int j = 0; j < UW; ++j) num[j] = den[j] = 0.f;

  for (int l0 = 0; l0 < nlist; l0 += p.res) {
    const int nr = min(p.res, nlist - l0);
    // the patches of the next nr sources: the part of the frame tile each window holds, and the upright prototype pixels under it
    for (int r = 0; r < nr; ++r) {
      const int s = t0 + s_list[l0 + r];
      const mtbt_tile& d = p.tiles[s];
      const int o = p.src[s].orient;
      const int ix0 = max(c.X0, d.wx0), ix1 = min(c.Xl, d.wx1 - 1), iy0 = max(c.Y0, d.wy0), iy1 = min(c.Yl, d.wy1 - 1);
      const Patch pt = patch_under(ix0, ix1, iy0, iy1, d.step, d.pox, d.poy, G, G);
      if (pt.NPX <= p.cap)   // (always, by the host's choice of the frame tile; a patch that did not fit is never read)
        stage_patch1(s_patch + r * p.cap, p.L + (long)s * G * G, pt, [&](int y, int x) {   // upright prototype pixel (y, x) ...
          const int a = (o & 4) ? x : y, b = (o & 4) ? y : x;                              // ... in the view: row a, column b, then the flips
          const int sy = (o & 2) ? G - 1 - a : a, sx = (o & 1) ? G - 1 - b : b;
          return (long)sy * G + sx;
        });
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
      const int s = t0 + s_list[l0 + r];
      const mtbt_tile& d = p.tiles[s];
      const mtbt_seg_source& sd = p.src[s];
      const float step = d.step, weight = sd.weight;
      const int pox = d.pox, poy = d.poy;
      const bool blend = sd.blend != 0;
      const int ix0 = max(c.X0, d.wx0), ix1 = min(c.Xl, d.wx1 - 1), iy0 = max(c.Y0, d.wy0), iy1 = min(c.Yl, d.wy1 - 1);
      const Patch pt = patch_under(ix0, ix1, iy0, iy1, step, pox, poy, G, G);
      if (pt.NPX > p.cap) continue;
      const float* patch = s_patch + r * p.cap;
      // sampling at this source's own tap positions; a lane outside the window taps the nearest pixel inside it and drops the value
#pragma unroll
      for (int j = 0; j < UW; ++j) {
        const int u = c.u0 + j, row = u >> c.wl, wd = u & (c.wt - 1);
        const int Y = c.Y0 + row, Xw = c.X0 + wd * 64, X = Xw + lane;
        if (j < c.un && wd < c.nwx && Y >= iy0 && Y <= iy1 && Xw <= ix1 && Xw + 63 >= ix0) {   // wave-uniform
          const bool inw = X >= ix0 && X <= ix1;
          const int Xc = min(max(X, ix0), ix1);
          const Taps t = taps_at(Xc, Y, step, pox, poy, G, G, pt);
          const float tap = bilinear(patch, t);
          float bx = 1.f, by = 1.f;
          if (blend) {
            int x0, x1, y0, y1;
            float lx, ly;
            frame_tap(Xc, step, pox, G, x0, x1, lx);
            frame_tap(Y, step, poy, G, y0, y1, ly);
            bx = (1.f - lx) * p.tab[x0] + lx * p.tab[x1];
            by = (1.f - ly) * p.tab[y0] + ly * p.tab[y1];
          }
          const float w = weight * (bx * by);
          if (inw) {
            num[j] = num[j] + w * tap;
            den[j] = den[j] + w;
          }
        }
      }
    }
    __syncthreads();   // the patches are rewritten for the next sources
  }

  // one ballot per unit: the ballot of the wave's unit j is kept by lane j; a lane stores its own v
  unsigned long long word = 0ull;
  float* lg = p.logits ? p.logits + p.loff[n] : nullptr;
#pragma unroll
  for (int j = 0; j < UW; ++j) {
    const int u = c.u0 + j, row = u >> c.wl, wd = u & (c.wt - 1);
    const int Y = c.Y0 + row, X = c.X0 + wd * 64 + lane;
    if (j < c.un && wd < c.nwx) {
      const bool seen = den[j] > 0.f;
      const float v = seen ? __fdiv_rn(num[j], den[j]) : 0.f;
      const bool in = X < c.W0;
      const unsigned long long mk = __ballot(in && seen && v > p.threshold);
      if (lane == j) word = mk;
      if (lg && in) lg[(long)Y * c.W0 + X] = v;
    }
  }
  if (c.my_store) *reinterpret_cast<unsigned long long*>(c.my_out) = word;
}

// the frame tiles and the residency: the most sources resident under which every image still gets the largest tile it could have alone
int seg_pick(const mtbt_frame* frames, int n_frames, int G, int64_t out_bytes, const mtbt_tile* tiles, const int32_t* first, BlendP& p,
             long& blocks) {
  int rc = MTBT_OK;
  long full = 0;
  {
    FrameD f1[MAX_FRAMES];
    rc = frame_layout(frames, n_frames, 1, G, G, false, out_bytes, tiles, first, MAX_SEG_UNITS, 5, f1, blocks, SEG_LDS, true);
    if (rc) return rc;
    for (int i = 0; i < n_frames; ++i) full += (long)f1[i].th << f1[i].wl;
  }
  for (int res = MAX_RES; res >= 1; res >>= 1) {
    rc = frame_layout(frames, n_frames, 1, G, G, false, out_bytes, tiles, first, MAX_SEG_UNITS, 5, p.f, blocks, SEG_LDS / res, true);
    if (rc) return rc;
    long area = 0;
    for (int i = 0; i < n_frames; ++i) area += (long)p.f[i].th << p.f[i].wl;
    p.res = res; p.cap = SEG_LDS / res;
    if (area == full) break;
  }
  return MTBT_OK;
}

}  // namespace

extern "C" int mtbt_sizeof_seg_frame_args(int which) {
  switch (which) {
    case 0: return (int)sizeof(mtbt_seg_source);
    case 1: return (int)sizeof(mtbt_seg_frame_args);
    default: return -1;
  }
}

extern "C" int64_t mtbt_seg_frame_workspace_bytes(int n_sources, int G) {
  if (n_sources < 1 || G < 1) return 0;
  return (int64_t)n_sources * G * G * (int64_t)sizeof(float);
}

extern "C" int mtbt_seg_to_frames(const mtbt_seg_frame_args* a, const mtbt_frame* frames, int n_frames, void* stream) {
  if (!a || !frames || !a->proj || !a->sources || !a->sources_dev || !a->tiles || !a->tiles_dev || !a->first || !a->workspace || !a->out)
    return MTBT_EINVAL;
  if (a->n_passes < 1 || a->n_passes > MTBT_SEG_MAX_PASSES) return MTBT_EINVAL;
  for (int i = 0; i < a->n_passes; ++i)
    if (!a->protos[i] || a->pass_items[i] < 1) return MTBT_EINVAL;
  if (!frame_args_ok(n_frames, a->N, a->nm, 1, a->hp, a->wp, a->out_bytes)) return MTBT_EINVAL;
  if (a->hp != a->wp || a->hp > 32768 || a->n_proj < 1 || a->reserved != 0 || a->n_sources < 0) return MTBT_EINVAL;
  const int N = a->N, G = a->hp;
  if (a->first[0] < 0) return MTBT_EINVAL;
  for (int n = 0; n < N; ++n) {
    const int T = a->first[n + 1] - a->first[n];
    if (T < 0 || T > MTBT_TILE_MAX_PER_IMAGE || a->first[n + 1] > a->n_sources) return MTBT_EINVAL;
  }
  const int s0 = a->first[0], s1 = a->first[N];
  bool any_blend = false;
  for (int s = s0; s < s1; ++s) {
    const mtbt_seg_source& d = a->sources[s];
    if (d.pass < 0 || d.pass >= a->n_passes || d.slot < 0 || d.slot >= a->pass_items[d.pass]) return MTBT_EINVAL;
    if (d.orient < 0 || d.orient > 7 || !(d.weight > 0.f) || !(d.weight <= 3.4028234e38f)) return MTBT_EINVAL;
    if (d.proj < 0 || d.proj >= a->n_proj || d.blend < 0 || d.blend > 1 || d.reserved[0] != 0 || d.reserved[1] != 0) return MTBT_EINVAL;
    if (d.blend && !(a->tab && a->tab_dev)) return MTBT_EINVAL;
    any_blend = any_blend || d.blend;
  }
  if (a->tab)
    for (int i = 0; i < G; ++i)
      if (!(a->tab[i] > 0.f) || !(a->tab[i] <= 3.4028234e38f)) return MTBT_EINVAL;
  if (a->threshold != a->threshold) return MTBT_EINVAL;
  if (a->workspace_bytes < mtbt_seg_frame_workspace_bytes(a->n_sources > 0 ? a->n_sources : 1, G) || a->workspace_bytes < (int64_t)s1 * G * G * 4)
    return MTBT_EINVAL;
  int Tbig = 0;
  if (int rc = tile_check::check_table(a->tiles, a->first, N, a->n_sources, 1, MTBT_TILE_MAX_PER_IMAGE, false, frames, Tbig)) return rc;
  BlendP p;
  long blocks = 0;
  if (int rc = seg_pick(frames, n_frames, G, a->out_bytes, a->tiles, a->first, p, blocks)) return rc;
  if (a->logits) {
    if (a->logits_floats < 0) return MTBT_EINVAL;
    for (int n = 0; n < N; ++n) {
      const int64_t off = a->logits_offset[n], px = (int64_t)frames[n].height * frames[n].width;
      if (off < 0 || off % 4 || off > a->logits_floats || px > a->logits_floats - off) return MTBT_EINVAL;
    }
  }
  for (int i = 0; i < a->n_passes; ++i)
    if (!aligned16(a->protos[i])) return MTBT_EALIGN;
  if (!aligned16(a->out) || !aligned16(a->workspace) || !aligned16(a->logits)) return MTBT_EALIGN;

  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (s1 > s0) {
    ProjectP j;
    for (int i = 0; i < MTBT_SEG_MAX_PASSES; ++i) j.protos[i] = i < a->n_passes ? a->protos[i] : nullptr;
    j.q = a->proj; j.src = a->sources_dev; j.L = a->workspace; j.s0 = s0; j.GG = G * G;
    // (at most 32 x 64 sources per call: inside the grid's y range)
    hipLaunchKernelGGL(seg_project_kernel, dim3((unsigned)((j.GG + PROJ_NT - 1) / PROJ_NT), (unsigned)(s1 - s0)), dim3(PROJ_NT), 0, st, j);
    MTBT_LAUNCH_CHECK();
  }
  p.L = a->workspace; p.src = a->sources_dev; p.tiles = a->tiles_dev; p.tab = any_blend ? a->tab_dev : nullptr;
  p.out = a->out; p.logits = a->logits; p.threshold = a->threshold; p.n_frames = n_frames; p.G = G;
  for (int n = 0; n <= MAX_FRAMES; ++n) p.first[n] = a->first[n < n_frames ? n : n_frames];
  for (int n = 0; n < MAX_FRAMES; ++n) p.loff[n] = a->logits && n < n_frames ? (long)a->logits_offset[n] : 0;
  hipLaunchKernelGGL(seg_blend_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}
