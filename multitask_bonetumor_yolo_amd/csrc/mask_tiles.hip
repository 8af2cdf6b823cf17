// Instance masks of merged rows of sliced inference, voted across the tiles of their members straight into the bit-packed frame planes
// (mtbt_vote_tile_masks; the definition is in include/mtbt_hip.h, tests/slice_reference.py restates it).
//
//   W[n,r,tl,:] = (sum over row r's members in tile tl of s_c * coeff_c[:]) / Ss[n,r]     -- tile_coeff_kernel (vote_coeff.h)
//   low_t       = W[n,r,tl,:] . P_t                                                        -- tile_mask_kernel: fp32 MFMA per (row group, tile)
//   v(Y,X)      = sum over the tiles whose window holds (X, Y), ascending, of bilinear(low_t) at the tile's own tap position
//   bit         = v > 0 (&& inside the merged box when cropping)                           -- packed as frame_tile.h packs
//
// tile_mask_kernel is the tile walk of frame_tile.h: its frame tile (words x rows), LDS layout, MFMA phase, taps and 8-byte stores.  Unlike
// mask_vote.hip the sources sample at DIFFERENT positions, so the sum over tiles happens after the tap, in registers: a wave carries at
// most UW (unit, 16 rows) accumulator sets, i.e. the frame tile is at most 4 UW units, picked on the host so that the prototype patch of
// every tile under (frame tile x that tile's window) fits the patch buffer.  Per (row group, tile): the tiles whose window misses the frame
// tile are never looked at (a list built once per workgroup), a pair whose 16 x 32 coefficients are all zero -- no member of the 16 rows
// in that tile -- is skipped, and the patch in LDS is kept while the next pair needs the same tile.
#include "common.h"
#include "frame_tile.h"
#include "tile_check.h"
#include "vote_coeff.h"

// No FMA contraction in this file (built with -ffp-contract=off, see build.py), as in mask_frame.hip and mask_vote.hip.

namespace {

using namespace frame_tile;

constexpr int UW = 4;          // (row, word) units per wave: UW x 16 accumulators per lane
constexpr int MAX_TILE_UNITS = 4 * UW;

struct CoefP {
  const float* mc;
  long cbs, cks, ccs;
  const int* anchors;
  const float* scores;
  const int* member_slot;
  const int* counts;
  float* W;
  float* Ss;
  int K, top_k, Tmax;
  int first[MAX_FRAMES + 1];
};

// image n's candidates: slot k of its tile tl (tile t0 + tl of the table), its score as it is
struct TileCandidates {
  const CoefP& p;
  int t0, groups, width;
  __device__ int slot(int c) const { return p.member_slot[(long)t0 * p.K + c]; }
  __device__ float score(int c) const { return p.scores[(long)t0 * p.K + c]; }
  __device__ float coeff(int tl, int k, int ch) const {
    const long a = p.anchors[(long)(t0 + tl) * p.K + k];
    return p.mc[(long)(t0 + tl) * p.cbs + a * p.cks + ch * p.ccs];
  }
};

__global__ __launch_bounds__(VC_NT) void tile_coeff_kernel(const CoefP p) {
  const int n = blockIdx.y, t0 = p.first[n];
  vote_coeff_rows(TileCandidates{p, t0, p.first[n + 1] - t0, p.Tmax}, n, p.K, p.top_k, p.counts, p.W, p.Ss);
}

struct TileMaskP {
  const float* protos;
  const float* W;
  const int* counts;
  const float* boxes;
  const mtbt_tile* tiles;
  unsigned char* out;
  int n_frames, K, G, Tmax;   // K = top_k planes per image
  int first[MAX_FRAMES + 1];
  FrameD f[MAX_FRAMES];
};

template <bool CROP>
__global__ __launch_bounds__(256) void tile_mask_kernel(const TileMaskP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int s_list[MTBT_TILE_MAX_PER_IMAGE], s_nlist;
  const Lds s = lds_layout(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const TileCtx c = tile_context(p.f, p.n_frames, p.out, UW);   // a run of at most UW units per wave (the host's choice of the tile)
  const int n = c.n, G = p.G, cnt = max(min(p.counts[n], p.K), 0);
  const int t0 = p.first[n], T = min(p.first[n + 1] - t0, MTBT_TILE_MAX_PER_IMAGE);

  // the tiles whose window meets the frame tile, ascending
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

  int staged = -1;   // the tile whose patch is in LDS (workgroup-uniform), and that patch's place
  Patch pt = {0, 0, 1, 0, 16};
  for (int g0 = 0; g0 < cnt; g0 += 16) {
    const int nb = min(16, cnt - g0);
    float bv = 0.f;
    if (CROP && tid < 64) bv = g0 + (tid >> 2) < cnt ? p.boxes[((long)n * p.K + g0) * 4 + tid] : 0.f;   // merged boxes: in the frame already
    const bool ghit = group_hit<CROP>(c, s.boxs, bv, nb);
    float acc[UW][16];
#pragma unroll
    for (int j = 0; j < UW; ++j)
#pragma unroll
      for (int b = 0; b < 16; ++b) acc[j][b] = 0.f;
    if (ghit) {
      for (int li = 0; li < nlist; ++li) {
        const int tl = s_list[li];
        const mtbt_tile& d = p.tiles[t0 + tl];
        if (stage_vote_coef(s.coef, p.W, n, p.K, p.Tmax, tl, g0, cnt)) {
          // the part of the frame tile the window holds, and the prototype patch under it
          const int ix0 = max(c.X0, d.wx0), ix1 = min(c.Xl, d.wx1 - 1), iy0 = max(c.Y0, d.wy0), iy1 = min(c.Yl, d.wy1 - 1);
          const float step = d.step;
          const int pox = d.pox, poy = d.poy;
          if (staged != tl) {
            pt = patch_under(ix0, ix1, iy0, iy1, step, pox, poy, G, G);
            staged = pt.NPX <= NPX_CAP ? tl : -1;   // (always fits, by the host's choice of the frame tile; a patch that did not is never read)
            if (staged >= 0) stage_patch(s.patch, p.protos + (long)(t0 + tl) * G * G * NM, pt, [&](int y, int x) { return (long)y * G + x; });
            __syncthreads();
          }
          if (staged >= 0) {
            mfma_to_low(s, pt.NPXP);
            __syncthreads();
            // sampling at this tile's own tap positions; a lane outside the window taps the nearest pixel inside it and drops the value
#pragma unroll
            for (int j = 0; j < UW; ++j) {
              const int u = c.u0 + j, row = u >> c.wl, wd = u & (c.wt - 1);
              const int Y = c.Y0 + row, Xw = c.X0 + wd * 64, X = Xw + lane;
              if (j < c.un && wd < c.nwx && Y >= iy0 && Y <= iy1 && Xw <= ix1 && Xw + 63 >= ix0) {   // wave-uniform
                const bool inw = X >= ix0 && X <= ix1;
                const Taps t = taps_at(min(max(X, ix0), ix1), Y, step, pox, poy, G, G, pt);
#pragma unroll
                for (int b = 0; b < 16; ++b)
                  if (word_hit<CROP>(s.boxs, b, nb, Xw, Y, c.W0)) {
                    const float v = bilinear(s.low + b * LPITCH, t);
                    if (inw) acc[j][b] = acc[j][b] + v;
                  }
              }
            }
          }
        }
        __syncthreads();   // coef and low are rewritten for the next tile
      }
    }
    // one ballot per (unit, row): the ballot of the wave's unit j is kept by lane j
    unsigned long long word[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) word[b] = 0ull;
#pragma unroll
    for (int j = 0; j < UW; ++j) {
      const int u = c.u0 + j, wd = u & (c.wt - 1);
      const int X = c.X0 + wd * 64 + lane;
      if (j < c.un && wd < c.nwx) {
#pragma unroll
        for (int b = 0; b < 16; ++b) {
          bool in = X < c.W0;
          if (CROP) in = in && box_holds_x(s.boxs + b * 4, (float)X);
          const unsigned long long mk = __ballot(in && acc[j][b] > 0.f);
          if (lane == j) word[b] = mk;
        }
      }
    }
    store_words(c, word, g0, nb);
    __syncthreads();   // boxs is rewritten by the next group
  }
  zero_tail(c, cnt, p.K);
}

}  // namespace

extern "C" int mtbt_sizeof_tile_args(int which) {
  switch (which) {
    case 0: return (int)sizeof(mtbt_tile);
    case 1: return (int)sizeof(mtbt_tile_merge_args);
    case 2: return (int)sizeof(mtbt_tile_mask_args);
    default: return -1;
  }
}

extern "C" int mtbt_vote_tile_masks(const mtbt_tile_mask_args* a, const mtbt_frame* frames, int n_frames, void* stream) {
  if (!a || !frames || !a->out || !a->member_slot || !a->counts || !a->W || !a->Ss) return MTBT_EINVAL;
  if (!a->protos || !a->mc || !a->anchors || !a->scores || !a->tiles || !a->tiles_dev || !a->first) return MTBT_EINVAL;
  if (!frame_args_ok(n_frames, a->N, a->nm, a->top_k, a->hp, a->wp, a->out_bytes)) return MTBT_EINVAL;
  if (a->K < 1 || a->reserved != 0 || a->hp != a->wp || a->Tmax < 1 || a->Tmax > MTBT_TILE_MAX_PER_IMAGE) return MTBT_EINVAL;
  if (a->crop && !a->boxes) return MTBT_EINVAL;
  int Tbig = 0;
  if (int rc = tile_check::check_table(a->tiles, a->first, a->N, a->n_tiles, a->K, a->Tmax, false, frames, Tbig)) return rc;
  TileMaskP p;
  long blocks = 0;
  if (int rc = frame_layout(frames, n_frames, a->top_k, a->hp, a->wp, false, a->out_bytes, a->tiles, a->first, MAX_TILE_UNITS, 4, p.f, blocks))
    return rc;
  if (!aligned16(a->protos) || !aligned16(a->out)) return MTBT_EALIGN;
  CoefP c;
  c.mc = a->mc; c.cbs = a->mc_batch_stride; c.cks = a->mc_k_stride; c.ccs = a->mc_c_stride;
  c.anchors = a->anchors; c.scores = a->scores; c.member_slot = a->member_slot; c.counts = a->counts; c.W = a->W; c.Ss = a->Ss;
  c.K = a->K; c.top_k = a->top_k; c.Tmax = a->Tmax;
  for (int n = 0; n <= MAX_FRAMES; ++n) c.first[n] = p.first[n] = a->first[n < n_frames ? n : n_frames];
  p.protos = a->protos; p.W = a->W; p.counts = a->counts; p.boxes = a->boxes; p.tiles = a->tiles_dev; p.out = a->out;
  p.n_frames = n_frames; p.K = a->top_k; p.G = a->hp; p.Tmax = a->Tmax;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tile_coeff_kernel, dim3((a->top_k + VC_ROWS - 1) / VC_ROWS, a->N), dim3(VC_NT), 0, s, c);
  MTBT_LAUNCH_CHECK();
  return launch_mask_kernel(a->crop ? tile_mask_kernel<true> : tile_mask_kernel<false>, blocks, p, s);
}
