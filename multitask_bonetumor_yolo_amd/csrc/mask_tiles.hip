// Instance masks of merged rows of sliced inference, voted across the tiles of their members straight into the bit-packed frame planes
// (mtbt_vote_tile_masks; the definition is in include/mtbt_hip.h, tests/slice_reference.py restates it).
//
//   W[n,r,tl,:] = (sum over row r's members in tile tl of s_c * coeff_c[:]) / Ss[n,r]     -- tile_coeff_kernel: small, serial sums in the
//                                                                                           stated order, bit-exact
//   low_t       = W[n,r,tl,:] . P_t                                                        -- tile_mask_kernel: fp32 MFMA per (row group, tile)
//   v(Y,X)      = sum over the tiles whose window holds (X, Y), ascending, of bilinear(low_t) at the tile's own tap position
//   bit         = v > 0 (&& inside the merged box when cropping)                           -- packed as mask_frame.hip packs
//
// tile_mask_kernel keeps mask_frame.hip's frame tile (words x rows), LDS layout, MFMA phase, ballot and 8-byte stores.  Unlike
// mask_vote.hip the sources sample at DIFFERENT positions, so the sum over tiles happens after the tap, in registers: a wave carries at
// most UW (unit, 16 rows) accumulator sets, i.e. the frame tile is at most 4 UW units, picked on the host so that the prototype patch of
// every tile under (frame tile x that tile's window) fits the patch buffer.  Per (row group, tile): the tiles whose window misses the frame
// tile are never looked at (a list built once per workgroup), a pair whose 16 x 32 coefficients are all zero -- no member of the 16 rows
// in that tile -- is skipped, and the patch in LDS is kept while the next pair needs the same tile.
#include "common.h"
#include "frame_tile.h"
#include "tile_check.h"

// No FMA contraction in this file (built with -ffp-contract=off, see build.py), as in mask_frame.hip and mask_vote.hip.

namespace {

using namespace frame_tile;

constexpr int VC_NT = 256;     // tile_coeff_kernel: thread = (tile of a pass of 8, channel)
constexpr int VC_ROWS = 8;     // merged rows per workgroup
constexpr int UW = 4;          // (row, word) units per wave: UW x 16 accumulators per lane
constexpr int MAX_TILE_UNITS = 4 * UW;

// frame_tap with the tile's prototype offset: the tap of frame pixel d in a tile whose grid starts `po` prototype pixels into the pass
__host__ __device__ __forceinline__ void tile_tap(int d, float step, int po, int size, int& i0, int& i1, float& l) {
  float s = ((float)d + 0.5f) * step - 0.5f - (float)po;
  s = s > 0.f ? s : 0.f;
  const int i = (int)s;
  i0 = i < size - 1 ? i : size - 1;
  i1 = i0 + 1 < size - 1 ? i0 + 1 : size - 1;
  float w = s - (float)i0;
  w = w > 0.f ? w : 0.f;
  l = w < 1.f ? w : 1.f;
}

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

// One workgroup per (VC_ROWS merged rows, image).  The membership and scores of the image's tiles are staged in LDS once; per row, wave 0
// adds the members' scores in candidate order, then thread (tile, ch) adds s_c * coeff_c[ch] over that tile's members in slot order and
// divides once (vote_coeff_kernel of mask_vote.hip with tiles for sources).
__global__ __launch_bounds__(VC_NT) void tile_coeff_kernel(const CoefP p) {
  __shared__ int s_slot[MTBT_FUSE_MAX_CANDIDATES];
  __shared__ float s_s[MTBT_FUSE_MAX_CANDIDATES];
  __shared__ float s_ss;
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int K = p.K, top_k = p.top_k, Tmax = p.Tmax;
  const int t0 = p.first[n], T = p.first[n + 1] - t0, C = T * K;
  const int cnt = max(min(p.counts[n], top_k), 0);
  for (int c = tid; c < C; c += VC_NT) {
    const int slot = p.member_slot[(long)t0 * K + c];
    s_slot[c] = slot;
    s_s[c] = slot >= 0 ? p.scores[(long)t0 * K + c] : 0.f;
  }
  __syncthreads();
  const int ch = tid & 31;
  for (int r = blockIdx.x * VC_ROWS; r < min((int)(blockIdx.x + 1) * VC_ROWS, top_k); ++r) {
    const bool live = r < cnt;
    if (tid < 64) {
      float ss = 0.f;
      if (live)
        for (int c0 = 0; c0 < C; c0 += 64) {
          unsigned long long mem = __ballot(c0 + lane < C && s_slot[min(c0 + lane, C - 1)] == r);
          while (mem) {   // wave-uniform: every lane adds the same members in ascending c
            const int j = __ffsll((long long)mem) - 1;
            mem &= mem - 1;
            ss = __fadd_rn(ss, s_s[c0 + j]);
          }
        }
      if (tid == 0) { s_ss = ss; p.Ss[(long)n * top_k + r] = ss; }
    }
    __syncthreads();
    for (int tl = tid >> 5; tl < Tmax; tl += VC_NT / 32) {
      float acc = 0.f;
      bool any = false;
      if (live && tl < T)
        for (int k = 0; k < K; ++k)
          if (s_slot[tl * K + k] == r) {
            const long a = p.anchors[(long)(t0 + tl) * K + k];
            const float co = p.mc[(long)(t0 + tl) * p.cbs + a * p.cks + ch * p.ccs];
            acc = __fadd_rn(acc, __fmul_rn(s_s[tl * K + k], co));
            any = true;
          }
      p.W[(((long)n * top_k + r) * Tmax + tl) * NM + ch] = any ? __fdiv_rn(acc, s_ss) : 0.f;
    }
    __syncthreads();   // s_ss is rewritten for the next row
  }
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
  float* patch = reinterpret_cast<float*>(smem);       // [NPX_CAP][PPITCH]
  float* coef = patch + NPX_CAP * PPITCH;              // [16][PPITCH]
  float* low = coef + 16 * PPITCH;                     // [16][LPITCH]
  float* boxs = low + 16 * LPITCH;                     // [16][4] merged boxes of the group
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  int n = 0;
  for (int i = 1; i < p.n_frames; ++i)
    if ((int)blockIdx.x >= p.f[i].blk0) n = i;
  const FrameD& f = p.f[n];
  const int H0 = f.H0, W0 = f.W0, wl = f.wl, wt = 1 << wl, G = p.G, Tmax = p.Tmax;
  const int t = (int)blockIdx.x - f.blk0;
  const int ty = t / f.tiles_x, tx = t - ty * f.tiles_x;
  const int X0 = tx * 64 * wt, Y0 = ty * f.th;
  const int Xl = min(X0 + 64 * wt, W0) - 1, Yl = min(Y0 + f.th, H0) - 1;   // last pixel of the frame tile
  const int words_x = f.pitch >> 3;
  const int nwx = min(wt, words_x - tx * wt), nrows = Yl - Y0 + 1;
  const int cnt = max(min(p.counts[n], p.K), 0);
  const int t0 = p.first[n], T = min(p.first[n + 1] - t0, MTBT_TILE_MAX_PER_IMAGE);

  // the tiles whose window meets the frame tile, ascending
  if (tid == 0) {
    int m = 0;
    for (int tl = 0; tl < T; ++tl) {
      const mtbt_tile& d = p.tiles[t0 + tl];
      if (d.wx0 <= Xl && X0 < d.wx1 && d.wy0 <= Yl && Y0 < d.wy1) s_list[m++] = tl;
    }
    s_nlist = m;
  }
  __syncthreads();
  const int nlist = s_nlist;

  // units of this wave: u = row * wt + word, a run of upw <= UW consecutive ones (the host's choice of the tile); lane j stores unit u0 + j
  const int U = nrows << wl, upw = min((U + 3) >> 2, UW), u0 = wave * upw;
  const int un = max(min(upw, U - u0), 0);
  const int my_u = u0 + lane, my_row = my_u >> wl, my_word = my_u & (wt - 1);
  const bool my_store = lane < un && my_word < nwx;
  unsigned char* my_out = p.out + f.offset + (long)(Y0 + my_row) * f.pitch + (long)(tx * wt + my_word) * 8;
  const long plane = (long)H0 * f.pitch;

  int staged = -1;   // the tile whose patch is in LDS (workgroup-uniform), and that patch's place
  int pxa = 0, pya = 0, PW = 1, NPXP = 16;
  for (int g0 = 0; g0 < cnt; g0 += 16) {
    const int nb = min(16, cnt - g0);
    if (CROP) {
      if (tid < 64) boxs[tid] = g0 + (tid >> 2) < cnt ? p.boxes[((long)n * p.K + g0) * 4 + tid] : 0.f;
      __syncthreads();
    }
    bool ghit = true;   // workgroup-uniform: does any box of the group touch the frame tile
    if (CROP) {
      ghit = false;
      for (int b = 0; b < nb; ++b) {
        const float x1 = boxs[b * 4], y1 = boxs[b * 4 + 1], x2 = boxs[b * 4 + 2], y2 = boxs[b * 4 + 3];
        ghit = ghit || (x1 <= (float)Xl && (float)X0 < x2 && y1 <= (float)Yl && (float)Y0 < y2);
      }
    }
    float acc[UW][16];
#pragma unroll
    for (int j = 0; j < UW; ++j)
#pragma unroll
      for (int b = 0; b < 16; ++b) acc[j][b] = 0.f;
    if (ghit) {
      for (int li = 0; li < nlist; ++li) {
        const int tl = s_list[li];
        const mtbt_tile& d = p.tiles[t0 + tl];
        bool nz = false;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int i = tid + u * 256, b = i >> 5, c = i & 31;
          const float v = g0 + b < cnt ? p.W[(((long)n * p.K + g0 + b) * Tmax + tl) * NM + c] : 0.f;
          coef[b * PPITCH + c] = v;
          nz = nz || v != 0.f;
        }
        if (__syncthreads_or(nz)) {   // (the barrier also publishes coef)
          // the part of the frame tile the window holds, and the prototype patch under it
          const int ix0 = max(X0, d.wx0), ix1 = min(Xl, d.wx1 - 1), iy0 = max(Y0, d.wy0), iy1 = min(Yl, d.wy1 - 1);
          const float step = d.step;
          const int pox = d.pox, poy = d.poy;
          if (staged != tl) {
            int pxb, pyb, tmp;
            float ftmp;
            tile_tap(ix0, step, pox, G, pxa, tmp, ftmp);
            tile_tap(ix1, step, pox, G, tmp, pxb, ftmp);
            tile_tap(iy0, step, poy, G, pya, tmp, ftmp);
            tile_tap(iy1, step, poy, G, tmp, pyb, ftmp);
            PW = pxb - pxa + 1;
            const int NPX = PW * (pyb - pya + 1);
            NPXP = (NPX + 15) & ~15;
            staged = NPXP <= NPX_CAP ? tl : -1;   // (always fits, by the host's choice of the frame tile; a patch that did not is never read)
            if (staged >= 0) {
              const float* pr = p.protos + (long)(t0 + tl) * G * G * NM;
              for (int i = tid; i < NPXP * (NM / 4); i += 256) {
                const int px = i >> 3, c4 = i & 7;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (px < NPX) {
                  const int py = px / PW, pxx = px - py * PW;
                  v = *reinterpret_cast<const float4*>(pr + ((long)(pya + py) * G + (pxa + pxx)) * NM + c4 * 4);
                }
                float* dd = patch + px * PPITCH + c4 * 4;
                dd[0] = v.x; dd[1] = v.y; dd[2] = v.z; dd[3] = v.w;
              }
            }
            __syncthreads();
          }
          if (staged >= 0) {
            // low[16][NPXP] = coef[16][32] x patch^T on the fp32 MFMA; wave w takes column groups w, w+4, ...
            float a[8];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) a[ks] = coef[(lane & 15) * PPITCH + ks * 4 + (lane >> 4)];
            for (int pg = wave; pg < NPXP / 16; pg += 4) {
              f32x4 c4 = f32x4{0.f, 0.f, 0.f, 0.f};
              const float* bp = patch + (pg * 16 + (lane & 15)) * PPITCH + (lane >> 4);
#pragma unroll
              for (int ks = 0; ks < 8; ++ks) c4 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks], bp[ks * 4], c4, 0, 0, 0);
#pragma unroll
              for (int r = 0; r < 4; ++r) low[(4 * (lane >> 4) + r) * LPITCH + pg * 16 + (lane & 15)] = c4[r];
            }
            __syncthreads();
            // sampling at this tile's own tap positions; a lane outside the window taps the nearest pixel inside it and drops the value
#pragma unroll
            for (int j = 0; j < UW; ++j) {
              const int u = u0 + j, row = u >> wl, wd = u & (wt - 1);
              const int Y = Y0 + row, Xw = X0 + wd * 64, X = Xw + lane;
              if (j < un && wd < nwx && Y >= iy0 && Y <= iy1 && Xw <= ix1 && Xw + 63 >= ix0) {   // wave-uniform
                const bool inw = X >= ix0 && X <= ix1;
                int x0, x1, y0, y1;
                float lx, ly;
                tile_tap(min(max(X, ix0), ix1), step, pox, G, x0, x1, lx);
                tile_tap(Y, step, poy, G, y0, y1, ly);
                const float wx0 = 1.f - lx, wy0 = 1.f - ly;
                const int i00 = (y0 - pya) * PW + (x0 - pxa), i01 = (y0 - pya) * PW + (x1 - pxa);
                const int i10 = (y1 - pya) * PW + (x0 - pxa), i11 = (y1 - pya) * PW + (x1 - pxa);
                const float fY = (float)Y, fXw = (float)Xw, fXe = (float)min(Xw + 63, W0 - 1);
#pragma unroll
                for (int b = 0; b < 16; ++b) {
                  bool hit = !CROP || b < nb;   // wave-uniform.  Without cropping a row past nb has zero coefficients: v = 0
                  if (CROP) {
                    const float bx1 = boxs[b * 4], by1 = boxs[b * 4 + 1], bx2 = boxs[b * 4 + 2], by2 = boxs[b * 4 + 3];
                    hit = hit && bx1 <= fXe && fXw < bx2 && by1 <= fY && fY < by2;   // else the word is wholly outside the box: it stays zero
                  }
                  if (hit) {
                    const float* l = low + b * LPITCH;
                    const float v = wy0 * (wx0 * l[i00] + lx * l[i01]) + ly * (wx0 * l[i10] + lx * l[i11]);
                    if (inw) acc[j][b] = acc[j][b] + v;
                  }
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
      const int u = u0 + j, wd = u & (wt - 1);
      const int X = X0 + wd * 64 + lane;
      if (j < un && wd < nwx) {
        const float fX = (float)X;
#pragma unroll
        for (int b = 0; b < 16; ++b) {
          bool in = X < W0;
          if (CROP) in = in && boxs[b * 4] <= fX && fX < boxs[b * 4 + 2];
          const unsigned long long mk = __ballot(in && acc[j][b] > 0.f);
          if (lane == j) word[b] = mk;
        }
      }
    }
    if (my_store) {
#pragma unroll
      for (int b = 0; b < 16; ++b)
        if (b < nb) *reinterpret_cast<unsigned long long*>(my_out + (long)(g0 + b) * plane) = word[b];
    }
    __syncthreads();   // boxs is rewritten by the next group
  }
  // planes r >= cnt: zeros
  if (my_store)
    for (int k = cnt; k < p.K; ++k) *reinterpret_cast<unsigned long long*>(my_out + (long)k * plane) = 0ull;
}

// prototype pixels of tile `d` spanned along one axis by any run of `len` frame pixels that starts at a multiple of `len`, cut to the window
inline int tile_span(int len, int w0, int w1, float step, int po, int size) {
  int best = 0;
  for (int a = (w0 / len) * len; a < w1; a += len) {
    const int lo = a > w0 ? a : w0, hi = (a + len < w1 ? a + len : w1) - 1;
    int i0, i1, t0, t1;
    float l;
    tile_tap(lo, step, po, size, i0, t0, l);
    tile_tap(hi, step, po, size, t1, i1, l);
    if (i1 - i0 + 1 > best) best = i1 - i0 + 1;
  }
  return best;
}

// the largest frame tile (2^wl words x th rows, at most MAX_TILE_UNITS units) under which every tile's patch fits NPX_CAP; wider wins a tie
inline void tile_pick(const mtbt_frame& fr, const mtbt_tile* tiles, int T, int G, int& wl, int& th) {
  const int words_x = fr.pitch >> 3;
  wl = 0; th = 1;   // a 64 x 1 run at step <= 1: at most 66 x 2 prototype pixels
  long best = 0;
  for (int l = 3; l >= 0; --l)
    for (int h = 4; h >= 0; --h) {
      if (((1 << l) << h) > MAX_TILE_UNITS || (l > 0 && (1 << (l - 1)) >= words_x) || (h > 0 && (1 << (h - 1)) >= fr.height)) continue;
      const long area = 1L << (l + h);
      if (area <= best) continue;
      bool fits = true;
      for (int t = 0; t < T && fits; ++t) {
        const mtbt_tile& d = tiles[t];
        const int n = tile_span(64 << l, d.wx0, d.wx1, d.step, d.pox, G) * tile_span(1 << h, d.wy0, d.wy1, d.step, d.poy, G);
        fits = ((n + 15) & ~15) <= NPX_CAP;
      }
      if (fits) { best = area; wl = l; th = 1 << h; }
    }
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
  if (n_frames < 1 || n_frames > MAX_FRAMES || n_frames != a->N) return MTBT_EINVAL;
  if (a->nm != NM || a->K < 1 || a->top_k < 1 || a->top_k > 65535 || a->reserved != 0) return MTBT_EINVAL;
  if (a->hp < 1 || a->hp != a->wp || a->Tmax < 1 || a->Tmax > MTBT_TILE_MAX_PER_IMAGE || a->out_bytes < 0) return MTBT_EINVAL;
  if (a->crop && !a->boxes) return MTBT_EINVAL;
  int Tbig = 0;
  if (int rc = tile_check::check_table(a->tiles, a->first, a->N, a->n_tiles, a->K, a->Tmax, false, frames, Tbig)) return rc;
  TileMaskP p;
  long blocks = 0;
  mtbt_frame fr[MAX_FRAMES];
  for (int n = 0; n < n_frames; ++n) {
    fr[n] = frames[n];
    fr[n].step = 1.f;    // the frame's own step and scale are not used: every tile carries its own
    fr[n].scale = 1.f;
  }
  if (int rc = frame_layout(fr, n_frames, a->top_k, a->hp, a->wp, false, a->out_bytes, p.f, blocks)) return rc;
  if (!aligned16(a->protos) || !aligned16(a->out)) return MTBT_EALIGN;

  blocks = 0;
  for (int n = 0; n < n_frames; ++n) {
    FrameD& d = p.f[n];
    tile_pick(fr[n], a->tiles + a->first[n], a->first[n + 1] - a->first[n], a->hp, d.wl, d.th);
    const int words_x = d.pitch >> 3;
    d.tiles_x = (words_x + (1 << d.wl) - 1) >> d.wl;
    d.blk0 = (int)blocks;
    blocks += (long)d.tiles_x * ((d.H0 + d.th - 1) / d.th);
    if (blocks > 0x7fffffffL) return MTBT_EINVAL;
  }
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
  if (a->crop) {
    if (int rc = mtbt_allow_lds(tile_mask_kernel<true>, (int)FRAME_LDS)) return rc;
    hipLaunchKernelGGL(tile_mask_kernel<true>, dim3((unsigned)blocks), dim3(256), FRAME_LDS, s, p);
  } else {
    if (int rc = mtbt_allow_lds(tile_mask_kernel<false>, (int)FRAME_LDS)) return rc;
    hipLaunchKernelGGL(tile_mask_kernel<false>, dim3((unsigned)blocks), dim3(256), FRAME_LDS, s, p);
  }
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}
