// Instance masks of fused detections voted over the members of their clusters (mtbt_vote_masks; the definition is in include/mtbt_hip.h,
// tests/vote_reference.py restates it).
//
//   W[n,r,m,:]   = (sum over the members c of source m of s_c * coeff_c[:]) / Ss[n,r]        -- vote_coeff_kernel: small, serial sums in the
//                                                                                              stated order, bit-exact
//   low[n,r,y,x] = sum_m sum_c W[n,r,m,c] * U_m[n,y,x,c]                                     -- vote_mask_kernel: fp32 MFMA over M sources
//   bit          = bilinear(low)(X, Y) > 0 (&& inside the fused frame box when cropping)     -- as mask_frame.hip
//
// vote_mask_kernel is frame_mask_kernel (mask_frame.hip: tile of words x rows, prototype patch in LDS, 16 rows per group on
// v_mfma_f32_16x16x4_f32, ballot, one 8-byte store per row word) with a loop over the sources inside each group: source m's patch is staged
// through the index map of orient[m] (the upright rectangle under the tile is a rectangle of the view, possibly transposed and mirrored),
// and the MFMA accumulators stay in registers from one source to the next.  One patch buffer: the LDS footprint, and with it two
// workgroups per CU, is mask_frame.hip's.  A (group, source) pair whose 16 x 32 coefficients are all zero -- the source has no member in
// any of the 16 clusters -- is skipped, and the patch in LDS is kept when the next pair needs the same source (always, with one source).
#include "common.h"
#include "frame_tile.h"

// No FMA contraction in this file (built with -ffp-contract=off, see build.py), as in mask_frame.hip and box_fuse.hip.

namespace {

using namespace frame_tile;

constexpr int VC_NT = 256;     // vote_coeff_kernel: thread = (source, channel)
constexpr int VC_ROWS = 8;     // fused rows per workgroup
static_assert(MTBT_FUSE_MAX_SOURCES * NM == VC_NT, "one thread per (source, channel)");
static_assert(NPX_CAP / 16 == 24, "a wave carries at most 6 column groups of 16 prototype pixels");

struct CoefP {
  const float* mc[MTBT_FUSE_MAX_SOURCES];
  long cbs[MTBT_FUSE_MAX_SOURCES], cks[MTBT_FUSE_MAX_SOURCES], ccs[MTBT_FUSE_MAX_SOURCES];
  const int* anchors[MTBT_FUSE_MAX_SOURCES];
  const float* scores[MTBT_FUSE_MAX_SOURCES];
  float weight[MTBT_FUSE_MAX_SOURCES];
  const int* member_slot;
  const int* counts;
  float* W;
  float* Ss;
  int M, K, top_k;
};

// One workgroup per (VC_ROWS fused rows, image).  The image's membership and candidate scores are staged in LDS once; per row, wave 0 adds
// the members' scores in candidate order (a ballot finds them, the additions are serial), then thread (m, ch) adds s_c * coeff_c[ch] over
// source m's members in slot order and divides once.
__global__ __launch_bounds__(VC_NT) void vote_coeff_kernel(const CoefP p) {
  __shared__ int s_slot[MTBT_FUSE_MAX_CANDIDATES];
  __shared__ float s_s[MTBT_FUSE_MAX_CANDIDATES];
  __shared__ float s_ss;
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int M = p.M, K = p.K, C = M * K, top_k = p.top_k;
  const int cnt = max(min(p.counts[n], top_k), 0);
  for (int c = tid; c < C; c += VC_NT) {
    const int m = c / K, k = c - m * K;
    const int slot = p.member_slot[(long)n * C + c];
    s_slot[c] = slot;
    s_s[c] = slot >= 0 ? __fmul_rn(p.scores[m][(long)n * K + k], p.weight[m]) : 0.f;
  }
  __syncthreads();
  const int m = tid >> 5, ch = tid & 31;
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
    if (m < M) {
      float acc = 0.f;
      bool any = false;
      if (live)
        for (int k = 0; k < K; ++k)
          if (s_slot[m * K + k] == r) {
            const long a = p.anchors[m][(long)n * K + k];
            const float co = p.mc[m][(long)n * p.cbs[m] + a * p.cks[m] + ch * p.ccs[m]];
            acc = __fadd_rn(acc, __fmul_rn(s_s[m * K + k], co));
            any = true;
          }
      p.W[(((long)n * top_k + r) * M + m) * NM + ch] = any ? __fdiv_rn(acc, s_ss) : 0.f;
    }
    __syncthreads();   // s_ss is rewritten for the next row
  }
}

struct VoteP {
  const float* protos[MTBT_FUSE_MAX_SOURCES];
  int orient[MTBT_FUSE_MAX_SOURCES];
  const float* W;
  const int* counts;
  const float* boxes;
  float* boxes_frame;
  unsigned char* out;
  int n_frames, K, G, M;   // K = top_k planes per image; G = hp = wp
  FrameD f[MAX_FRAMES];
};

template <bool CROP>
__global__ __launch_bounds__(256) void vote_mask_kernel(const VoteP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* patch = reinterpret_cast<float*>(smem);       // [NPX_CAP][PPITCH]
  float* coef = patch + NPX_CAP * PPITCH;              // [16][PPITCH]
  float* low = coef + 16 * PPITCH;                     // [16][LPITCH]
  float* boxs = low + 16 * LPITCH;                     // [16][4] frame boxes of the group
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  int n = 0;
  for (int i = 1; i < p.n_frames; ++i)
    if ((int)blockIdx.x >= p.f[i].blk0) n = i;
  const FrameD& f = p.f[n];
  const int H0 = f.H0, W0 = f.W0, wl = f.wl, wt = 1 << wl, G = p.G, M = p.M;
  const float step = f.step;
  const int t = (int)blockIdx.x - f.blk0;
  const int ty = t / f.tiles_x, tx = t - ty * f.tiles_x;
  const int X0 = tx * 64 * wt, Y0 = ty * f.th;
  const int Xl = min(X0 + 64 * wt, W0) - 1, Yl = min(Y0 + f.th, H0) - 1;   // last pixel of the tile
  const int words_x = f.pitch >> 3;
  const int nwx = min(wt, words_x - tx * wt), nrows = Yl - Y0 + 1;
  const int cnt = max(min(p.counts[n], p.K), 0);

  // fused boxes in the frame: written once per image, by its first tile
  if (t == 0 && p.boxes_frame) {
    for (int i = tid; i < p.K * 4; i += 256) {
      const long at = (long)n * p.K * 4 + i;
      p.boxes_frame[at] = (i >> 2) < cnt ? frame_box(p.boxes[at], f.scale, i & 3, H0, W0) : 0.f;
    }
  }

  // upright prototype patch under the tile
  int pxa, pxb, pya, pyb, tmp;
  float ftmp;
  frame_tap(X0, step, G, pxa, tmp, ftmp);
  frame_tap(Xl, step, G, tmp, pxb, ftmp);
  frame_tap(Y0, step, G, pya, tmp, ftmp);
  frame_tap(Yl, step, G, tmp, pyb, ftmp);
  const int PW = pxb - pxa + 1, PH = pyb - pya + 1;
  const int NPX = PW * PH, NPXP = min((NPX + 15) & ~15, NPX_CAP);   // <= NPX_CAP by the host's choice of the tile
  const int npg = NPXP / 16;

  // units of this wave: u = row * wt + word, a run of upw consecutive ones; lane j keeps (and stores) unit u0 + j
  const int U = nrows << wl, upw = (U + 3) >> 2, u0 = wave * upw;
  const int un = max(min(upw, U - u0), 0);
  const int my_u = u0 + lane, my_row = my_u >> wl, my_word = my_u & (wt - 1);
  const bool my_store = lane < un && my_word < nwx;
  unsigned char* my_out = p.out + f.offset + (long)(Y0 + my_row) * f.pitch + (long)(tx * wt + my_word) * 8;
  const long plane = (long)H0 * f.pitch;

  int staged = -1;   // the source whose patch is in LDS (workgroup-uniform)
  for (int g0 = 0; g0 < cnt; g0 += 16) {
    const int nb = min(16, cnt - g0);
    if (CROP) {
      if (tid < 64) {
        const int b = tid >> 2;
        boxs[tid] = g0 + b < cnt ? frame_box(p.boxes[((long)n * p.K + g0 + b) * 4 + (tid & 3)], f.scale, tid & 3, H0, W0) : 0.f;
      }
      __syncthreads();
    }
    bool ghit = true;   // workgroup-uniform: does any box of the group touch the tile
    if (CROP) {
      ghit = false;
      for (int b = 0; b < nb; ++b) {
        const float x1 = boxs[b * 4], y1 = boxs[b * 4 + 1], x2 = boxs[b * 4 + 2], y2 = boxs[b * 4 + 3];
        ghit = ghit || (x1 <= (float)Xl && (float)X0 < x2 && y1 <= (float)Yl && (float)Y0 < y2);
      }
    }
    if (ghit) {
      // low[16][NPXP] = sum_m coef_m[16][32] x patch_m^T on the fp32 MFMA; wave w carries column groups w, w+4, ... over the sources
      f32x4 acc[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int m = 0; m < M; ++m) {
        bool nz = false;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int i = tid + u * 256, b = i >> 5, c = i & 31;
          const float v = g0 + b < cnt ? p.W[(((long)n * p.K + g0 + b) * M + m) * NM + c] : 0.f;
          coef[b * PPITCH + c] = v;
          nz = nz || v != 0.f;
        }
        if (__syncthreads_or(nz)) {   // (the barrier also publishes coef)
          if (staged != m) {
            const float* pr = p.protos[m] + (long)n * G * G * NM;
            const int o = p.orient[m];
            for (int i = tid; i < NPXP * (NM / 4); i += 256) {
              const int px = i >> 3, c4 = i & 7;
              float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
              if (px < NPX) {
                const int py = px / PW, pxx = px - py * PW;
                const int y = pya + py, x = pxa + pxx;                         // upright prototype pixel
                const int a = (o & 4) ? x : y, b = (o & 4) ? y : x;            // ... in the view: row a, column b, then the flips
                const int sy = (o & 2) ? G - 1 - a : a, sx = (o & 1) ? G - 1 - b : b;
                v = *reinterpret_cast<const float4*>(pr + ((long)sy * G + sx) * NM + c4 * 4);
              }
              float* d = patch + px * PPITCH + c4 * 4;
              d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
            staged = m;
            __syncthreads();
          }
          float a[8];
#pragma unroll
          for (int ks = 0; ks < 8; ++ks) a[ks] = coef[(lane & 15) * PPITCH + ks * 4 + (lane >> 4)];
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            const int pg = wave + 4 * i;
            if (pg < npg) {
              const float* bp = patch + (pg * 16 + (lane & 15)) * PPITCH + (lane >> 4);
#pragma unroll
              for (int ks = 0; ks < 8; ++ks) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks], bp[ks * 4], acc[i], 0, 0, 0);
            }
          }
        }
        __syncthreads();   // coef (and the patch) are rewritten for the next source
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const int pg = wave + 4 * i;
        if (pg < npg) {
#pragma unroll
          for (int r = 0; r < 4; ++r) low[(4 * (lane >> 4) + r) * LPITCH + pg * 16 + (lane & 15)] = acc[i][r];
        }
      }
      __syncthreads();
    }
    // sampling: one ballot per (unit, box)
    unsigned long long word[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) word[b] = 0ull;
    if (ghit) {
      for (int j = 0; j < un; ++j) {
        const int u = u0 + j, row = u >> wl, wd = u & (wt - 1);
        if (wd >= nwx) continue;
        const int Y = Y0 + row, Xw = X0 + wd * 64, X = Xw + lane;
        const bool valid = X < W0;
        int x0, x1, y0, y1;
        float lx, ly;
        frame_tap(min(X, W0 - 1), step, G, x0, x1, lx);
        frame_tap(Y, step, G, y0, y1, ly);
        const float wx0 = 1.f - lx, wy0 = 1.f - ly;
        const int i00 = (y0 - pya) * PW + (x0 - pxa), i01 = (y0 - pya) * PW + (x1 - pxa);
        const int i10 = (y1 - pya) * PW + (x0 - pxa), i11 = (y1 - pya) * PW + (x1 - pxa);
        const float fX = (float)X, fY = (float)Y, fXw = (float)Xw, fXe = (float)min(Xw + 63, W0 - 1);
#pragma unroll
        for (int b = 0; b < 16; ++b) {
          // hit is wave-uniform.  Without cropping all 16 rows are sampled (a row past nb has zero coefficients: v = 0, no bit)
          bool in = valid, hit = !CROP || b < nb;
          if (CROP) {
            const float bx1 = boxs[b * 4], by1 = boxs[b * 4 + 1], bx2 = boxs[b * 4 + 2], by2 = boxs[b * 4 + 3];
            hit = hit && bx1 <= fXe && fXw < bx2 && by1 <= fY && fY < by2;   // else the word is wholly outside the box: it stays zero
            in = in && bx1 <= fX && fX < bx2;
          }
          if (hit) {
            const float* l = low + b * LPITCH;
            const float v = wy0 * (wx0 * l[i00] + lx * l[i01]) + ly * (wx0 * l[i10] + lx * l[i11]);
            const unsigned long long mk = __ballot(in && v > 0.f);
            if (lane == j) word[b] = mk;
          }
        }
      }
    }
    if (my_store) {
#pragma unroll
      for (int b = 0; b < 16; ++b)
        if (b < nb) *reinterpret_cast<unsigned long long*>(my_out + (long)(g0 + b) * plane) = word[b];
    }
    __syncthreads();   // low / boxs are rewritten by the next group
  }
  // planes r >= cnt: zeros
  if (my_store)
    for (int k = cnt; k < p.K; ++k) *reinterpret_cast<unsigned long long*>(my_out + (long)k * plane) = 0ull;
}

}  // namespace

extern "C" int mtbt_sizeof_vote_mask_args(void) { return (int)sizeof(mtbt_vote_mask_args); }

extern "C" int mtbt_vote_masks(const mtbt_vote_mask_args* a, const mtbt_frame* frames, int n_frames, void* stream) {
  if (!a || !frames || !a->out || !a->member_slot || !a->counts || !a->W || !a->Ss) return MTBT_EINVAL;
  const int M = a->n_sources;
  if (M < 1 || M > MTBT_FUSE_MAX_SOURCES) return MTBT_EINVAL;
  if (n_frames < 1 || n_frames > MAX_FRAMES || n_frames != a->N) return MTBT_EINVAL;
  if (a->nm != NM || a->K < 1 || (long)M * a->K > MTBT_FUSE_MAX_CANDIDATES || a->top_k < 1 || a->top_k > 65535) return MTBT_EINVAL;
  if (a->hp < 1 || a->hp != a->wp || a->out_bytes < 0) return MTBT_EINVAL;
  for (int m = 0; m < M; ++m) {
    if (a->orient[m] < 0 || a->orient[m] > 7) return MTBT_EINVAL;
    if (!a->protos[m] || !a->mc[m] || !a->anchors[m] || !a->scores[m]) return MTBT_EINVAL;
  }
  if ((a->crop || a->boxes_frame) && !a->boxes) return MTBT_EINVAL;
  VoteP p;
  long blocks = 0;
  if (int rc = frame_layout(frames, n_frames, a->top_k, a->hp, a->wp, a->boxes != nullptr, a->out_bytes, p.f, blocks)) return rc;
  for (int m = 0; m < M; ++m)
    if (!aligned16(a->protos[m])) return MTBT_EALIGN;
  if (!aligned16(a->out)) return MTBT_EALIGN;

  CoefP c;
  for (int m = 0; m < MTBT_FUSE_MAX_SOURCES; ++m) {
    const bool on = m < M;
    c.mc[m] = on ? a->mc[m] : nullptr;
    c.cbs[m] = on ? a->mc_batch_stride[m] : 0; c.cks[m] = on ? a->mc_k_stride[m] : 0; c.ccs[m] = on ? a->mc_c_stride[m] : 0;
    c.anchors[m] = on ? a->anchors[m] : nullptr;
    c.scores[m] = on ? a->scores[m] : nullptr;
    c.weight[m] = on ? a->weight[m] : 0.f;
    p.protos[m] = on ? a->protos[m] : nullptr;
    p.orient[m] = on ? a->orient[m] : 0;
  }
  c.member_slot = a->member_slot; c.counts = a->counts; c.W = a->W; c.Ss = a->Ss;
  c.M = M; c.K = a->K; c.top_k = a->top_k;
  p.W = a->W; p.counts = a->counts; p.boxes = a->boxes; p.boxes_frame = a->boxes_frame; p.out = a->out;
  p.n_frames = n_frames; p.K = a->top_k; p.G = a->hp; p.M = M;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(vote_coeff_kernel, dim3((a->top_k + VC_ROWS - 1) / VC_ROWS, a->N), dim3(VC_NT), 0, s, c);
  MTBT_LAUNCH_CHECK();
  if (a->crop) {
    if (int rc = mtbt_allow_lds(vote_mask_kernel<true>, (int)FRAME_LDS)) return rc;
    hipLaunchKernelGGL(vote_mask_kernel<true>, dim3((unsigned)blocks), dim3(256), FRAME_LDS, s, p);
  } else {
    if (int rc = mtbt_allow_lds(vote_mask_kernel<false>, (int)FRAME_LDS)) return rc;
    hipLaunchKernelGGL(vote_mask_kernel<false>, dim3((unsigned)blocks), dim3(256), FRAME_LDS, s, p);
  }
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}
