// Instance masks of fused detections voted over the members of their clusters (mtbt_vote_masks; the definition is in include/mtbt_hip.h,
// tests/vote_reference.py restates it).
//
//   W[n,r,m,:]   = (sum over the members c of source m of s_c * coeff_c[:]) / Ss[n,r]        -- vote_coeff_kernel (vote_coeff.h)
//   low[n,r,y,x] = sum_m sum_c W[n,r,m,c] * U_m[n,y,x,c]                                     -- vote_mask_kernel: fp32 MFMA over M sources
//   bit          = bilinear(low)(X, Y) > 0 (&& inside the fused frame box when cropping)     -- frame_tile.h
//
// vote_mask_kernel is the tile walk of frame_tile.h with a loop over the sources inside each group: source m's patch is staged
// through the index map of orient[m] (the upright rectangle under the tile is a rectangle of the view, possibly transposed and mirrored),
// and the MFMA accumulators stay in registers from one source to the next.  One patch buffer: the LDS footprint, and with it two
// workgroups per CU, is mask_frame.hip's.  A (group, source) pair whose 16 x 32 coefficients are all zero -- the source has no member in
// any of the 16 clusters -- is skipped, and the patch in LDS is kept when the next pair needs the same source (always, with one source).
#include "common.h"
#include "frame_tile.h"
#include "vote_coeff.h"

// No FMA contraction in this file (built with -ffp-contract=off, see build.py), as in mask_frame.hip and box_fuse.hip.

namespace {

using namespace frame_tile;

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

// image n's candidates: slot k of source m, its score times the source's weight
struct SourceCandidates {
  const CoefP& p;
  int n, groups, width;
  __device__ int slot(int c) const { return p.member_slot[(long)n * groups * p.K + c]; }
  __device__ float score(int c) const {
    const int m = c / p.K, k = c - m * p.K;
    return __fmul_rn(p.scores[m][(long)n * p.K + k], p.weight[m]);
  }
  __device__ float coeff(int m, int k, int ch) const {
    const long a = p.anchors[m][(long)n * p.K + k];
    return p.mc[m][(long)n * p.cbs[m] + a * p.cks[m] + ch * p.ccs[m]];
  }
};

__global__ __launch_bounds__(VC_NT) void vote_coeff_kernel(const CoefP p) {
  const int n = blockIdx.y;
  vote_coeff_rows(SourceCandidates{p, n, p.M, p.M}, n, p.K, p.top_k, p.counts, p.W, p.Ss);
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
  const Lds s = lds_layout(smem);
  const int tid = threadIdx.x, wave = tid >> 6;
  const TileCtx c = tile_context(p.f, p.n_frames, p.out, 0);
  const FrameD& f = p.f[c.n];
  const int n = c.n, G = p.G, M = p.M, cnt = max(min(p.counts[n], p.K), 0);
  write_frame_boxes(c, f, p.boxes, p.boxes_frame, p.K, cnt);
  const Patch pt = patch_under(c.X0, c.Xl, c.Y0, c.Yl, f.step, 0, 0, G, G);   // upright
  const int npg = pt.NPXP / 16;

  int staged = -1;   // the source whose patch is in LDS (workgroup-uniform)
  for (int g0 = 0; g0 < cnt; g0 += 16) {
    const int nb = min(16, cnt - g0);
    float bv = 0.f;
    if (CROP && tid < 64) bv = g0 + (tid >> 2) < cnt ? frame_box(p.boxes[((long)n * p.K + g0) * 4 + tid], f.scale, tid & 3, c.H0, c.W0) : 0.f;
    const bool ghit = group_hit<CROP>(c, s.boxs, bv, nb);
    if (ghit) {
      // low[16][NPXP] = sum_m coef_m[16][32] x patch_m^T; wave w carries column groups w, w+4, ... over the sources
      f32x4 acc[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int m = 0; m < M; ++m) {
        if (stage_vote_coef(s.coef, p.W, n, p.K, M, m, g0, cnt)) {
          if (staged != m) {
            const int o = p.orient[m];
            stage_patch(s.patch, p.protos[m] + (long)n * G * G * NM, pt, [&](int y, int x) {   // upright prototype pixel (y, x) ...
              const int a = (o & 4) ? x : y, b = (o & 4) ? y : x;                              // ... in the view: row a, column b, then the flips
              const int sy = (o & 2) ? G - 1 - a : a, sx = (o & 1) ? G - 1 - b : b;
              return (long)sy * G + sx;
            });
            staged = m;
            __syncthreads();
          }
          float a[8];
          coef_fragment(s.coef, a);
#pragma unroll
          for (int i = 0; i < 6; ++i)
            if (wave + 4 * i < npg) mfma_columns(s.patch, a, wave + 4 * i, acc[i]);
        }
        __syncthreads();   // coef (and the patch) are rewritten for the next source
      }
#pragma unroll
      for (int i = 0; i < 6; ++i)
        if (wave + 4 * i < npg) spill_low(s.low, wave + 4 * i, acc[i]);
      __syncthreads();
    }
    unsigned long long word[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) word[b] = 0ull;
    if (ghit) sample_words<CROP>(c, s, pt, f.step, G, G, nb, word);
    store_words(c, word, g0, nb);
    __syncthreads();   // low / boxs are rewritten by the next group
  }
  zero_tail(c, cnt, p.K);
}

}  // namespace

extern "C" int mtbt_sizeof_vote_mask_args(void) { return (int)sizeof(mtbt_vote_mask_args); }

extern "C" int mtbt_vote_masks(const mtbt_vote_mask_args* a, const mtbt_frame* frames, int n_frames, void* stream) {
  if (!a || !frames || !a->out || !a->member_slot || !a->counts || !a->W || !a->Ss) return MTBT_EINVAL;
  const int M = a->n_sources;
  if (M < 1 || M > MTBT_FUSE_MAX_SOURCES) return MTBT_EINVAL;
  if (!frame_args_ok(n_frames, a->N, a->nm, a->top_k, a->hp, a->wp, a->out_bytes)) return MTBT_EINVAL;
  if (a->K < 1 || (long)M * a->K > MTBT_FUSE_MAX_CANDIDATES || a->hp != a->wp) return MTBT_EINVAL;
  for (int m = 0; m < M; ++m) {
    if (a->orient[m] < 0 || a->orient[m] > 7) return MTBT_EINVAL;
    if (!a->protos[m] || !a->mc[m] || !a->anchors[m] || !a->scores[m]) return MTBT_EINVAL;
  }
  if ((a->crop || a->boxes_frame) && !a->boxes) return MTBT_EINVAL;
  VoteP p;
  long blocks = 0;
  if (int rc = frame_layout(frames, n_frames, a->top_k, a->hp, a->wp, a->boxes != nullptr, a->out_bytes, nullptr, nullptr, MAX_UNITS, 8, p.f, blocks))
    return rc;
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
  return launch_mask_kernel(a->crop ? vote_mask_kernel<true> : vote_mask_kernel<false>, blocks, p, s);
}
