// Instance masks and boxes in the ORIGINAL image frame, masks one bit per pixel (mtbt_masks_to_frames).  The algorithm and every piece of
// the kernel but its own way to `low` are in frame_tile.h: here a group's 16 coefficient rows are gathered through the kept anchors, one
// group ahead, and one prototype patch per tile serves every group.
#include "common.h"
#include "frame_tile.h"

namespace {

using namespace frame_tile;

struct FrameP {
  const float* protos;
  const float* coeff;
  long cbs, cks, ccs;
  const int* gather;
  const int* counts;
  const float* boxes;
  float* boxes_frame;
  unsigned char* out;
  int n_frames, K, hp, wp;
  FrameD f[MAX_FRAMES];
};

template <bool CROP>
__global__ __launch_bounds__(256) void frame_mask_kernel(const FrameP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Lds s = lds_layout(smem);
  const int tid = threadIdx.x;
  const TileCtx c = tile_context(p.f, p.n_frames, p.out, 0);
  const FrameD& f = p.f[c.n];
  const int n = c.n, cnt = p.counts ? max(min(p.counts[n], p.K), 0) : p.K;
  write_frame_boxes(c, f, p.boxes, p.boxes_frame, p.K, cnt);
  const Patch pt = patch_under(c.X0, c.Xl, c.Y0, c.Yl, f.step, 0, 0, p.hp, p.wp);
  const float* pr = p.protos + (long)n * p.hp * p.wp * NM;

  float cpre[2];
  float bpre = 0.f;
  auto fetch_group = [&](int g) {   // coefficients (gather index -> coefficient: two dependent loads) and boxes, one group ahead
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = tid + u * 256, b = i >> 5, ch = i & 31;
      float v = 0.f;
      if (g + b < cnt) {
        const long kk = p.gather ? p.gather[(long)n * p.K + g + b] : (g + b);
        v = p.coeff[(long)n * p.cbs + kk * p.cks + ch * p.ccs];
      }
      cpre[u] = v;
    }
    if (CROP && tid < 64) {
      const int b = tid >> 2;
      bpre = g + b < cnt ? frame_box(p.boxes[((long)n * p.K + g + b) * 4 + (tid & 3)], f.scale, tid & 3, c.H0, c.W0) : 0.f;
    }
  };

  bool staged = false;
  if (cnt > 0) fetch_group(0);
  for (int g0 = 0; g0 < cnt; g0 += 16) {
    const int nb = min(16, cnt - g0);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = tid + u * 256;
      s.coef[(i >> 5) * PPITCH + (i & 31)] = cpre[u];
    }
    if (!CROP) __syncthreads();   // (with cropping group_hit's barrier publishes coef too)
    const bool ghit = group_hit<CROP>(c, s.boxs, bpre, nb);
    if (g0 + 16 < cnt) fetch_group(g0 + 16);
    if (ghit) {
      if (!staged) {
        stage_patch(s.patch, pr, pt, [&](int y, int x) { return (long)y * p.wp + x; });
        staged = true;
        __syncthreads();
      }
      mfma_to_low(s, pt.NPXP);
      __syncthreads();
    }
    unsigned long long word[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) word[b] = 0ull;
    if (ghit) sample_words<CROP>(c, s, pt, f.step, p.hp, p.wp, nb, word);
    store_words(c, word, g0, nb);
    __syncthreads();   // coef / low / boxs are rewritten by the next group
  }
  zero_tail(c, cnt, p.K);
}

}  // namespace

extern "C" int mtbt_sizeof_frame_args(int which) {
  switch (which) {
    case 0: return (int)sizeof(mtbt_frame);
    case 1: return (int)sizeof(mtbt_frame_mask_args);
    default: return -1;
  }
}

extern "C" int mtbt_masks_to_frames(const mtbt_frame_mask_args* a, const mtbt_frame* frames, int n_frames, void* stream) {
  if (!a || !frames || !a->protos || !a->coeff || !a->out) return MTBT_EINVAL;
  if (!frame_args_ok(n_frames, a->N, a->nm, a->K, a->hp, a->wp, a->out_bytes)) return MTBT_EINVAL;
  if ((a->crop || a->boxes_frame) && !a->boxes) return MTBT_EINVAL;
  FrameP p;
  long blocks = 0;
  if (int rc = frame_layout(frames, n_frames, a->K, a->hp, a->wp, a->boxes != nullptr, a->out_bytes, nullptr, nullptr, MAX_UNITS, 8, p.f, blocks))
    return rc;
  if (!aligned16(a->protos) || !aligned16(a->out)) return MTBT_EALIGN;
  p.protos = a->protos; p.coeff = a->coeff;
  p.cbs = a->coeff_batch_stride; p.cks = a->coeff_k_stride; p.ccs = a->coeff_c_stride;
  p.gather = a->gather_idx; p.counts = a->counts; p.boxes = a->boxes; p.boxes_frame = a->boxes_frame; p.out = a->out;
  p.n_frames = n_frames; p.K = a->K; p.hp = a->hp; p.wp = a->wp;
  return launch_mask_kernel(a->crop ? frame_mask_kernel<true> : frame_mask_kernel<false>, blocks, p, reinterpret_cast<hipStream_t>(stream));
}
