// COCO box matching on the device: pycocotools `COCOeval.evaluateImg` (iouType "bbox", no crowd boxes) for a whole batch of
// images in one launch, feeding `metrics.DeviceMeanAveragePrecision` (the torchmetrics `MeanAveragePrecision` objects of
// running_main_v3.py:209-217 and evaluate_model.py:81-93).  The once-per-epoch accumulation (`accumulate` / `summarize`) runs
// on the host over the compact per-detection records written here.
//
// Inputs of one batch of B images: detections padded to [B][K] (xyxy fp32 boxes, fp32 scores, int64 labels; the first
// counts[b] slots of image b are valid, counts == NULL => all K), GT rows [M][6] fp32 (batch_idx, cls, a, b, c, d):
//   gt_format 0: (cx, cy, w, h) normalised, converted in fp32 with validation_step's per-box formula (:566; the reference
//                concatenates the four columns and views them as [-1, 4], which mixes boxes when an image has several):
//                x1 = (cx - w/2) * S, y1 = (cy - h/2) * S, x2 = (cx + w/2) * S, y2 = (cy + h/2) * S, each clamped to [0, S]
//   gt_format 1: (x1, y1, x2, y2) pixels.
// A row belongs to image b when batch_idx == (float)b; the GT boxes of an image keep their row order.
//
// Semantics, per (image, class) -- detections of class c are compared with the GT boxes of class c only:
//   order      detections by score descending, stable on the slot index (numpy mergesort on -score); the first max_det
//              are kept; rank = position in that order, -1 for invalid or truncated slots
//   IoU        fp64 from the fp32 coordinates in the operation order of metrics.box_iou_xyxy:
//              iw = max(min(a2,b2) - max(a0,b0), 0), ih likewise, inter = iw*ih,
//              union = (a2-a0)*(a3-a1) + (b2-b0)*(b3-b1) - inter, IoU = union > 0 ? inter/union : 0
//              (this file is built with -ffp-contract=off: every match decision is bit-identical to the host class)
//   areas      all [0, 1e10], small [0, 32^2], medium [32^2, 96^2], large [96^2, 1e10], both bounds inclusive, area =
//              (x2-x1)*(y2-y1) in fp64; a GT box outside range a is IGNORED for a
//   matching   per (area range a, threshold t), lim = min(t, 1 - 1e-10), detections in rank order:
//              a detection takes the free non-ignored GT box of highest IoU >= lim (equal IoU: the later box -- pycocotools
//              tests with `<`); only when there is none, the best free ignored GT box by the same rule (pycocotools' `break`
//              at the first ignored box after a non-ignored match, over GT sorted stably non-ignored first); a matched GT
//              box is no longer free for (a, t); a detection is IGNORED for (a, t) if it matched an ignored GT box, or if it
//              is unmatched and its own area lies outside a
// Matching runs once with the largest max-detection threshold: the smaller ones are prefixes (accumulate slices
// dtm[:, :maxDet] the same way).
//
// Outputs: rank [B][K] int32, match [B][K][4] and ignore [B][K][4] uint32 (word a = area range, bit t = threshold t),
// gt_area [M] uint32 (bit a set: the row is not ignored in range a; 0 for rows of no image of the batch), and one status
// word the kernel sets to 1 when an image holds more than 1024 GT rows (that image's detections are then written as
// invalid).  The caller zeroes the status word; nothing here clears it.
//
// Shape: one 1024-thread workgroup per (image, area range).  The image's detections and GT boxes are staged in LDS
// (~60 KiB at the caps); ranks by counting in LDS (O(n^2) compares over a total order on (score, slot), so the walk order
// is a permutation); then wave w walks the detections for thresholds w, w + 16, ...: lanes span the GT boxes in chunks
// of 64 with the IoU recomputed in fp64 (no D x G matrix), a two-candidate wave argmax (non-ignored / ignored) with the
// tie -> higher index rule, and the free-GT set as one bit per (lane, chunk) in a register.  Latency-bound: the chain of
// a threshold is as long as the image's kept detections.
#include <climits>
#include <cmath>

#include "common.h"
#include "coco_eval.h"

namespace {

__device__ __forceinline__ double box_area(float4 b) { return ((double)b.z - (double)b.x) * ((double)b.w - (double)b.y); }

__device__ __forceinline__ double box_iou(float4 p, float4 q) {
  const double a0 = p.x, a1 = p.y, a2 = p.z, a3 = p.w, b0 = q.x, b1 = q.y, b2 = q.z, b3 = q.w;
  double iw = fmin(a2, b2) - fmax(a0, b0), ih = fmin(a3, b3) - fmax(a1, b1);
  iw = iw < 0.0 ? 0.0 : iw;
  ih = ih < 0.0 ? 0.0 : ih;
  const double inter = iw * ih;
  const double uni = ((a2 - a0) * (a3 - a1) + (b2 - b0) * (b3 - b1)) - inter;
  return uni > 0.0 ? inter / uni : 0.0;
}

__device__ __forceinline__ float clamp_s(float v, float S) { return v < 0.f ? 0.f : (v > S ? S : v); }   // torch clamp_(0, S): NaN stays

__device__ __forceinline__ float4 gt_box(const float* r, int fmt, float S) {
  if (fmt == 1) return make_float4(r[2], r[3], r[4], r[5]);
  const float cx = r[2], cy = r[3], w = r[4], h = r[5];
  return make_float4(clamp_s((cx - w / 2.f) * S, S), clamp_s((cy - h / 2.f) * S, S), clamp_s((cx + w / 2.f) * S, S),
                     clamp_s((cy + h / 2.f) * S, S));
}

__global__ __launch_bounds__(NT) void box_eval_kernel(const mtbt_box_eval_args p) {
  __shared__ float4 dbox[CAP];
  __shared__ int dkey[CAP], dlab[CAP], order[CAP];
  __shared__ unsigned mword[CAP], iword[CAP];
  __shared__ float4 gbox[CAP];
  __shared__ int gcls[CAP], gign[CAP];
  __shared__ int wcnt[NW];

  const int b = blockIdx.x, a = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K, M = p.M, fmt = p.gt_format;
  const float S = p.img_size;

  // every GT row's area-range set, each row written by exactly one workgroup of the grid
  for (long g = (long)(b * NA + a) * NT + tid; g < M; g += (long)p.B * NA * NT) {
    const float* r = p.gt + g * 6;
    const float bi = r[0];
    unsigned bits = 0;
    if (bi >= 0.f && bi < (float)p.B && bi == truncf(bi)) {
      const double area = box_area(gt_box(r, fmt, S));
#pragma unroll
      for (int q = 0; q < NA; ++q) bits |= in_area(area, q) ? 1u << q : 0u;
    }
    p.gt_area[g] = bits;
  }

  int n = K;
  if (p.counts) {
    n = p.counts[b];
    n = n < 0 ? 0 : (n > K ? K : n);
  }
  const long row = (long)b * K;
  if (tid < n) {
    dbox[tid] = reinterpret_cast<const float4*>(p.boxes)[row + tid];
    dkey[tid] = score_key(p.scores[row + tid]);
    dlab[tid] = (int)p.labels[row + tid];
    mword[tid] = 0u;
    iword[tid] = 0u;
  }
  __syncthreads();   // the rank loop reads every slot; the GT loop below has barriers only when M > 0

  // the image's GT rows, compacted in row order (ballot prefix within a wave, wave counts across the workgroup)
  int ng = 0;
  for (int base = 0; base < M; base += NT) {
    const int g = base + tid;
    bool mine = false;
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
    int cls = 0;
    if (g < M) {
      const float* r = p.gt + (long)g * 6;
      mine = r[0] == (float)b;
      if (mine) {
        box = gt_box(r, fmt, S);
        cls = (int)(long long)r[1];
      }
    }
    const unsigned long long bal = __ballot(mine);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      off += w < wave ? wcnt[w] : 0;
      tot += wcnt[w];
    }
    const int pos = ng + off + __popcll(bal & ((1ull << lane) - 1ull));
    if (mine && pos < CAP) {
      gbox[pos] = box;
      gcls[pos] = cls;
      gign[pos] = in_area(box_area(box), a) ? 0 : 1;
    }
    ng += tot;
    __syncthreads();
  }

  if (ng > CAP) {   // uniform over the workgroup: the image is reported, its detections are written as invalid
    if (tid == 0) p.status[0] = 1;
    if (tid < K) {
      if (a == 0) p.rank[row + tid] = -1;
      p.match[(row + tid) * NA + a] = 0u;
      p.ignore[(row + tid) * NA + a] = 0u;
    }
    return;
  }

  // rank within (image, class) and position in the image's global score order
  if (tid < n) {
    const int ki = dkey[tid], li = dlab[tid];
    int pos = 0, rk = 0;
    for (int j = 0; j < n; ++j) {
      const int kj = dkey[j];
      const bool before = kj > ki || (kj == ki && j < tid);
      pos += before;
      rk += (before && dlab[j] == li) ? 1 : 0;
    }
    const bool kept = rk < p.max_det;
    order[pos] = kept ? tid : -1;
    if (a == 0) p.rank[row + tid] = kept ? rk : -1;
  } else if (tid < K && a == 0) {
    p.rank[row + tid] = -1;
  }
  __syncthreads();

  const int nchunk = (ng + 63) >> 6;   // <= 16 (ng <= CAP)
  for (int t = wave; t < p.T; t += NW) {
    const double lim = fmin(p.iou_thresholds[t], 1.0 - 1e-10);
    unsigned used = 0u;   // bit c: GT box c * 64 + lane is matched
    for (int q = 0; q < n; ++q) {
      const int i = order[q];
      if (i < 0) continue;
      const float4 d = dbox[i];
      const int lab = dlab[i];
      double vn = -INFINITY, vi = -INFINITY;
      int jn = -1, ji = -1;
      for (int c = 0; c < nchunk; ++c) {
        const int j = (c << 6) + lane;
        if (j < ng && gcls[j] == lab && !((used >> c) & 1u)) {
          const double v = box_iou(d, gbox[j]);
          if (v >= lim) {
            if (gign[j]) {
              if (v >= vi) { vi = v; ji = j; }
            } else if (v >= vn) {
              vn = v; jn = j;
            }
          }
        }
      }
      wave_argmax(vn, jn);
      wave_argmax(vi, ji);
      const int m = jn >= 0 ? jn : ji;
      if (m >= 0 && (m & 63) == lane) used |= 1u << (m >> 6);
      if (lane == 0) {
        if (m >= 0) atomicOr(&mword[i], 1u << t);
        if (m >= 0 ? jn < 0 : !in_area(box_area(d), a)) atomicOr(&iword[i], 1u << t);
      }
    }
  }
  __syncthreads();
  if (tid < K) {
    p.match[(row + tid) * NA + a] = tid < n ? mword[tid] : 0u;
    p.ignore[(row + tid) * NA + a] = tid < n ? iword[tid] : 0u;
  }
}

template <typename T> bool aligned_to(const T* ptr) { return (reinterpret_cast<uintptr_t>(ptr) % sizeof(T)) == 0; }

}  // namespace

extern "C" int mtbt_box_eval(const mtbt_box_eval_args* args, void* stream) {
  if (!args) return MTBT_EINVAL;
  const mtbt_box_eval_args& p = *args;
  if (p.T < 1 || p.T > 32 || p.K < 1 || p.K > CAP || p.B < 0 || p.M < 0 || p.max_det < 1 || (p.gt_format != 0 && p.gt_format != 1))
    return MTBT_EINVAL;
  if (!p.boxes || !p.scores || !p.labels || !p.rank || !p.match || !p.ignore || !p.status) return MTBT_EINVAL;
  if (p.M > 0 && (!p.gt || !p.gt_area)) return MTBT_EINVAL;
  if (p.gt_format == 0 && !(p.img_size > 0.f)) return MTBT_EINVAL;
  if (!aligned16(p.boxes) || !aligned_to(p.scores) || !aligned_to(p.labels) || !aligned_to(p.counts) || !aligned_to(p.gt) ||
      !aligned_to(p.rank) || !aligned_to(p.match) || !aligned_to(p.ignore) || !aligned_to(p.gt_area) || !aligned_to(p.status))
    return MTBT_EALIGN;
  if (p.B == 0) return MTBT_OK;
  hipLaunchKernelGGL(box_eval_kernel, dim3((unsigned)p.B, NA), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), p);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}
