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

// a pair = (detection box, GT box), both staged in LDS; the IoU is recomputed in fp64 per pair (no D x G matrix)
struct BoxPairs {
  using Args = mtbt_box_eval_args;
  struct Lds { float4 dbox[CAP], gbox[CAP]; };
  const Args& p;
  Lds& s;
  __device__ bool gt_in_batch(long g, double& area) const {
    const float* r = p.gt + g * 6;
    const float bi = r[0];
    if (!(bi >= 0.f && bi < (float)p.B && bi == truncf(bi))) return false;
    area = box_area(gt_box(r, p.gt_format, p.img_size));
    return true;
  }
  __device__ void load_det(int i, long at) { s.dbox[i] = reinterpret_cast<const float4*>(p.boxes)[at]; }
  __device__ bool gt_of(int g, int b) const { return p.gt[(long)g * 6] == (float)b; }
  __device__ double load_gt(int g, int pos, int& cls) {
    const float* r = p.gt + (long)g * 6;
    const float4 box = gt_box(r, p.gt_format, p.img_size);
    s.gbox[pos] = box;
    cls = (int)(long long)r[1];
    return box_area(box);
  }
  __device__ double iou(int i, int j) const { return box_iou(s.dbox[i], s.gbox[j]); }
  __device__ double det_area(int i) const { return box_area(s.dbox[i]); }
};

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
  hipLaunchKernelGGL(coco_match_kernel<BoxPairs>, dim3((unsigned)p.B, NA), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), p);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}
