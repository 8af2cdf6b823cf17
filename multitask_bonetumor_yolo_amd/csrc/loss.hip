// Multitask loss VALUE on the device (`MultiTaskLitModel._multitask_loss`, running_main_v3.py:232-387):
// no per-image Python loop, no `.item()` synchronisation.  The value, its gradient (below) and the eval-mode confusion counts.
//
//   det_loss_kernel   4 lanes per (image, anchor), one per box side: softmax expectation of the side's 16-bin
//                     distribution (+ its log-sum-exp for the DFL cross-entropy), box decode, IoU against the image's
//                     GT boxes (first maximum wins, like torch.max), positives = max IoU > threshold; per positive:
//                     1 - IoU, BCE-with-logits(sum) of the class logits against one-hot / label-smoothed targets,
//                     two-bin DFL cross-entropy.  Workgroup partial sums -> workspace (no atomics).
//   bce_kernel        sum of BCE-with-logits over the S x S segmentation logits (the 1x1 projector + bilinear resize is
//                     mtbt_mask_assemble's projector path), workgroup partials.
//   finalize_kernel   fixed-order reduction of the partials, image-classification cross-entropy, normalisation by the
//                     batch's positive count (batch size if none), weighted total.  One workgroup.
//   det_confusion_kernel
//                     the detection confusion matrix of the eval-mode loss (`temp_matched_preds_for_cm`, :349-350): the same
//                     anchors and positives, argmax of each positive's class logits against its GT class, integer counts.
// det_loss_kernel, det_loss_grad_kernel and det_confusion_kernel share one per-anchor decode + match prologue (match_anchor,
// loss_match.h: also the instance-mask loss's), and with the task-aligned loss the DFL target and gradient and the host's level table.
// Deterministic (fixed reduction orders); fp32 with libm exp / log (this file is built with -ffp-contract=off like the rest
// of the post-process so that the IoU matches torch's arithmetic).
#include <cmath>

#include "common.h"
#include "loss_match.h"

namespace {

__global__ __launch_bounds__(256) void det_loss_kernel(const LossP p) {
  __shared__ float red[4][5];
  const int side = threadIdx.x & 3;
  const AnchorMatch am = match_anchor(p, (long)blockIdx.x * 64 + (threadIdx.x >> 2), side);
  float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};   // n_pos, sum(1 - iou), sum(iou), sum(cls bce), sum(dfl)
  if (am.pos) {
    const float lse = am.sd.m + logf(am.sd.s);
    const DflTarget tg = dfl_target(am.at, ld4(p.gt_xyxy + 4 * am.bi), side, p.reg_max);
    const float wl = (float)tg.tr - tg.t, wr = tg.t - (float)tg.tl;
    v[4] = (lse - am.d[tg.tl]) * wl + (lse - am.d[tg.tr]) * wr;
    // class BCE: the group's lanes split the classes
    const int gc = p.gt_cls[am.bi];
    const bool smooth = p.smoothing > 0.f && p.training;
    for (int c = side; c < p.nc; c += 4) {
      const float tgt = smooth ? (c == gc ? 1.f - p.smoothing : p.smoothing / (float)(p.nc - 1)) : (c == gc ? 1.f : 0.f);
      v[3] += bce_logits(am.row[4 * p.reg_max + c], tgt);
    }
    if (side == 0) { v[0] = 1.f; v[1] = 1.f - am.best; v[2] = am.best; }
  }
  block_sum_f32<5>(v, red);   // fixed order, no atomics
  if (threadIdx.x == 0)
#pragma unroll
    for (int q = 0; q < 5; ++q) p.partial[(long)blockIdx.x * 5 + q] = v[q];
}

__global__ __launch_bounds__(256) void bce_kernel(const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ bias,
                                                  long n, float* __restrict__ partial) {
  __shared__ float red[4][1];
  const float b = bias ? *bias : 0.f;
  float s[1] = {0.f};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) s[0] += bce_logits(x[i] + b, t[i]);
  block_sum_f32<1>(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s[0];
}

struct FinP {
  const float* det_partial; int det_blocks;
  const float* seg_partial; int seg_blocks; long seg_n;
  const float* img_logits; const long long* img_gt; int N, n_img_classes;
  float w_seg, w_box, w_dfl, w_cls, w_img;
  float* out;  // total, seg, box, dfl, cls_det, img_cls, n_pos, mean matched IoU
};

__global__ __launch_bounds__(256) void finalize_kernel(const FinP p) {
  __shared__ float red[4][7];
  float v[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // 5 detection sums, seg sum, img CE sum
  for (int b = threadIdx.x; b < p.det_blocks; b += 256)
#pragma unroll
    for (int q = 0; q < 5; ++q) v[q] += p.det_partial[(long)b * 5 + q];
  for (int b = threadIdx.x; b < p.seg_blocks; b += 256) v[5] += p.seg_partial[b];
  for (int i = threadIdx.x; i < p.N; i += 256) {  // CrossEntropyLoss, mean over the batch
    const float* lg = p.img_logits + (long)i * p.n_img_classes;
    float m = -INFINITY;
    for (int c = 0; c < p.n_img_classes; ++c) m = fmaxf(m, lg[c]);
    float s = 0.f;
    for (int c = 0; c < p.n_img_classes; ++c) s += expf(lg[c] - m);
    v[6] += (m + logf(s)) - lg[p.img_gt[i]];
  }
  block_sum_f32<7>(v, red);
  if (threadIdx.x == 0) {
    const float* t = v;
    const float n_pos = t[0];
    const float norm = n_pos > 0.f ? n_pos : (float)p.N;                 // running_main_v3.py:371
    const float box = t[1] / norm, cls = t[3] / norm, dfl = t[4] / norm;
    const float seg = p.seg_n > 0 ? t[5] / (float)p.seg_n : 0.f;
    const float img = t[6] / (float)p.N;
    p.out[0] = p.w_seg * seg + p.w_box * box + p.w_dfl * dfl + p.w_cls * cls + p.w_img * img;
    p.out[1] = seg; p.out[2] = box; p.out[3] = dfl; p.out[4] = cls; p.out[5] = img;
    p.out[6] = n_pos;
    p.out[7] = n_pos > 0.f ? t[2] / n_pos : 0.f;
  }
}

inline long det_blocks_of(long N, long A) { return (N * A + 63) / 64; }
inline long seg_blocks_of(long n) { long b = (n + 256 * 8 - 1) / (256 * 8); return b > 2048 ? 2048 : (b < 1 ? 1 : b); }

// ---- gradient of the weighted total with respect to the three head outputs (first operator of the backward pass) ----
// Same thread mapping as det_loss_kernel.  What autograd does on the reference's expressions:
//   box   d(1 - IoU)/d(corner) through batch_bbox_iou (:71-97; max / min pick the larger / smaller operand, clamp(min=0) passes
//         the gradient where its input is positive), corner = anchor -/+ dist * stride, dist = sum_j softmax(raw)_j * j
//         => d dist / d raw_j = p_j (j - dist)
//   DFL   two-bin cross-entropy: wl (p - onehot(tl)) + wr (p - onehot(tr))
//   class BCE-with-logits(sum): sigmoid(x) - target
// each scaled by its weight / (#positives of the batch, batch size if none) -- read from the forward's out[6].  Anchors that are
// not positives get zeros.  The positives mask and the matched GT index carry no gradient (comparison / argmax).
struct GradP {
  LossP l;
  GradMaps d;
  const float* fwd_out;   // out[8] of mtbt_multitask_loss
  float w_box, w_dfl, w_cls;
};

__global__ __launch_bounds__(256) void det_loss_grad_kernel(const GradP q) {
  const LossP& p = q.l;
  const int side = threadIdx.x & 3;
  const AnchorMatch am = match_anchor(p, (long)blockIdx.x * 64 + (threadIdx.x >> 2), side);
  if (!am.live) return;
  float* drow = q.d.map[am.at.l] + am.at.pix * q.d.ld[am.at.l];
  if (!am.pos) {
    for (int i = 0; i < p.reg_max; ++i) drow[side * p.reg_max + i] = 0.f;
    for (int c = side; c < p.nc; c += 4) drow[4 * p.reg_max + c] = 0.f;
    return;
  }
  const float x1 = am.box.x, y1 = am.box.y, x2 = am.box.z, y2 = am.box.w, st = am.at.st;
  const float n_pos = q.fwd_out[6];
  const float inv = 1.f / (n_pos > 0.f ? n_pos : (float)p.N);
  const float4 b = ld4(p.gt_xyxy + 4 * am.bi);
  // d IoU / d (this lane's corner)
  const float iwr = fminf(x2, b.z) - fmaxf(x1, b.x), ihr = fminf(y2, b.w) - fmaxf(y1, b.y);
  const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
  const float inter = iw * ih;
  const float bw = x2 - x1, bh = y2 - y1;
  const float uni = bw * bh + (b.z - b.x) * (b.w - b.y) - inter + 1e-7f;
  float dinter, darea;   // with respect to the corner owned by `side`
  if (side == 0)      { dinter = (iwr > 0.f && x1 > b.x) ? -ih : 0.f; darea = -bh; }
  else if (side == 1) { dinter = (ihr > 0.f && y1 > b.y) ? -iw : 0.f; darea = -bw; }
  else if (side == 2) { dinter = (iwr > 0.f && x2 < b.z) ? ih : 0.f;  darea = bh; }
  else                { dinter = (ihr > 0.f && y2 < b.w) ? iw : 0.f;  darea = bw; }
  const float diou = (dinter * uni - inter * (darea - dinter)) / (uni * uni);
  const float dcorner = -q.w_box * inv * diou;                       // d total / d corner
  const float ddist = dcorner * (side < 2 ? -st : st);               // corner = anchor -/+ dist * stride
  const DflTarget tg = dfl_target(am.at, b, side, p.reg_max);
  const float wl = (float)tg.tr - tg.t, wr = tg.t - (float)tg.tl;
  dfl_side_grad(am.d, am.sd, p.reg_max, ddist, q.w_dfl * inv, tg, wl, wr, drow + side * p.reg_max, false);
  const int gc = p.gt_cls[am.bi];
  const bool smooth = p.smoothing > 0.f && p.training;
  for (int c = side; c < p.nc; c += 4) {
    const float tgt = smooth ? (c == gc ? 1.f - p.smoothing : p.smoothing / (float)(p.nc - 1)) : (c == gc ? 1.f : 0.f);
    drow[4 * p.reg_max + c] = q.w_cls * inv * (sigmoid(am.row[4 * p.reg_max + c]) - tgt);
  }
}

// d total / d seg logit = w_seg / n * (sigmoid(x + bias) - target);  d total / d img logit = w_img / N * (softmax - onehot)
__global__ __launch_bounds__(256) void seg_img_grad_kernel(const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ bias,
                                                           long n, float k_seg, float* __restrict__ dx, const float* __restrict__ img_logits,
                                                           const long long* __restrict__ img_gt, int N, int ncls, float k_img,
                                                           float* __restrict__ dimg) {
  const float b = bias ? *bias : 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dx[i] = k_seg * (sigmoid(x[i] + b) - t[i]);
  if (blockIdx.x == 0 && dimg) {
    for (int i = threadIdx.x; i < N; i += 256) {
      const float* lg = img_logits + (long)i * ncls;
      float m = -INFINITY;
      for (int c = 0; c < ncls; ++c) m = fmaxf(m, lg[c]);
      float s = 0.f;
      for (int c = 0; c < ncls; ++c) s += expf(lg[c] - m);
      for (int c = 0; c < ncls; ++c) dimg[(long)i * ncls + c] = k_img * (expf(lg[c] - m) / s - (c == img_gt[i] ? 1.f : 0.f));
    }
  }
}


// ---- detection confusion matrix of `_multitask_loss` in eval mode (running_main_v3.py:349-350, :710-722) ----
// Same anchors, decode and match as det_loss_kernel (match_anchor), so its positives are the loss's positives.  Per positive:
// pred = argmax of the nc raw class logits (torch semantics: the first maximum wins, a NaN counts as the maximum), one count at
// [gt_cls][pred].  Counts are summed per workgroup in LDS, then one 64-bit global atomicAdd per non-zero bin per workgroup: integer
// sums, so the result does not depend on the order.  A positive whose GT class lies outside [0, nc) is not counted and sets bit 0 of
// *status (a plain read-modify-write: every writer sets the same bit).  The grid strides over the anchors, 64 per pass.
__global__ __launch_bounds__(256) void det_confusion_kernel(const LossP p, unsigned long long* __restrict__ counts, int* __restrict__ status) {
  __shared__ unsigned int bins[MTBT_CONFUSION_MAX_NC * MTBT_CONFUSION_MAX_NC];
  __shared__ int bad;
  const int nbins = p.nc * p.nc;
  for (int i = threadIdx.x; i < nbins; i += 256) bins[i] = 0u;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  const int side = threadIdx.x & 3;
  const long total = (long)p.N * p.A;
  for (long base = (long)blockIdx.x * 64; base < total; base += (long)gridDim.x * 64) {   // block-uniform: every lane takes part
    const AnchorMatch am = match_anchor(p, base + (threadIdx.x >> 2), side);
    if (am.pos && side == 0) {
      const float* lg = am.row + 4 * p.reg_max;
      int pred = 0;
      float v = lg[0];
      for (int c = 1; c < p.nc && v == v; ++c) {      // stops at the first NaN
        const float x = lg[c];
        if (x != x || x > v) { v = x; pred = c; }
      }
      const int gc = p.gt_cls[am.bi];
      if (gc >= 0 && gc < p.nc) atomicAdd(&bins[gc * p.nc + pred], 1u);
      else bad = 1;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += 256)
    if (bins[i]) atomicAdd(counts + i, (unsigned long long)bins[i]);
  if (threadIdx.x == 0 && bad) *status = *status | 1;
}

}  // namespace

// validated detection fields (maps, GT boxes, match threshold): what det_loss_kernel's prologue reads; with `g`, the gradient maps too
static int fill_det_params(const mtbt_loss_args* a, LossP& p, GradMaps* g = nullptr, float* const* d_map = nullptr, const int32_t* d_ld = nullptr) {
  if (a->n_levels < 1 || a->n_levels > 3 || a->N <= 0 || a->nc <= 0 || a->reg_max <= 0 || a->reg_max > 64) return MTBT_EINVAL;
  if (!a->gt_xyxy || !a->gt_cls || !a->gt_off) return MTBT_EINVAL;
  if (!aligned16(a->gt_xyxy)) return MTBT_EALIGN;
  if (int rc = fill_levels(a, 4 * a->reg_max + a->nc, p, g, d_map, d_ld)) return rc;
  p.N = a->N; p.nc = a->nc; p.reg_max = a->reg_max;
  p.gt_xyxy = a->gt_xyxy; p.gt_cls = a->gt_cls; p.gt_off = a->gt_off;
  p.iou_thresh = a->iou_thresh; p.smoothing = a->label_smoothing; p.training = a->training;
  p.partial = nullptr;
  return MTBT_OK;
}

// validated kernel parameters shared by the value and the gradient entry points
static int fill_loss_params(const mtbt_loss_args* a, LossP& p, GradMaps* g = nullptr, float* const* d_map = nullptr, const int32_t* d_ld = nullptr) {
  if (!a || !a->out || !a->img_logits || !a->img_gt || a->n_img_classes <= 0) return MTBT_EINVAL;
  if ((a->seg_n > 0) != (a->seg_logits != nullptr && a->seg_targets != nullptr)) return MTBT_EINVAL;
  return fill_det_params(a, p, g, d_map, d_ld);
}

extern "C" int64_t mtbt_loss_workspace_bytes(int N, int A, int64_t seg_n) {
  if (N <= 0 || A <= 0 || seg_n < 0) return 0;
  return (det_blocks_of(N, A) * 5 + seg_blocks_of(seg_n)) * (int64_t)sizeof(float);
}

extern "C" int mtbt_multitask_loss(const mtbt_loss_args* a, void* stream) {
  if (!a || !a->workspace) return MTBT_EINVAL;
  LossP p;
  if (int rc = fill_loss_params(a, p)) return rc;
  const long db = det_blocks_of(a->N, p.A), sb = a->seg_n > 0 ? seg_blocks_of(a->seg_n) : 0;
  if (db > 0x7fffffffL) return MTBT_EINVAL;
  if (a->workspace_bytes < mtbt_loss_workspace_bytes(a->N, p.A, a->seg_n)) return MTBT_EWORKSPACE;
  float* det_partial = a->workspace;
  float* seg_partial = det_partial + db * 5;
  p.partial = det_partial;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(det_loss_kernel, dim3((unsigned)db), dim3(256), 0, s, p);
  if (sb > 0) hipLaunchKernelGGL(bce_kernel, dim3((unsigned)sb), dim3(256), 0, s, a->seg_logits, a->seg_targets, a->seg_bias, (long)a->seg_n, seg_partial);
  FinP f;
  f.det_partial = det_partial; f.det_blocks = (int)db; f.seg_partial = seg_partial; f.seg_blocks = (int)sb; f.seg_n = a->seg_n;
  f.img_logits = a->img_logits; f.img_gt = reinterpret_cast<const long long*>(a->img_gt); f.N = a->N; f.n_img_classes = a->n_img_classes;
  f.w_seg = a->w_seg; f.w_box = a->w_box; f.w_dfl = a->w_dfl; f.w_cls = a->w_cls; f.w_img = a->w_img;
  f.out = a->out;
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, s, f);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}

extern "C" int mtbt_multitask_loss_grad(const mtbt_loss_args* a, float* const* d_map, const int32_t* d_map_pixel_stride, float* d_seg_logits,
                                        float* d_img_logits, void* stream) {
  if (!a || !d_map || !d_map_pixel_stride) return MTBT_EINVAL;
  GradP q;
  if (int rc = fill_loss_params(a, q.l, &q.d, d_map, d_map_pixel_stride)) return rc;
  if (a->seg_n > 0 && !d_seg_logits) return MTBT_EINVAL;
  q.fwd_out = a->out; q.w_box = a->w_box; q.w_dfl = a->w_dfl; q.w_cls = a->w_cls;
  const long db = det_blocks_of(a->N, q.l.A);
  if (db > 0x7fffffffL) return MTBT_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(det_loss_grad_kernel, dim3((unsigned)db), dim3(256), 0, s, q);
  const long sb = a->seg_n > 0 ? seg_blocks_of(a->seg_n) : 1;
  hipLaunchKernelGGL(seg_img_grad_kernel, dim3((unsigned)sb), dim3(256), 0, s, a->seg_logits, a->seg_targets, a->seg_bias, (long)a->seg_n,
                     a->seg_n > 0 ? a->w_seg / (float)a->seg_n : 0.f, d_seg_logits, a->img_logits, reinterpret_cast<const long long*>(a->img_gt), a->N,
                     a->n_img_classes, a->w_img / (float)a->N, d_img_logits);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}

extern "C" int mtbt_det_confusion(const mtbt_loss_args* a, int64_t* counts, int32_t* status, void* stream) {
  if (!a || !counts || !status || a->nc > MTBT_CONFUSION_MAX_NC) return MTBT_EINVAL;
  LossP p;
  if (int rc = fill_det_params(a, p)) return rc;
  const long db = det_blocks_of(a->N, p.A);
  const unsigned grid = (unsigned)(db < 1024 ? db : 1024);
  hipLaunchKernelGGL(det_confusion_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p,
                     reinterpret_cast<unsigned long long*>(counts), reinterpret_cast<int*>(status));
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}
