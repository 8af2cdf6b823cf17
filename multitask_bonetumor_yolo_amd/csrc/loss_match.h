// The per-anchor decode + match prologue shared by the detection loss (loss.hip: value, gradient, confusion counts) and the
// instance-mask loss (mask_loss.hip): one definition, so that every consumer sees the same positives.  Files that include it are built
// with -ffp-contract=off (the IoU must round like torch's).
#pragma once
#include <cmath>

#include "common.h"

namespace {

struct LossP {
  const float* map[3];
  int h[3], w[3], ld[3];
  int off[4];
  float stride[3];
  int n_levels, N, A, nc, reg_max;
  const float* gt_xyxy;   // [G][4]
  const int* gt_cls;      // [G]
  const int* gt_off;      // [N+1]
  float iou_thresh, smoothing;
  int training;
  float* partial;         // [blocks][5]: n_pos, sum(1-iou), sum(iou), sum(cls bce), sum(dfl)
};

__device__ __forceinline__ float iou_xyxy(float ax1, float ay1, float ax2, float ay2, float bx1, float by1, float bx2, float by2) {
  // running_main_v3.py:71-97
  const float iw = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.f), ih = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.f);
  const float inter = iw * ih;
  const float a1 = (ax2 - ax1) * (ay2 - ay1), a2 = (bx2 - bx1) * (by2 - by1);
  return inter / (a1 + a2 - inter + 1e-7f);
}

__device__ __forceinline__ float bce_logits(float x, float t) {  // torch: max(x,0) - x*t + log(1 + exp(-|x|))
  return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
}

// Per-anchor prologue shared by det_loss_kernel, det_loss_grad_kernel and det_confusion_kernel: 4 lanes per (image, anchor)
// g, one per box side.  Softmax expectation of the side's reg_max-bin distribution, trainer decode (stride = img_size / w,
// running_main_v3.py:266-290), IoU against the image's GT boxes (:316, first maximum wins like torch.max), positive = max IoU >
// iou_thresh (:319-321).  Every lane of a wave must call it (the decode exchanges the four sides with __shfl); lanes of an anchor
// beyond N * A compute anchor 0 of image 0 and come back with live = pos = false.
struct AnchorMatch {
  const float* row;     // the anchor's map row: 4 * reg_max distribution logits, then nc class logits
  const float* d;       // this lane's side: row + side * reg_max
  long pix;             // n * h_l * w_l + cell: the anchor's pixel in level l's maps
  int l, bi;            // level; matched GT row (-1 if the image has none)
  float m, s, dist;     // side distribution: max logit, sum of exp(logit - m), expectation
  float st, ax, ay;     // stride, anchor point in pixels
  float x1, y1, x2, y2; // decoded box
  float best;           // max IoU
  bool live, pos;
};

__device__ __forceinline__ AnchorMatch match_anchor(const LossP& p, long g, int side) {
  AnchorMatch r;
  const long total = (long)p.N * p.A;
  r.live = g < total;
  const long gg = r.live ? g : 0;
  const int n = (int)(gg / p.A), a = (int)(gg - (long)n * p.A);
  int l = 0;
  if (p.n_levels > 1 && a >= p.off[1]) l = 1;
  if (p.n_levels > 2 && a >= p.off[2]) l = 2;
  const int cell = a - p.off[l];
  const int w = p.w[l], hw = p.h[l] * w;
  const int cy = cell / w, cx = cell - cy * w;
  r.l = l;
  r.pix = (long)n * hw + cell;
  r.row = p.map[l] + r.pix * p.ld[l];
  r.d = r.row + side * p.reg_max;
  const float* d = r.d;

  // this side's distribution: expectation (and the pieces of its log-sum-exp)
  float m = -INFINITY;
  for (int i = 0; i < p.reg_max; ++i) m = fmaxf(m, d[i]);
  float s = 0.f;
  for (int i = 0; i < p.reg_max; ++i) s += expf(d[i] - m);
  float dist = 0.f;
  for (int i = 0; i < p.reg_max; ++i) dist += (expf(d[i] - m) / s) * (float)i;
  r.m = m; r.s = s; r.dist = dist;

  const int qbase = (threadIdx.x & 63) & ~3;
  const float st = p.stride[l];
  const float ax = (cx + 0.5f) * st, ay = (cy + 0.5f) * st;
  r.st = st; r.ax = ax; r.ay = ay;
  r.x1 = ax - __shfl(dist, qbase + 0, 64) * st; r.y1 = ay - __shfl(dist, qbase + 1, 64) * st;
  r.x2 = ax + __shfl(dist, qbase + 2, 64) * st; r.y2 = ay + __shfl(dist, qbase + 3, 64) * st;

  // match against this image's GT boxes (every lane of the group computes the same thing)
  const int g0 = p.gt_off[n], g1 = p.gt_off[n + 1];
  float best = -INFINITY;
  int bi = -1;
  for (int k = g0; k < g1; ++k) {
    const float4 b = *reinterpret_cast<const float4*>(p.gt_xyxy + 4 * k);
    const float v = iou_xyxy(r.x1, r.y1, r.x2, r.y2, b.x, b.y, b.z, b.w);
    if (v > best) { best = v; bi = k; }
  }
  r.best = best; r.bi = bi;
  r.pos = r.live && bi >= 0 && best > p.iou_thresh;
  return r;
}

}  // namespace
