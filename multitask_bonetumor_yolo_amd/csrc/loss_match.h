// The prologue shared by the losses that start from the raw Detect maps and the grouped GT rows: the detection loss (loss.hip: value,
// gradient, confusion counts), the task-aligned detection loss (det_loss_tal.hip) and the instance-mask loss (mask_loss.hip).  One
// definition of the anchor walk, the side decode, the DFL target and gradient, the IoU match and the host's level table, so that every
// consumer sees the same anchors, boxes and positives.  Files that include it are built with -ffp-contract=off (the IoU must round like
// torch's).
#pragma once
#include <climits>
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

// the gradient maps of a loss that differentiates with respect to the Detect maps: NHWC rows like LossP::map
struct GradMaps {
  float* map[3];
  int ld[3];
};

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ float sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

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

// ---- anchor walk: (image, anchor) -> level, pixel of the level's maps, stride (img_size / w, running_main_v3.py:266), anchor point ----
struct AnchorAt {
  int n, a, l;
  long pix;             // n * h_l * w_l + cell: the anchor's pixel in level l's maps
  float st, ax, ay;     // stride, anchor point in pixels
};

__device__ __forceinline__ AnchorAt anchor_at(const LossP& p, int n, int a) {
  AnchorAt r;
  int l = 0;
  if (p.n_levels > 1 && a >= p.off[1]) l = 1;
  if (p.n_levels > 2 && a >= p.off[2]) l = 2;
  const int cell = a - p.off[l];
  const int w = p.w[l], hw = p.h[l] * w;
  const int cy = cell / w, cx = cell - cy * w;
  r.n = n; r.a = a; r.l = l;
  r.pix = (long)n * hw + cell;
  r.st = p.stride[l];
  r.ax = (cx + 0.5f) * r.st; r.ay = (cy + 0.5f) * r.st;
  return r;
}

// ... from the flat index i = n * A + a of the 4-lanes-per-anchor kernels
__device__ __forceinline__ AnchorAt anchor_at(const LossP& p, long i) {
  const int n = (int)(i / p.A);
  return anchor_at(p, n, (int)(i - (long)n * p.A));
}

__device__ __forceinline__ const float* anchor_row(const LossP& p, const AnchorAt& at) { return p.map[at.l] + at.pix * p.ld[at.l]; }

// ---- side decode: one box side's reg_max-bin distribution d -> max logit, sum of exp(logit - max), softmax expectation ----
struct SideDist {
  float m, s, dist;
};

__device__ __forceinline__ SideDist side_dist(const float* d, int reg_max) {
  SideDist r;
  r.m = -INFINITY;
  for (int i = 0; i < reg_max; ++i) r.m = fmaxf(r.m, d[i]);
  r.s = 0.f;
  for (int i = 0; i < reg_max; ++i) r.s += expf(d[i] - r.m);
  r.dist = 0.f;
  for (int i = 0; i < reg_max; ++i) r.dist += (expf(d[i] - r.m) / r.s) * (float)i;
  return r;
}

// The trainer's decode (running_main_v3.py:266-290): the anchor's four lanes (one per side) exchange their expectations.  EVERY lane of
// the wave must call it (__shfl): a lane of an anchor beyond N * A decodes anchor 0 of image 0 and drops the result.
__device__ __forceinline__ float4 decode_box(const AnchorAt& at, float dist) {
  const int qbase = (threadIdx.x & 63) & ~3;
  float4 b;
  b.x = at.ax - __shfl(dist, qbase + 0, 64) * at.st; b.y = at.ay - __shfl(dist, qbase + 1, 64) * at.st;
  b.z = at.ax + __shfl(dist, qbase + 2, 64) * at.st; b.w = at.ay + __shfl(dist, qbase + 3, 64) * at.st;
  return b;
}

// ---- DFL: the two-bin distribution cross-entropy of a box side (running_main_v3.py:351-367) ----
// Target of `side`: t = clamp(distance from the anchor point to the GT side / stride, 0, reg_max - 1 - 0.01), its bins tl = floor(t) and
// tr = tl + 1 (tl = tr = 0 for reg_max == 1).  The two bin weights are the caller's: the reference loss takes (tr - t, t - tl), the
// task-aligned loss (tr - t, 1 - wl), and the second weights differ in the last bit where tl == 0.
struct DflTarget {
  float t;
  int tl, tr;
};

__device__ __forceinline__ DflTarget dfl_target(const AnchorAt& at, const float4 b, int side, int reg_max) {
  const float apc = (side & 1) ? at.ay : at.ax;
  const float gtc = side == 0 ? b.x : side == 1 ? b.y : side == 2 ? b.z : b.w;
  DflTarget r;
  r.t = ((side < 2) ? (apc - gtc) : (gtc - apc)) / at.st;
  r.t = fminf(fmaxf(r.t, 0.f), (float)reg_max - 1.01f);
  r.tl = min(max((int)floorf(r.t), 0), reg_max - 1);
  r.tr = min(r.tl + 1, reg_max - 1);
  return r;
}

// d total / d (the side's reg_max logits d) -> out, added to it with `acc`: through the expectation (ddist = d total / d dist,
// d dist / d raw_j = p_j (j - dist)) plus the DFL term kd * (wl (p - onehot(tl)) + wr (p - onehot(tr))).
__device__ __forceinline__ void dfl_side_grad(const float* d, const SideDist& sd, int reg_max, float ddist, float kd, const DflTarget& tg,
                                              float wl, float wr, float* out, bool acc) {
  for (int j = 0; j < reg_max; ++j) {
    const float pj = expf(d[j] - sd.m) / sd.s;
    float gv = ddist * pj * ((float)j - sd.dist) + kd * (wl + wr) * pj;
    if (j == tg.tl) gv -= kd * wl;
    if (j == tg.tr) gv -= kd * wr;
    out[j] = acc ? out[j] + gv : gv;
  }
}

// ---- IoU match of the reference loss: det_loss_kernel, det_loss_grad_kernel, det_confusion_kernel and ml_match_kernel ----
// 4 lanes per (image, anchor) g, one per box side: walk, side decode, box, IoU against the image's GT boxes (:316, first maximum wins
// like torch.max), positive = max IoU > iou_thresh (:319-321).  Every lane of a wave must call it (decode_box); lanes of an anchor
// beyond N * A come back with live = pos = false.
struct AnchorMatch {
  AnchorAt at;
  const float* row;     // the anchor's map row: 4 * reg_max distribution logits, then nc class logits
  const float* d;       // this lane's side: row + side * reg_max
  SideDist sd;
  float4 box;           // decoded box
  int bi;               // matched GT row (-1 if the image has none)
  float best;           // max IoU
  bool live, pos;
};

__device__ __forceinline__ AnchorMatch match_anchor(const LossP& p, long g, int side) {
  AnchorMatch r;
  r.live = g < (long)p.N * p.A;
  r.at = anchor_at(p, r.live ? g : 0);
  r.row = anchor_row(p, r.at);
  r.d = r.row + side * p.reg_max;
  r.sd = side_dist(r.d, p.reg_max);
  r.box = decode_box(r.at, r.sd.dist);
  // match against this image's GT boxes (every lane of the group computes the same thing)
  const int g0 = p.gt_off[r.at.n], g1 = p.gt_off[r.at.n + 1];
  r.best = -INFINITY;
  r.bi = -1;
  for (int k = g0; k < g1; ++k) {
    const float4 b = ld4(p.gt_xyxy + 4 * k);
    const float v = iou_xyxy(r.box.x, r.box.y, r.box.z, r.box.w, b.x, b.y, b.z, b.w);
    if (v > r.best) { r.best = v; r.bi = k; }
  }
  r.pos = r.live && r.bi >= 0 && r.best > p.iou_thresh;
  return r;
}

// ---- host: the level table of LossP from an argument block (mtbt_loss_args, mtbt_tal_loss_args and mtbt_mask_loss_args share the
// fields map / h / w / map_pixel_stride / n_levels / img_size) ----
// Fills p.map / h / w / ld / off / stride / n_levels / A (unused levels: null maps, 1 x 1) and, with `g`, the gradient maps from d_map /
// d_ld.  min_ld = the narrowest pixel stride the caller's kernels can read (and write); 0 = the maps are not read: their pointers may
// be null and are not passed on.  A is summed in 64 bits.  MTBT_EINVAL for n_levels outside [1, 3], a level without pixels, a missing
// or too narrow map (or gradient map), or more than INT_MAX anchors.
template <typename Args>
inline int fill_levels(const Args* a, int min_ld, LossP& p, GradMaps* g = nullptr, float* const* d_map = nullptr, const int32_t* d_ld = nullptr) {
  if (a->n_levels < 1 || a->n_levels > 3) return MTBT_EINVAL;
  long A = 0;
  for (int l = 0; l < 3; ++l) {
    p.off[l] = (int)A;
    p.map[l] = nullptr; p.h[l] = p.w[l] = 1; p.ld[l] = 0; p.stride[l] = 0.f;
    if (g) { g->map[l] = nullptr; g->ld[l] = 0; }
    if (l >= a->n_levels) continue;
    if (a->h[l] <= 0 || a->w[l] <= 0) return MTBT_EINVAL;
    if (min_ld > 0 && (!a->map[l] || a->map_pixel_stride[l] < min_ld)) return MTBT_EINVAL;
    if (g && (!d_map[l] || d_ld[l] < min_ld)) return MTBT_EINVAL;
    p.map[l] = min_ld > 0 ? a->map[l] : nullptr; p.h[l] = a->h[l]; p.w[l] = a->w[l]; p.ld[l] = a->map_pixel_stride[l];
    p.stride[l] = a->img_size / (float)a->w[l];                         // running_main_v3.py:266
    if (g) { g->map[l] = d_map[l]; g->ld[l] = d_ld[l]; }
    A += (long)a->h[l] * a->w[l];
    if (A > INT_MAX) return MTBT_EINVAL;
  }
  p.off[3] = (int)A;
  p.n_levels = a->n_levels; p.A = (int)A;
  return MTBT_OK;
}

}  // namespace
