// COCO matching for box_eval.hip (IoU from box coordinates) and mask_eval.hip (IoU from pixel counts), and for nobody else: the caps,
// the area ranges, the score order key, the wave argmax and the matching kernel itself, templated on what a pair is.
#pragma once
#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int CAP = 1024;   // detections (K) and GT boxes per image
constexpr int NT = 1024;    // threads per workgroup
constexpr int NW = NT / 64;
constexpr int NA = 4;       // COCO area ranges

__device__ __forceinline__ bool in_area(double area, int a) {
  const double lo = a == 2 ? 1024.0 : (a == 3 ? 9216.0 : 0.0);
  const double hi = a == 1 ? 1024.0 : (a == 2 ? 9216.0 : 1e10);
  return !(area < lo || area > hi);
}

// descending score as an ascending-comparable int: larger key = earlier; -0 == +0 (numpy compares them equal); NaN last.
// Not det_order.h's order_key (torch's stable descending sort: smaller key = earlier, -0 below +0): two orders, kept apart.
__device__ __forceinline__ int score_key(float s) {
  if (s != s) return INT_MIN;
  if (s == 0.f) s = 0.f;
  const int k = __float_as_int(s);
  return k < 0 ? k ^ 0x7fffffff : k;
}

// wave argmax of (v, j), j < 0 = no candidate; equal values -> higher j.  A detection has few candidate GT boxes (IoU >= lim,
// its class, still free): a loop over the ballot of candidate lanes with uniform readlanes (usually 0 - 2 trips) instead of a
// 6-step shuffle butterfly of doubles (155 -> 81 us per 16-image batch at K = 100, T = 10: tools/box_eval_probe.py)
__device__ __forceinline__ void wave_argmax(double& v, int& j) {
  unsigned long long live = __ballot(j >= 0);
  double bv = -INFINITY;
  int bj = -1;
  while (live) {
    const int l = __builtin_ctzll(live);
    live &= live - 1ull;
    const long long bits = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)bits, l), hi = __builtin_amdgcn_readlane((int)(bits >> 32), l);
    const double ov = __hiloint2double(hi, lo);
    const int oj = __builtin_amdgcn_readlane(j, l);
    if (ov > bv || (ov == bv && oj > bj)) { bv = ov; bj = oj; }
  }
  v = bv;
  j = bj;
}

// The matching kernel (semantics at the top of box_eval.hip), once for both kinds of pair.  A pair policy `Pairs` never asks which
// kernel it is in; it supplies
//   Args                      the entry point's argument struct (the walk reads B, K, M, T, max_det, counts, scores, labels,
//                             iou_thresholds and writes rank, match, ignore, gt_area, status)
//   Lds                       its per-image payload in LDS, and Pairs{p, lds} holds references to both
//   gt_in_batch(g, area)      GT row g belongs to an image of the batch; its area
//   load_det(i, at)           detection slot i of the image, `at` its index in the batch
//   gt_of(g, b)               GT row g belongs to image b
//   load_gt(g, pos, cls)      GT row g into slot pos: its class in cls, its area returned
//   iou(i, j), det_area(i)    of detection slot i and GT slot j, in fp64
template <typename Pairs>
__global__ __launch_bounds__(NT) void coco_match_kernel(const typename Pairs::Args p) {
  __shared__ typename Pairs::Lds payload;
  __shared__ int dkey[CAP], dlab[CAP], order[CAP];
  __shared__ unsigned mword[CAP], iword[CAP];
  __shared__ int gcls[CAP], gign[CAP];
  __shared__ int wcnt[NW];
  Pairs pairs{p, payload};

  const int b = blockIdx.x, a = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K, M = p.M;

  // every GT row's area-range set, each row written by exactly one workgroup of the grid
  for (long g = (long)(b * NA + a) * NT + tid; g < M; g += (long)p.B * NA * NT) {
    unsigned bits = 0;
    double area;
    if (pairs.gt_in_batch(g, area)) {
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
    pairs.load_det(tid, row + tid);
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
    const bool mine = g < M && pairs.gt_of(g, b);
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
      int cls;
      const double area = pairs.load_gt(g, pos, cls);
      gcls[pos] = cls;
      gign[pos] = in_area(area, a) ? 0 : 1;
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
    unsigned used = 0u;   // bit c: GT slot c * 64 + lane is matched
    for (int q = 0; q < n; ++q) {
      const int i = order[q];
      if (i < 0) continue;
      const int lab = dlab[i];
      double vn = -INFINITY, vi = -INFINITY;
      int jn = -1, ji = -1;
      for (int c = 0; c < nchunk; ++c) {
        const int j = (c << 6) + lane;
        if (j < ng && gcls[j] == lab && !((used >> c) & 1u)) {
          const double v = pairs.iou(i, j);
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
        if (m >= 0 ? jn < 0 : !in_area(pairs.det_area(i), a)) atomicOr(&iword[i], 1u << t);
      }
    }
  }
  __syncthreads();
  if (tid < K) {
    p.match[(row + tid) * NA + a] = tid < n ? mword[tid] : 0u;
    p.ignore[(row + tid) * NA + a] = tid < n ? iword[tid] : 0u;
  }
}

}  // namespace
