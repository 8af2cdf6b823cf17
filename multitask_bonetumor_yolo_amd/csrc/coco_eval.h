// What the two COCO matching kernels share (box_eval.hip: IoU from box coordinates; mask_eval.hip: IoU from pixel counts): the caps,
// the area ranges, the score order key and the wave argmax of the walk.
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

// descending score as an ascending-comparable int: larger key = earlier; -0 == +0 (numpy compares them equal); NaN last
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

}  // namespace
