// What the greedy box kernels share (postprocess.hip: nms_kernel; box_fuse.hip: fuse_kernel; tile_merge.hip: merge_kernel): the score
// order key, the workgroup bitonic sort, torchvision's box overlap, the candidate front end of the fusion and merge kernels and their
// output row.  The three greedy passes themselves are three different algorithms and stay in their files.
//
// Only correct in a translation unit built with -ffp-contract=off (build.py's EXTRA_FLAGS lists every includer): the overlap must round
// like the CPU references, which evaluate every product and sum separately.  hipcc's default contracts in the backend, and the
// __fmul_rn / __fadd_rn spellings are plain operators.
//
// Not here, on purpose: bbox_iou_kernel's IoU (postprocess.hip; its eps makes it different arithmetic) and coco_eval.h's score_key (a
// different order: NaN last, -0 equal to +0, larger key first).
#pragma once
#include "common.h"

namespace {

// ---- the order: ascending keys == descending score, ascending index on ties (torch's stable descending sort) ----
__device__ __forceinline__ unsigned orderable(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

constexpr unsigned long long KEY_NONE = ~0ull;   // a dropped or padded slot: sorts behind every real key

__device__ __forceinline__ unsigned long long order_key(float score, int index) {
  return ((unsigned long long)(~orderable(score)) << 32) | (unsigned)index;
}
__device__ __forceinline__ int key_index(unsigned long long key) { return (int)(key & 0xffffffffu); }

// ascending bitonic sort of keys[0, P) (LDS or global memory), P a power of two, by a whole workgroup of NT threads; ends on a barrier
template <int NT>
__device__ __forceinline__ void bitonic_sort(unsigned long long* keys, int P, int tid) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += NT) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int hi = lo | j;
        const bool up = (lo & k) == 0;
        const unsigned long long x = keys[lo], y = keys[hi];
        if ((x > y) == up) { keys[lo] = y; keys[hi] = x; }
      }
      __syncthreads();
    }
  }
}

// the sort's length for v keys: the least power of two >= v and >= floor (itself a power of two)
__host__ __device__ inline int pow2ceil(int v, int floor = 1) { int p = floor; while (p < v) p <<= 1; return p; }

// ---- the overlap: torchvision nms_kernel.cpp's arithmetic up to the intersection, then IoU (MTBT_MERGE_IOU) or intersection over the
//      smaller area (MTBT_MERGE_IOS).  bi = the EARLIER box (kept box, cluster's fused box, row leader), bj = the candidate ----
__device__ __forceinline__ float overlap(const float4 bi, const float4 bj, int metric = MTBT_MERGE_IOU) {
  const float iarea = __fmul_rn(__fsub_rn(bi.z, bi.x), __fsub_rn(bi.w, bi.y));
  const float jarea = __fmul_rn(__fsub_rn(bj.z, bj.x), __fsub_rn(bj.w, bj.y));
  const float xx1 = fmaxf(bi.x, bj.x), yy1 = fmaxf(bi.y, bj.y);
  const float xx2 = fminf(bi.z, bj.z), yy2 = fminf(bi.w, bj.w);
  const float w = fmaxf(0.f, __fsub_rn(xx2, xx1)), h = fmaxf(0.f, __fsub_rn(yy2, yy1));
  const float inter = __fmul_rn(w, h);
  const float den = metric == MTBT_MERGE_IOS ? fminf(iarea, jarea) : __fsub_rn(__fadd_rn(iarea, jarea), inter);
  return __fdiv_rn(inter, den);
}

// ---- the candidate front end of fuse_kernel and merge_kernel: keys of slots [0, P2), KEY_NONE for a slot that is padding (c >= C), not
//      listed, or scored at or below skip_thr; the sort puts the nc candidates first.  slot(c, listed) calls listed(score) if slot c is
//      in its list.  The caller zeroed s_cnt behind a barrier.  Returns nc ----
template <int NT, typename Slot>
__device__ __forceinline__ int sorted_candidates(unsigned long long* keys, int P2, int C, float skip_thr, int& s_cnt, int tid, Slot slot) {
  int mine = 0;
  for (int c = tid; c < P2; c += NT) {
    unsigned long long key = KEY_NONE;
    if (c < C)
      slot(c, [&](float s) {
        if (s > skip_thr) { key = order_key(s, c); ++mine; }
      });
    keys[c] = key;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if ((tid & 63) == 0 && mine) atomicAdd(&s_cnt, mine);
  __syncthreads();
  const int nc = s_cnt;
  bitonic_sort<NT>(keys, P2, tid);
  return nc;
}

// ---- one output row of the fusion and merge kernels; a default Row is the padded row behind the last real one ----
struct RowOut {
  float* boxes;
  float* scores;
  long long* labels;
  int* n_members;
  int* lead_source;   // the leader's source list (fusion) or tile (merging)
  int* lead_slot;
  int* lead_anchor;   // or nullptr
};
struct Row {
  float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
  float score = 0.f;
  long long label = -1;
  int members = 0, lead_source = -1, lead_slot = -1, lead_anchor = -1;
};
__device__ __forceinline__ void store_row(const RowOut& o, long at, const Row& r) {
  reinterpret_cast<float4*>(o.boxes)[at] = r.box;
  o.scores[at] = r.score;
  o.labels[at] = r.label;
  o.n_members[at] = r.members;
  o.lead_source[at] = r.lead_source;
  o.lead_slot[at] = r.lead_slot;
  if (o.lead_anchor) o.lead_anchor[at] = r.lead_anchor;
}

}  // namespace
