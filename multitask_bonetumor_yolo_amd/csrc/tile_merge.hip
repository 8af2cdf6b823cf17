// Merging the per-tile detection lists of sliced inference in the image's own pixel frame: mtbt_merge_tiles.  The arithmetic is the
// project's own definition (include/mtbt_hip.h; tests/slice_reference.py restates it) and the results are bit-exact restatements of it: no
// FMA contraction, IEEE division, stable ordering, no floating-point atomics.
#include "common.h"
#include "det_order.h"
#include "tile_check.h"

// No FMA contraction in this file (built with -ffp-contract=off, see build.py and det_order.h).

namespace {

constexpr int MERGE_NT = 256;    // one workgroup per image
constexpr int FREE = -1;         // state of a candidate that neither leads nor is absorbed

struct MergeP {
  const float* boxes;
  const float* scores;
  const long long* labels;
  const int* counts;
  const int* anchors;
  const mtbt_tile* tiles;
  int n_tiles, K, top_k, metric, class_agnostic;
  float thr, skip_thr;
  RowOut out;         // lead_source = the leader's tile
  int* out_counts;
  int* member_slot;
  int* n_left;
};

// clamp((v + off) / scale, 0, hi): frame_tile.h's frame_box with the tile's offset added first
__device__ __forceinline__ float to_frame(float v, float off, float scale, float hi) {
  return fminf(fmaxf(__fdiv_rn(__fadd_rn(v, off), scale), 0.f), hi);
}

// One 256-thread workgroup per image.
//  1. the image's tiles are found in the tile table (they are consecutive); member_slot of all their slots starts at -1
//  2. det_order.h's keys of the candidates and its sort == stable descending s, ascending c; the sorted candidates' frame boxes and labels go to LDS
//  3. the greedy pass walks the sorted candidates: one that is still free opens a row and every thread tests its share of the later free
//     candidates against the LEADER's own box (one barrier per row, none for an absorbed candidate)
//  4. per row a wave reduces the union box and the member count (min / max are exact, any order), then the write-out
// LDS: keys [P2] | boxes [C] | labels [C] | state [C], C = Cmax = the largest T_n K of the launch.
__global__ __launch_bounds__(MERGE_NT) void merge_kernel(const MergeP p, int Cmax, int P2max) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int s_t0, s_t1, s_cnt, s_left;
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);
  float4* cbox = reinterpret_cast<float4*>(smem + (long)P2max * 8);
  long long* clab = reinterpret_cast<long long*>(smem + (long)P2max * 8 + (long)Cmax * 16);
  int* state = reinterpret_cast<int*>(smem + (long)P2max * 8 + (long)Cmax * 24);
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = p.K, top_k = p.top_k;

  // ---- 1. the image's tiles ----
  if (tid == 0) { s_t0 = p.n_tiles; s_t1 = 0; s_cnt = 0; s_left = 0; }
  __syncthreads();
  for (int t = tid; t < p.n_tiles; t += MERGE_NT)
    if (p.tiles[t].image == n) { atomicMin(&s_t0, t); atomicMax(&s_t1, t + 1); }
  __syncthreads();
  const int t0 = min(s_t0, s_t1), T = min(s_t1 - t0, Cmax / K);   // (the host checked T K <= Cmax; the min keeps a table that differs from the host's in bounds)
  const int C = T * K;
  int* mslot = p.member_slot + (long)t0 * K;

  // ---- 2. keys, order, frame boxes ----
  const int nc = sorted_candidates<MERGE_NT>(keys, pow2ceil(C), C, p.skip_thr, s_cnt, tid, [&](int c, auto listed) {
    const int t = t0 + c / K, k = c - (c / K) * K;
    if (k < min(p.counts[t], K)) listed(p.scores[(long)t * K + k]);
  });
  for (int i = tid; i < nc; i += MERGE_NT) {
    const int c = key_index(keys[i]);
    const int t = t0 + c / K, k = c - (c / K) * K;
    const mtbt_tile& d = p.tiles[t];
    const float4 b = reinterpret_cast<const float4*>(p.boxes)[(long)t * K + k];
    const float wf = (float)d.width, hf = (float)d.height;
    cbox[i] = make_float4(to_frame(b.x, d.fox, d.scale, wf), to_frame(b.y, d.foy, d.scale, hf), to_frame(b.z, d.fox, d.scale, wf),
                          to_frame(b.w, d.foy, d.scale, hf));
    clab[i] = p.labels[(long)t * K + k];
    state[i] = FREE;
  }
  __syncthreads();

  // ---- 3. greedy merging ----
  int rows = 0;
  for (int i = 0; i < nc && rows < top_k; ++i) {
    if (state[i] != FREE) continue;           // workgroup-uniform: nothing was written since the last barrier
    const float4 bi = cbox[i];
    const long long li = clab[i];
    __syncthreads();                          // every thread has read state[i] before thread 0 rewrites it
    if (tid == 0) state[i] = rows;
    for (int j = i + 1 + tid; j < nc; j += MERGE_NT)
      if (state[j] == FREE && (p.class_agnostic || clab[j] == li) && overlap(bi, cbox[j], p.metric) > p.thr) state[j] = rows;   // (a NaN never matches)
    ++rows;
    __syncthreads();
  }

  // ---- 4. rows and write-out ----
  const long row0 = (long)n * top_k;
  for (int r = wave; r < top_k; r += MERGE_NT / 64) {
    float4 u = make_float4(INFINITY, INFINITY, -INFINITY, -INFINITY);
    int nm = 0, lead = 0x7fffffff;
    if (r < rows)
      for (int j = lane; j < nc; j += 64)
        if (state[j] == r) {
          const float4 b = cbox[j];
          u.x = fminf(u.x, b.x); u.y = fminf(u.y, b.y); u.z = fmaxf(u.z, b.z); u.w = fmaxf(u.w, b.w);
          ++nm;
          lead = min(lead, j);
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      u.x = fminf(u.x, __shfl_xor(u.x, o, 64)); u.y = fminf(u.y, __shfl_xor(u.y, o, 64));
      u.z = fmaxf(u.z, __shfl_xor(u.z, o, 64)); u.w = fmaxf(u.w, __shfl_xor(u.w, o, 64));
      nm += __shfl_xor(nm, o, 64);
      lead = min(lead, __shfl_xor(lead, o, 64));
    }
    if (lane == 0) {
      Row o;
      if (r < rows) {
        const int c = key_index(keys[lead]);   // the leader is the row's first candidate in the order
        o.box = u;
        o.members = nm;
        o.lead_source = t0 + c / K;
        o.lead_slot = c - (c / K) * K;
        const long at = (long)o.lead_source * K + o.lead_slot;
        o.score = p.scores[at];
        o.label = clab[lead];
        if (p.out.lead_anchor) o.lead_anchor = p.anchors[at];
      }
      store_row(p.out, row0 + r, o);
    }
  }
  // membership: every slot of the image's tiles is written once.  keys is free after the leaders were looked up
  __syncthreads();
  int* row_of = reinterpret_cast<int*>(cbox);   // the boxes' space is free now and holds 4 Cmax ints
  for (int c = tid; c < C; c += MERGE_NT) row_of[c] = -1;
  __syncthreads();
  int left = 0;
  for (int i = tid; i < nc; i += MERGE_NT) {
    row_of[key_index(keys[i])] = state[i];
    left += state[i] == FREE;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) left += __shfl_xor(left, o, 64);
  if (lane == 0 && left) atomicAdd(&s_left, left);
  __syncthreads();
  for (int c = tid; c < C; c += MERGE_NT) mslot[c] = row_of[c];
  if (tid == 0) { p.out_counts[n] = rows; p.n_left[n] = s_left; }
}

}  // namespace

extern "C" int mtbt_merge_tiles(const mtbt_tile_merge_args* a, void* stream) {
  if (!a) return MTBT_EINVAL;
  if (a->N < 0 || a->K < 1 || a->top_k < 1 || a->metric < MTBT_MERGE_IOU || a->metric > MTBT_MERGE_IOS) return MTBT_EINVAL;
  if (a->thr != a->thr || a->skip_thr != a->skip_thr) return MTBT_EINVAL;
  if (a->N == 0) return MTBT_OK;
  if (!a->boxes || !a->scores || !a->labels || !a->counts || !a->tiles || !a->tiles_dev || !a->first) return MTBT_EINVAL;
  if (!a->out_boxes || !a->out_scores || !a->out_labels || !a->out_counts || !a->n_members || !a->lead_tile || !a->lead_slot ||
      !a->member_slot || !a->n_left)
    return MTBT_EINVAL;
  if (a->lead_anchor && !a->anchors) return MTBT_EINVAL;
  if (a->first[0] != 0) return MTBT_EINVAL;
  int Tbig = 0;
  if (int rc = tile_check::check_table(a->tiles, a->first, a->N, a->n_tiles, a->K, MTBT_TILE_MAX_PER_IMAGE, true, nullptr, Tbig)) return rc;
  if (a->first[a->N] != a->n_tiles) return MTBT_EINVAL;
  if (!aligned16(a->boxes) || !aligned16(a->out_boxes)) return MTBT_EALIGN;

  MergeP p;
  p.boxes = a->boxes; p.scores = a->scores; p.labels = reinterpret_cast<const long long*>(a->labels); p.counts = a->counts;
  p.anchors = a->anchors; p.tiles = a->tiles_dev;
  p.n_tiles = a->n_tiles; p.K = a->K; p.top_k = a->top_k; p.metric = a->metric; p.class_agnostic = a->class_agnostic ? 1 : 0;
  p.thr = a->thr; p.skip_thr = a->skip_thr;
  p.out = RowOut{a->out_boxes, a->out_scores, reinterpret_cast<long long*>(a->out_labels), a->n_members, a->lead_tile, a->lead_slot, a->lead_anchor};
  p.out_counts = a->out_counts; p.member_slot = a->member_slot; p.n_left = a->n_left;
  const int Cmax = (Tbig > 0 ? Tbig : 1) * a->K, P2max = pow2ceil(Cmax, 2);   // (>= 2: the boxes behind the keys stay 16-byte aligned)
  const size_t lds = (size_t)P2max * 8 + (size_t)Cmax * 28;
  if (int rc = mtbt_allow_lds(merge_kernel, (int)((size_t)MTBT_FUSE_MAX_CANDIDATES * 36))) return rc;
  hipLaunchKernelGGL(merge_kernel, dim3(a->N), dim3(MERGE_NT), lds, reinterpret_cast<hipStream_t>(stream), p, Cmax, P2max);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}
