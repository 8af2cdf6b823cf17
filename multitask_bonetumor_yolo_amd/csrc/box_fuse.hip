// Weighted box fusion of several detection lists of the same images (test-time augmentation views, model ensembles):
// mtbt_fuse_detections.  The arithmetic is the project's own definition (include/mtbt_hip.h; tests/fuse_reference.py restates it in
// numpy) and the results are bit-exact restatements of it: no FMA contraction, IEEE division, stable ordering, no floating-point atomics.
#include "common.h"
#include "det_order.h"

// No FMA contraction in this file (built with -ffp-contract=off, see build.py and det_order.h).

namespace {

constexpr int FUSE_NT = 256;               // one workgroup per image
constexpr int FUSE_LDS_BUDGET = 144 * 1024; // dynamic LDS this kernel ever asks for (160 KiB per CU less the static part)

struct FuseP {
  const float* boxes[MTBT_FUSE_MAX_SOURCES];
  const float* scores[MTBT_FUSE_MAX_SOURCES];
  const long long* labels[MTBT_FUSE_MAX_SOURCES];
  const int* counts[MTBT_FUSE_MAX_SOURCES];
  const int* anchors[MTBT_FUSE_MAX_SOURCES];
  float weight[MTBT_FUSE_MAX_SOURCES];
  int orient[MTBT_FUSE_MAX_SOURCES];
  int M, K, top_k, C, P2, acc_in_lds;
  float S, iou_thr, skip_thr, wsum;
  RowOut out;
  int* out_counts;
  int* n_clusters;
  int* member_slot;   // [N, C] or nullptr: the cluster index during the greedy pass, the output row after the write-out
  char* ws;
  long ws_per_image;
};

// running sums of one cluster: touched by lane 0 of wave 0 only while the greedy pass runs
struct Acc {
  float ss, x1, y1, x2, y2;
  int n, lead, pad;
};

__device__ __forceinline__ float cluster_score(const Acc& a, int M, float wsum) {
  return __fdiv_rn(__fmul_rn(__fdiv_rn(a.ss, (float)a.n), (float)min(a.n, M)), wsum);
}

// One 256-thread workgroup per image.
//  1. candidates: det_order.h's key of (s, c) for every kept (m, k), c = m K + k; its sort == stable descending s, ascending c
//  2. the sorted candidates (un-oriented box, s, label, c) go to the workspace
//  3. greedy clustering by wave 0: 64 sorted candidates per step live in registers (lane = candidate) and are broadcast one at a time;
//     each lane scans clusters lane, lane + 64, ... in LDS, a butterfly (value, index) arg-max picks the winner, lane 0 applies the update.
//     No workgroup barrier inside the loop: LDS operations of one wave complete in order, the fence keeps the compiler from moving them.
//  4. cluster scores -> keys, bitonic sort, write-out by the whole workgroup
// With member_slot (mtbt_fuse_detections_members) every candidate's cluster index is kept by the greedy pass and turned into its output
// row at the end; nothing else changes.
__global__ __launch_bounds__(FUSE_NT) void fuse_kernel(const FuseP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int s_cnt, s_ncl;
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = p.C, K = p.K, M = p.M;
  // LDS: fused boxes [C] | cluster labels [C] | keys [P2] | (running sums [C])
  float4* fused = reinterpret_cast<float4*>(smem);
  long long* clabel = reinterpret_cast<long long*>(smem + (long)C * 16);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem + (long)C * 24);
  // workspace: sorted candidate boxes [C] | labels [C] | scores [C] | indices [C] | (running sums [C])
  char* wsi = p.ws + (long)n * p.ws_per_image;
  float4* cbox = reinterpret_cast<float4*>(wsi);
  long long* clab = reinterpret_cast<long long*>(wsi + (long)C * 16);
  float* cs = reinterpret_cast<float*>(wsi + (long)C * 24);
  int* cc = reinterpret_cast<int*>(wsi + (long)C * 28);
  Acc* acc = p.acc_in_lds ? reinterpret_cast<Acc*>(smem + (long)C * 24 + (long)p.P2 * 8) : reinterpret_cast<Acc*>(wsi + (long)C * 32);

  // ---- 1. keys of the candidates ----
  if (tid == 0) { s_cnt = 0; s_ncl = 0; }
  int* mslot = p.member_slot ? p.member_slot + (long)n * C : nullptr;
  if (mslot)
    for (int c = tid; c < C; c += FUSE_NT) mslot[c] = -1;
  __syncthreads();
  const int nc = sorted_candidates<FUSE_NT>(keys, p.P2, C, p.skip_thr, s_cnt, tid, [&](int c, auto listed) {
    const int m = c / K, k = c - m * K;
    if (k < min(p.counts[m][n], K)) listed(__fmul_rn(p.scores[m][(long)n * K + k], p.weight[m]));
  });

  // ---- 2. sorted candidates, un-oriented ----
  for (int i = tid; i < nc; i += FUSE_NT) {
    const int c = key_index(keys[i]);
    const int m = c / K, k = c - m * K;
    const long at = (long)n * K + k;
    float4 b = reinterpret_cast<const float4*>(p.boxes[m])[at];
    const int o = p.orient[m];
    if (o & 1) { b.x = __fsub_rn(p.S, b.x); b.z = __fsub_rn(p.S, b.z); }
    if (o & 2) { b.y = __fsub_rn(p.S, b.y); b.w = __fsub_rn(p.S, b.w); }
    if (o & 4) { float t = b.x; b.x = b.y; b.y = t; t = b.z; b.z = b.w; b.w = t; }
    float4 r;
    r.x = fminf(b.x, b.z); r.z = fmaxf(b.x, b.z); r.y = fminf(b.y, b.w); r.w = fmaxf(b.y, b.w);
    cbox[i] = r;
    clab[i] = p.labels[m][at];
    cs[i] = __fmul_rn(p.scores[m][at], p.weight[m]);
    cc[i] = c;
  }
  __threadfence_block();
  __syncthreads();

  // ---- 3. greedy clustering, wave 0 ----
  if (wave == 0) {
    int ncl = 0;
    for (int j0 = 0; j0 < nc; j0 += 64) {
      const int j = min(j0 + lane, nc - 1);
      const float4 mb = cbox[j];
      const float ms = cs[j];
      const long long ml = clab[j];
      const int mc = cc[j];
      const int steps = min(64, nc - j0);
      for (int t = 0; t < steps; ++t) {
        float4 bj;
        bj.x = __shfl(mb.x, t, 64); bj.y = __shfl(mb.y, t, 64); bj.z = __shfl(mb.z, t, 64); bj.w = __shfl(mb.w, t, 64);
        const float s = __shfl(ms, t, 64);
        const long long lab = ((long long)__shfl((int)(ml >> 32), t, 64) << 32) | (unsigned)__shfl((int)ml, t, 64);
        const int c = __shfl(mc, t, 64);
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int k = lane; k < ncl; k += 64) {
          if (clabel[k] == lab) {
            const float ovr = overlap(fused[k], bj);
            if (ovr > best) { best = ovr; bi = k; }          // (a NaN never wins; ascending k: ties stay with the lowest index)
          }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float ob = __shfl_xor(best, o, 64);
          const int oi = __shfl_xor(bi, o, 64);
          if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        const bool join = best > p.iou_thr;                   // (uniform: every lane holds the same winner)
        if (lane == 0) {
          if (join) {
            Acc a = acc[bi];
            a.ss = __fadd_rn(a.ss, s);
            a.x1 = __fadd_rn(a.x1, __fmul_rn(s, bj.x)); a.y1 = __fadd_rn(a.y1, __fmul_rn(s, bj.y));
            a.x2 = __fadd_rn(a.x2, __fmul_rn(s, bj.z)); a.y2 = __fadd_rn(a.y2, __fmul_rn(s, bj.w));
            a.n += 1;
            acc[bi] = a;
            fused[bi] = make_float4(__fdiv_rn(a.x1, a.ss), __fdiv_rn(a.y1, a.ss), __fdiv_rn(a.x2, a.ss), __fdiv_rn(a.y2, a.ss));
          } else {
            Acc a;
            a.ss = s;
            a.x1 = __fmul_rn(s, bj.x); a.y1 = __fmul_rn(s, bj.y); a.x2 = __fmul_rn(s, bj.z); a.y2 = __fmul_rn(s, bj.w);
            a.n = 1; a.lead = c; a.pad = 0;
            acc[ncl] = a;
            fused[ncl] = bj;
            clabel[ncl] = lab;
          }
          if (mslot) mslot[c] = join ? bi : ncl;
        }
        if (!join) ++ncl;
        __threadfence_block();                                // the update is in LDS before the next candidate's scan reads it
        __builtin_amdgcn_wave_barrier();
      }
    }
    if (lane == 0) s_ncl = ncl;
  }
  __threadfence_block();
  __syncthreads();

  // ---- 4. cluster order and write-out ----
  const int ncl = s_ncl;
  const int Pc = pow2ceil(ncl);
  for (int i = tid; i < Pc; i += FUSE_NT) keys[i] = i < ncl ? order_key(cluster_score(acc[i], M, p.wsum), i) : KEY_NONE;
  __syncthreads();
  bitonic_sort<FUSE_NT>(keys, Pc, tid);
  const int top_k = p.top_k, nout = min(ncl, top_k);
  const long row = (long)n * top_k;
  for (int r = tid; r < top_k; r += FUSE_NT) {
    Row o;
    if (r < nout) {
      const int i = key_index(keys[r]);
      const Acc a = acc[i];
      o.box = fused[i];
      o.score = cluster_score(a, M, p.wsum);
      o.label = clabel[i];
      o.members = a.n;
      o.lead_source = a.lead / K;
      o.lead_slot = a.lead - o.lead_source * K;
      if (p.out.lead_anchor) o.lead_anchor = p.anchors[o.lead_source][(long)n * K + o.lead_slot];
    }
    store_row(p.out, row + r, o);
  }
  if (tid == 0) { p.out_counts[n] = nout; p.n_clusters[n] = ncl; }
  if (mslot) {
    // cluster index -> output row (-1 past the cut), through the sorted candidates' score array: the greedy pass was its last reader
    int* row_of = reinterpret_cast<int*>(cs);
    for (int r = tid; r < ncl; r += FUSE_NT) row_of[key_index(keys[r])] = r < nout ? r : -1;
    __threadfence_block();
    __syncthreads();
    for (int c = tid; c < C; c += FUSE_NT) {
      const int i = mslot[c];
      if (i >= 0) mslot[c] = row_of[i];
    }
  }
}

inline long fuse_ws_per_image(int C) { return ((long)C * 64 + 255) / 256 * 256; }

}  // namespace

extern "C" int64_t mtbt_fuse_workspace_bytes(int n_sources, int N, int K) {
  if (n_sources < 1 || n_sources > MTBT_FUSE_MAX_SOURCES || N <= 0 || K <= 0 || (long)n_sources * K > MTBT_FUSE_MAX_CANDIDATES) return 0;
  return (int64_t)N * fuse_ws_per_image(n_sources * K);
}

extern "C" int mtbt_sizeof_box_fuse_args(void) { return (int)sizeof(mtbt_box_fuse_args); }

static int fuse_launch(const mtbt_box_fuse_args* a, int32_t* member_slot, bool want_members, void* stream) {
  if (!a) return MTBT_EINVAL;
  const int M = a->n_sources;
  if (M < 1 || M > MTBT_FUSE_MAX_SOURCES || a->N < 0 || a->K < 1 || (long)M * a->K > MTBT_FUSE_MAX_CANDIDATES || a->top_k < 1) return MTBT_EINVAL;
  if (!(a->img_size > 0.f)) return MTBT_EINVAL;
  float wsum = 0.f;
  for (int m = 0; m < M; ++m) {
    if (a->orient[m] < 0 || a->orient[m] > 7 || !(a->weight[m] > 0.f)) return MTBT_EINVAL;
    wsum = m ? wsum + a->weight[m] : a->weight[m];
  }
  if (a->N == 0) return MTBT_OK;
  bool all_anchors = true;
  for (int m = 0; m < M; ++m) {
    if (!a->boxes[m] || !a->scores[m] || !a->labels[m] || !a->counts[m]) return MTBT_EINVAL;
    if (!a->anchors[m]) all_anchors = false;
  }
  if (!a->out_boxes || !a->out_scores || !a->out_labels || !a->out_counts || !a->n_clusters || !a->n_members || !a->lead_source ||
      !a->lead_slot || !a->workspace || (want_members && !member_slot))
    return MTBT_EINVAL;
  if (a->lead_anchor && !all_anchors) return MTBT_EINVAL;
  const int C = M * a->K;
  const long per = fuse_ws_per_image(C);
  if (a->workspace_bytes < (int64_t)a->N * per) return MTBT_EINVAL;
  for (int m = 0; m < M; ++m)
    if (!aligned16(a->boxes[m])) return MTBT_EALIGN;
  if (!aligned16(a->out_boxes) || !aligned16(a->workspace)) return MTBT_EALIGN;

  FuseP p;
  for (int m = 0; m < MTBT_FUSE_MAX_SOURCES; ++m) {
    const bool on = m < M;
    p.boxes[m] = on ? a->boxes[m] : nullptr;
    p.scores[m] = on ? a->scores[m] : nullptr;
    p.labels[m] = on ? reinterpret_cast<const long long*>(a->labels[m]) : nullptr;
    p.counts[m] = on ? a->counts[m] : nullptr;
    p.anchors[m] = on ? a->anchors[m] : nullptr;
    p.weight[m] = on ? a->weight[m] : 0.f;
    p.orient[m] = on ? a->orient[m] : 0;
  }
  p.M = M; p.K = a->K; p.top_k = a->top_k; p.C = C; p.P2 = pow2ceil(C);
  const long lds_small = (long)C * 24 + (long)p.P2 * 8, lds_acc = lds_small + (long)C * (long)sizeof(Acc);
  p.acc_in_lds = lds_acc <= FUSE_LDS_BUDGET ? 1 : 0;
  p.S = a->img_size; p.iou_thr = a->iou_thr; p.skip_thr = a->skip_thr; p.wsum = wsum;
  p.out = RowOut{a->out_boxes, a->out_scores, reinterpret_cast<long long*>(a->out_labels), a->n_members, a->lead_source, a->lead_slot, a->lead_anchor};
  p.out_counts = a->out_counts; p.n_clusters = a->n_clusters;
  p.member_slot = want_members ? member_slot : nullptr;
  p.ws = reinterpret_cast<char*>(a->workspace); p.ws_per_image = per;
  const size_t lds = (size_t)(p.acc_in_lds ? lds_acc : lds_small);
  // one-time (per device) opt-in to the LARGEST dynamic LDS this kernel ever asks for
  if (int rc = mtbt_allow_lds(fuse_kernel, FUSE_LDS_BUDGET)) return rc;
  hipLaunchKernelGGL(fuse_kernel, dim3(a->N), dim3(FUSE_NT), lds, reinterpret_cast<hipStream_t>(stream), p);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}

extern "C" int mtbt_fuse_detections(const mtbt_box_fuse_args* a, void* stream) { return fuse_launch(a, nullptr, false, stream); }

extern "C" int mtbt_fuse_detections_members(const mtbt_box_fuse_args* a, int32_t* member_slot, void* stream) {
  return fuse_launch(a, member_slot, true, stream);
}
