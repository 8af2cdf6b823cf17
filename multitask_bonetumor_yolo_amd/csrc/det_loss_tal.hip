// Task-aligned detection loss (TaskAlignedAssigner + CIoU + DFL + BCE over all anchors) and its gradient with respect to the raw
// Detect maps.  Definition: include/mtbt_hip.h (mtbt_tal_loss_args).  Anchor walk, side decode, DFL target and gradient, bce_logits and the
// host's level table: loss_match.h, shared with the reference loss.
//
//   tal_decode_kernel    4 lanes per (image, anchor), one per box side: (max, sum-exp, expectation) of the side's distribution and the
//                        decoded box -> workspace
//   tal_topk_kernel      one workgroup per GT row g, streaming its image's A anchors: thread t computes ov / metric of anchors
//                        t, t + 256, ... and keeps them in the workspace (met / ovl [G][A]; in the rounds a thread re-reads only the
//                        metrics it wrote; thread 0 reads the winner's ovl entry behind the round's __syncthreads);
//                        then `topk` rounds of a workgroup arg-max on (metric, -index) below the previous winner's key, so ties go to
//                        the lower index exactly like a stable descending sort.  Works for any A (A < topk leaves empty slots).
//   tal_resolve_kernel   one thread per (image, anchor): scans the image's G_n * topk selections, largest ov wins (first maximum in
//                        row order) -> assigned
//   tal_gtmax_kernel     one thread per GT row: M_g, O_g over its final fg anchors (at most topk of them)
//   tal_value_kernel     4 lanes per anchor: target score, BCE over all classes, (1 - CIoU) t, DFL; workgroup partials
//   tal_finalize_kernel  one workgroup, fixed order: T and out[8]
//   tal_grad_kernel      same mapping as the value kernel; writes (or adds to) every map row whole
// Deterministic: every sum has a fixed order, the only maxima are over values compared in a fixed order.  Built with -ffp-contract=off.
#include <climits>
#include <cmath>

#include "common.h"
#include "loss_match.h"

namespace {

constexpr int TAL_MAX_TOPK = 64;
constexpr float TAL_EPS = 1e-7f;

struct TalP {
  LossP l;
  int G, topk;
  float alpha, beta, w_box, w_dfl, w_cls;
  float* boxes;      // [N * A][4]
  float* stat;       // [N * A * 4][4]: max logit, sum of exp(logit - max), expectation, 0
  float* met;        // [G][A]
  float* ovl;        // [G][A]: ov where inside, -1 where not
  int* sel;          // [G][topk]: selected anchor or -1
  int* img;          // [G]: image of the row or -1
  float* gmax;       // [G][2]: M_g, O_g
  int* assigned;     // [N * A]
  float* tscore;     // [N * A]
  float* partial;    // [blocks][6]: sum t, box, dfl, cls, #fg, sum ov
  GradMaps d;
  int accumulate;
  float* out;
};

__device__ __forceinline__ bool inside_box(float ax, float ay, const float4 g) {
  return fminf(fminf(ax - g.x, ay - g.y), fminf(g.z - ax, g.w - ay)) > 1e-9f;
}

// the pieces of ciou(p, g) that both the value and the gradient need
struct CiouQ {
  float wp, hp, iwr, ihr, iw, ih, inter, uni, iou, cw, ch, c2, dx, dy, rho2, atd, v, alpha, val;
};

__device__ __forceinline__ CiouQ ciou_q(const float4 p, const float4 g) {
  CiouQ q;
  q.wp = p.z - p.x; q.hp = p.w - p.y + TAL_EPS;
  const float wg = g.z - g.x, hg = g.w - g.y + TAL_EPS;
  q.iwr = fminf(p.z, g.z) - fmaxf(p.x, g.x); q.ihr = fminf(p.w, g.w) - fmaxf(p.y, g.y);
  q.iw = fmaxf(q.iwr, 0.f); q.ih = fmaxf(q.ihr, 0.f);
  q.inter = q.iw * q.ih;
  q.uni = q.wp * q.hp + wg * hg - q.inter + TAL_EPS;
  q.iou = q.inter / q.uni;
  q.cw = fmaxf(p.z, g.z) - fminf(p.x, g.x); q.ch = fmaxf(p.w, g.w) - fminf(p.y, g.y);
  q.c2 = q.cw * q.cw + q.ch * q.ch + TAL_EPS;
  q.dx = g.x + g.z - p.x - p.z; q.dy = g.y + g.w - p.y - p.w;
  q.rho2 = (q.dx * q.dx + q.dy * q.dy) / 4.f;
  q.atd = atanf(wg / hg) - atanf(q.wp / q.hp);
  q.v = 0.40528473456935109f * (q.atd * q.atd);                    // 4 / pi^2
  q.alpha = q.v / (q.v - q.iou + (1.f + TAL_EPS));
  q.val = q.iou - (q.rho2 / q.c2 + q.v * q.alpha);
  return q;
}

// d ciou / d (the corner of p owned by `side`: x1, y1, x2, y2), alpha constant
__device__ __forceinline__ float ciou_dcorner(const CiouQ& q, const float4 p, const float4 g, int side) {
  const float k2 = 2.f * 0.40528473456935109f * q.atd / (q.wp * q.wp + q.hp * q.hp);
  const float dv_dwp = -k2 * q.hp, dv_dhp = k2 * q.wp;
  float dinter, darea, drho2, dc2, dv;
  if (side == 0)      { dinter = (q.iwr > 0.f && p.x > g.x) ? -q.ih : 0.f; darea = -q.hp; drho2 = -q.dx / 2.f; dc2 = p.x < g.x ? -2.f * q.cw : 0.f; dv = -dv_dwp; }
  else if (side == 1) { dinter = (q.ihr > 0.f && p.y > g.y) ? -q.iw : 0.f; darea = -q.wp; drho2 = -q.dy / 2.f; dc2 = p.y < g.y ? -2.f * q.ch : 0.f; dv = -dv_dhp; }
  else if (side == 2) { dinter = (q.iwr > 0.f && p.z < g.z) ? q.ih : 0.f;  darea = q.hp;  drho2 = -q.dx / 2.f; dc2 = p.z > g.z ? 2.f * q.cw : 0.f;  dv = dv_dwp; }
  else                { dinter = (q.ihr > 0.f && p.w < g.w) ? q.iw : 0.f;  darea = q.wp;  drho2 = -q.dy / 2.f; dc2 = p.w > g.w ? 2.f * q.ch : 0.f;  dv = dv_dhp; }
  const float diou = (dinter * q.uni - q.inter * (darea - dinter)) / (q.uni * q.uni);
  const float dpen = (drho2 * q.c2 - q.rho2 * dc2) / (q.c2 * q.c2);
  return diou - dpen - q.alpha * dv;
}

__global__ __launch_bounds__(256) void tal_decode_kernel(const TalP q) {
  const LossP& p = q.l;
  const long i = (long)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int side = threadIdx.x & 3;
  const bool live = i < (long)p.N * p.A;
  const AnchorAt at = anchor_at(p, live ? i : 0);                 // every lane takes part in decode_box's exchange
  const SideDist sd = side_dist(anchor_row(p, at) + side * p.reg_max, p.reg_max);
  const float4 box = decode_box(at, sd.dist);
  if (!live) return;
  *reinterpret_cast<f32x4*>(q.stat + (i * 4 + side) * 4) = f32x4{sd.m, sd.s, sd.dist, 0.f};
  if (side == 0) *reinterpret_cast<f32x4*>(q.boxes + i * 4) = f32x4{box.x, box.y, box.z, box.w};
}

__global__ __launch_bounds__(256) void tal_topk_kernel(const TalP q) {
  __shared__ int s_n;
  __shared__ float s_m[4];
  __shared__ int s_i[4];
  const LossP& p = q.l;
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = p.A;
  if (tid == 0) s_n = -1;
  __syncthreads();
  for (int n = tid; n < p.N; n += 256)
    if (p.gt_off[n] <= g && g < p.gt_off[n + 1]) s_n = n;        // at most one n
  __syncthreads();
  const int n = s_n;
  int* sel = q.sel + (long)g * q.topk;
  if (tid == 0) q.img[g] = n;
  if (n < 0) {                                                    // a row of no image
    for (int r = tid; r < q.topk; r += 256) sel[r] = -1;
    return;
  }
  const float4 b = ld4(p.gt_xyxy + 4 * (long)g);
  const int gc = p.gt_cls[g];
  const bool cok = gc >= 0 && gc < p.nc;
  float* met = q.met + (long)g * A;
  float* ovl = q.ovl + (long)g * A;
  for (int a = tid; a < A; a += 256) {
    const AnchorAt at = anchor_at(p, n, a);
    float ov = -1.f, m = 0.f;
    if (inside_box(at.ax, at.ay, b)) {
      const float4 pb = ld4(q.boxes + ((long)n * A + a) * 4);
      ov = fmaxf(ciou_q(pb, b).val, 0.f);
      const float sc = cok ? sigmoid(anchor_row(p, at)[4 * p.reg_max + gc]) : 0.f;
      m = powf(sc, q.alpha) * powf(ov, q.beta);
    }
    met[a] = m; ovl[a] = ov;
  }
  float pm = INFINITY;
  int pi = -1;
  for (int r = 0; r < q.topk; ++r) {                              // block-uniform: pm, pi and the break are the same in every thread
    float bm = -1.f;
    int bi = INT_MAX;
    for (int a = tid; a < A; a += 256) {                          // ascending, strict >: the lowest index among equal metrics
      const float m = met[a];
      if ((m < pm || (m == pm && a > pi)) && m > bm) { bm = m; bi = a; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(bm, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (om > bm || (om == bm && oi < bi)) { bm = om; bi = oi; }
    }
    if (lane == 0) { s_m[wave] = bm; s_i[wave] = bi; }
    __syncthreads();
    bm = s_m[0]; bi = s_i[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (s_m[w] > bm || (s_m[w] == bm && s_i[w] < bi)) { bm = s_m[w]; bi = s_i[w]; }
    __syncthreads();
    if (bi == INT_MAX) {                                          // fewer than topk anchors
      for (int k = r + tid; k < q.topk; k += 256) sel[k] = -1;
      break;
    }
    if (tid == 0) sel[r] = ovl[bi] >= 0.f ? bi : -1;              // selected but not inside: dropped
    pm = bm; pi = bi;
  }
}

__global__ __launch_bounds__(256) void tal_resolve_kernel(const TalP q) {
  const LossP& p = q.l;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)p.N * p.A) return;
  const int n = (int)(i / p.A), a = (int)(i - (long)n * p.A);
  const int g0 = min(max(p.gt_off[n], 0), q.G), g1 = min(max(p.gt_off[n + 1], 0), q.G);
  int best = -1;
  float bov = -1.f;
  for (int g = g0; g < g1; ++g) {
    const int* sel = q.sel + (long)g * q.topk;
    for (int r = 0; r < q.topk; ++r) {
      if (sel[r] == a) {
        const float ov = q.ovl[(long)g * p.A + a];
        if (ov > bov) { bov = ov; best = g; }
      }
    }
  }
  q.assigned[i] = best;
}

__global__ __launch_bounds__(256) void tal_gtmax_kernel(const TalP q) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= q.G) return;
  const int n = q.img[g], A = q.l.A;
  float M = 0.f, O = 0.f;
  if (n >= 0) {
    for (int r = 0; r < q.topk; ++r) {
      const int a = q.sel[(long)g * q.topk + r];
      if (a >= 0 && q.assigned[(long)n * A + a] == g) {
        M = fmaxf(M, q.met[(long)g * A + a]);
        O = fmaxf(O, q.ovl[(long)g * A + a]);
      }
    }
  }
  q.gmax[2 * g] = M; q.gmax[2 * g + 1] = O;
}

__global__ __launch_bounds__(256) void tal_value_kernel(const TalP q) {
  __shared__ float red[4][6];
  const LossP& p = q.l;
  const long i = (long)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int side = threadIdx.x & 3;
  float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // sum t, box, dfl, cls, #fg, sum ov
  if (i < (long)p.N * p.A) {
    const AnchorAt at = anchor_at(p, i);
    const int a = at.a;
    const float* row = anchor_row(p, at);
    const int g = q.assigned[i];
    float t = 0.f;
    int gc = -1;
    if (g >= 0) {
      t = q.met[(long)g * p.A + a] * q.gmax[2 * g + 1] / (q.gmax[2 * g] + 1e-9f);
      gc = p.gt_cls[g];
    }
    if (side == 0) q.tscore[i] = t;
    for (int c = side; c < p.nc; c += 4) v[3] += bce_logits(row[4 * p.reg_max + c], c == gc ? t : 0.f);
    if (g >= 0) {
      const float4 b = ld4(p.gt_xyxy + 4 * (long)g);
      const float4 st = ld4(q.stat + (i * 4 + side) * 4);
      const float lse = st.x + logf(st.y);
      const float* d = row + side * p.reg_max;
      const DflTarget tg = dfl_target(at, b, side, p.reg_max);
      const float wl = (float)tg.tr - tg.t, wr = 1.f - wl;
      v[2] = t * (0.25f * ((lse - d[tg.tl]) * wl + (lse - d[tg.tr]) * wr));
      if (side == 0) {
        const float4 pb = ld4(q.boxes + i * 4);
        v[1] = (1.f - ciou_q(pb, b).val) * t;
        v[0] = t; v[4] = 1.f; v[5] = q.ovl[(long)g * p.A + a];
      }
    }
  }
  block_sum_f32<6>(v, red);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < 6; ++k) q.partial[(long)blockIdx.x * 6 + k] = v[k];
}

__global__ __launch_bounds__(256) void tal_finalize_kernel(const TalP q, int blocks) {
  __shared__ float red[4][6];
  float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int b = threadIdx.x; b < blocks; b += 256)
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += q.partial[(long)b * 6 + k];
  block_sum_f32<6>(v, red);
  if (threadIdx.x == 0) {
    const float* t = v;
    const float T = fmaxf(t[0], 1.f);
    const float box = t[1] / T, dfl = t[2] / T, cls = t[3] / T;
    q.out[0] = box; q.out[1] = dfl; q.out[2] = cls;
    q.out[3] = t[4];
    q.out[4] = t[4] > 0.f ? t[5] / t[4] : 0.f;
    q.out[5] = T;
    q.out[6] = q.w_box * box + q.w_dfl * dfl + q.w_cls * cls;
    q.out[7] = 0.f;
  }
}

__global__ __launch_bounds__(256) void tal_grad_kernel(const TalP q) {
  const LossP& p = q.l;
  const long i = (long)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int side = threadIdx.x & 3;
  if (i >= (long)p.N * p.A) return;
  const AnchorAt at = anchor_at(p, i);
  const float* row = anchor_row(p, at);
  float* drow = q.d.map[at.l] + at.pix * q.d.ld[at.l];
  const bool acc = q.accumulate != 0;
  const float invT = 1.f / q.out[5];
  const int g = q.assigned[i];
  const float t = q.tscore[i];
  const int gc = g >= 0 ? p.gt_cls[g] : -1;
  const float kc = q.w_cls * invT;
  for (int c = side; c < p.nc; c += 4) {
    const float v = kc * (sigmoid(row[4 * p.reg_max + c]) - (c == gc ? t : 0.f));
    float* d = drow + 4 * p.reg_max + c;
    *d = acc ? *d + v : v;
  }
  float* dd = drow + side * p.reg_max;
  if (g < 0) {
    if (!acc)
      for (int k = 0; k < p.reg_max; ++k) dd[k] = 0.f;
    return;
  }
  const float4 b = ld4(p.gt_xyxy + 4 * (long)g);
  const float4 pb = ld4(q.boxes + i * 4);
  const float4 st = ld4(q.stat + (i * 4 + side) * 4);
  const SideDist sd{st.x, st.y, st.z};
  const CiouQ cq = ciou_q(pb, b);
  const float dcorner = -q.w_box * t * invT * ciou_dcorner(cq, pb, b, side);   // d total / d corner
  const float ddist = dcorner * (side < 2 ? -at.st : at.st);                   // corner = anchor -/+ dist * stride
  const DflTarget tg = dfl_target(at, b, side, p.reg_max);
  const float wl = (float)tg.tr - tg.t, wr = 1.f - wl;
  dfl_side_grad(row + side * p.reg_max, sd, p.reg_max, ddist, q.w_dfl * t * invT * 0.25f, tg, wl, wr, dd, acc);
}

inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }
inline int64_t blocks_of(int64_t NA) { return (NA + 63) / 64; }

struct TalLayout {
  int64_t boxes, stat, met, ovl, sel, img, gmax, assigned, tscore, partial, total;
};

inline TalLayout layout_of(int64_t N, int64_t A, int64_t G) {
  const int64_t NA = N * A;
  TalLayout t;
  int64_t o = 0;
  t.boxes = o;    o += align16(NA * 16);
  t.stat = o;     o += align16(NA * 64);
  t.met = o;      o += align16(G * A * 4);
  t.ovl = o;      o += align16(G * A * 4);
  t.sel = o;      o += align16(G * TAL_MAX_TOPK * 4);
  t.img = o;      o += align16(G * 4);
  t.gmax = o;     o += align16(G * 8);
  t.assigned = o; o += align16(NA * 4);
  t.tscore = o;   o += align16(NA * 4);
  t.partial = o;  o += align16(blocks_of(NA) * 6 * 4);
  t.total = o;
  return t;
}

}  // namespace

extern "C" int64_t mtbt_tal_loss_workspace_bytes(int N, int A, int G) {
  if (N <= 0 || A <= 0 || G < 0) return 0;
  return layout_of(N, A, G).total;
}

extern "C" int mtbt_sizeof_tal_loss_args(void) { return (int)sizeof(mtbt_tal_loss_args); }

extern "C" int mtbt_tal_det_loss(const mtbt_tal_loss_args* a, void* stream) {
  if (!a || !a->gt_xyxy || !a->gt_cls || !a->gt_off || !a->out || !a->workspace) return MTBT_EINVAL;
  if (a->n_levels < 1 || a->n_levels > 3 || a->N <= 0 || a->nc <= 0 || a->reg_max < 2 || a->reg_max > 64) return MTBT_EINVAL;
  if (a->topk < 1 || a->topk > TAL_MAX_TOPK || a->n_gt < 0 || !(a->img_size > 0.f)) return MTBT_EINVAL;
  const int no = 4 * a->reg_max + a->nc;
  TalP q{};
  LossP& p = q.l;
  int n_dmap = 0;
  for (int l = 0; l < a->n_levels; ++l) n_dmap += a->d_map[l] ? 1 : 0;
  if (n_dmap != 0 && n_dmap != a->n_levels) return MTBT_EINVAL;
  if (int rc = fill_levels(a, no, p, n_dmap ? &q.d : nullptr, a->d_map, a->d_map_pixel_stride)) return rc;
  const long A = p.A;
  const long NA = (long)a->N * A;
  if (NA > 0x7fffffffL / 64 || a->N > 0x7fffffff / 64) return MTBT_EINVAL;
  if (!aligned16(a->gt_xyxy) || !aligned16(a->workspace)) return MTBT_EALIGN;
  const TalLayout lay = layout_of(a->N, A, a->n_gt);
  if (a->workspace_bytes < lay.total) return MTBT_EWORKSPACE;
  p.N = a->N; p.nc = a->nc; p.reg_max = a->reg_max;
  p.gt_xyxy = a->gt_xyxy; p.gt_cls = a->gt_cls; p.gt_off = a->gt_off;
  p.iou_thresh = 0.f; p.smoothing = 0.f; p.training = 1; p.partial = nullptr;
  q.G = a->n_gt; q.topk = a->topk;
  q.alpha = a->alpha; q.beta = a->beta; q.w_box = a->w_box; q.w_dfl = a->w_dfl; q.w_cls = a->w_cls;
  char* w = reinterpret_cast<char*>(a->workspace);
  q.boxes = reinterpret_cast<float*>(w + lay.boxes); q.stat = reinterpret_cast<float*>(w + lay.stat);
  q.met = reinterpret_cast<float*>(w + lay.met); q.ovl = reinterpret_cast<float*>(w + lay.ovl);
  q.sel = reinterpret_cast<int*>(w + lay.sel); q.img = reinterpret_cast<int*>(w + lay.img);
  q.gmax = reinterpret_cast<float*>(w + lay.gmax);
  q.assigned = a->assigned ? a->assigned : reinterpret_cast<int*>(w + lay.assigned);
  q.tscore = a->target_score ? a->target_score : reinterpret_cast<float*>(w + lay.tscore);
  q.partial = reinterpret_cast<float*>(w + lay.partial);
  q.accumulate = a->accumulate;
  q.out = a->out;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned nb = (unsigned)blocks_of(NA);
  hipLaunchKernelGGL(tal_decode_kernel, dim3(nb), dim3(256), 0, s, q);
  if (q.G > 0) hipLaunchKernelGGL(tal_topk_kernel, dim3((unsigned)q.G), dim3(256), 0, s, q);
  hipLaunchKernelGGL(tal_resolve_kernel, dim3((unsigned)((NA + 255) / 256)), dim3(256), 0, s, q);
  if (q.G > 0) hipLaunchKernelGGL(tal_gtmax_kernel, dim3((unsigned)((q.G + 255) / 256)), dim3(256), 0, s, q);
  hipLaunchKernelGGL(tal_value_kernel, dim3(nb), dim3(256), 0, s, q);
  hipLaunchKernelGGL(tal_finalize_kernel, dim3(1), dim3(256), 0, s, q, (int)nb);
  if (n_dmap) hipLaunchKernelGGL(tal_grad_kernel, dim3(nb), dim3(256), 0, s, q);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}
