// Instance-mask loss (YOLOv8-seg single_mask_loss / crop_mask) and its gradient with respect to the mask coefficients and the
// prototypes: the operator that lets training reach Segment.cv4 and use the prototypes as a per-instance basis.  Definition:
// include/mtbt_hip.h (mtbt_mask_loss_args).  Positives come from the detection loss's own prologue (match_anchor, loss_match.h), or,
// through mtbt_instance_mask_loss_assigned, from an assignment the caller hands in (the task-aligned assigner's, det_loss_tal.hip).
//
//   ml_match_kernel     4 lanes per (image, anchor): match[b][a] = matched GT row or -1; zero rows of d_mc for non-positives
//   ml_assigned_kernel  its sibling for a given assignment: match[b][a] = assigned[b][a] if it is a row of image b, else -1; the same
//                       zeroing; reads no detection map.  Everything below reads match[b][a] only and is shared by both entry points
//   ml_list_kernel      one workgroup per GT row g: the anchors matched to g, ascending, compacted into the image's positive list
//                       (list[b][start_g .. start_g + cnt_g), GT rows of an image in order) -- sized for all A anchors
//   ml_count_kernel     #positives of the batch (integer sum of cnt)
//   ml_value_kernel     workgroup = (16 positives of one GT); its 4 waves stride over the 16-pixel groups of the GT's box:
//                         logits^T [16 px x 16 pos] = P [px x nm] . MC^T [nm x pos]      8 x v_mfma_f32_16x16x4_f32
//                         BCE-with-logits -> per-positive sums;  r = k_g (sigmoid - t) stays in the accumulator's registers and IS the
//                         A operand of  d_mc [16 pos x nm] += R [pos x px] . P [px x nm]  (4 K-steps x 2 column tiles)
//                       wave partials summed in LDS in wave order
//   ml_dprotos_kernel   gather form: workgroup = (image, 16 x 16 pixel tile), wave w owns 4 rows; loops over the image's GT boxes that
//                       touch the tile and their positives 16 at a time:
//                         logits [16 pos x 16 px] = MC . P^T;  r in registers IS the B operand of
//                         d_protos^T [nm x px] += MC^T [nm x pos] . R [pos x px]
//                       and writes every pixel of the tile once (zeros included): no atomics where boxes overlap
//   ml_finalize_kernel  sum of the per-positive losses in list order / norm
// All three products use the exact-fp32 MFMA; the K index of a 16x16x4 step is free to permute, so channels are assigned to K as
// c = 8 (lane >> 4) + step (8 consecutive floats per lane straight from global memory) and pixels / positives as 4 (lane >> 4) + step
// (exactly the accumulator layout of the previous product): no operand goes through LDS.  Deterministic: every sum has a fixed order.
#include <cmath>

#include "common.h"
#include "loss_match.h"

namespace {

constexpr int NM = 32;
constexpr int VALUE_GRID_X = 16;   // 16-positive groups of one GT in flight (grid.y; the others are looped over)

struct MaskLossP {
  LossP l;
  const float* mc;
  long mbs, mas, mcs;
  const float* protos;
  const float* gtm;
  int hp, wp, S, ry, rx;       // ry = S / hp, rx = S / wp
  float sx, sy;                // wp / S, hp / S
  float weight;
  int G;
  // workspace
  int* match;                  // [N * A]
  int* list;                   // [N * A]
  float* loss_pos;             // [N * A]  (list order)
  int* start;                  // [G]
  int* cnt;                    // [G]
  int* img;                    // [G]
  int* n_pos;                  // [1]
  float* d_mc;
  int acc_dmc;
  void* d_protos;
  int acc_dprotos;
  float* out;
};

struct BoxQ {
  float x1, y1, x2, y2, area;
  int xs, xe, ys, ye;          // a superset of the inside pixels, clipped to the map (the float predicate decides)
  __device__ __forceinline__ bool inside(int x, int y) const {
    const float fx = (float)x, fy = (float)y;
    return fx >= x1 && fx < x2 && fy >= y1 && fy < y2;
  }
};

__device__ __forceinline__ BoxQ box_of(const MaskLossP& p, int g) {
  const float4 b = ld4(p.l.gt_xyxy + 4 * (long)g);
  BoxQ q;
  q.x1 = b.x * p.sx; q.y1 = b.y * p.sy; q.x2 = b.z * p.sx; q.y2 = b.w * p.sy;
  q.area = (q.x2 - q.x1) * (q.y2 - q.y1);
  q.xs = (int)floorf(fminf(fmaxf(q.x1, 0.f), (float)p.wp));
  q.ys = (int)floorf(fminf(fmaxf(q.y1, 0.f), (float)p.hp));
  q.xe = (int)ceilf(fminf(fmaxf(q.x2, 0.f), (float)p.wp));
  q.ye = (int)ceilf(fminf(fmaxf(q.y2, 0.f), (float)p.hp));
  return q;
}

// What both match kernels end in: match[g] = `row` (a GT row, or -1), and the d_mc row of an anchor that is not a positive zeroed, 8
// floats per lane of the anchor's 4 (the value kernel writes the positives' rows only).
__device__ __forceinline__ void store_match(const MaskLossP& p, long g, int side, int row) {
  if (side == 0) p.match[g] = row;
  if (p.d_mc && !p.acc_dmc && row < 0) {
    f32x4* d = reinterpret_cast<f32x4*>(p.d_mc + g * NM + side * 8);
    d[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    d[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

__global__ __launch_bounds__(256) void ml_match_kernel(const MaskLossP p) {
  const long g = (long)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int side = threadIdx.x & 3;
  const AnchorMatch am = match_anchor(p.l, g, side);
  if (am.live) store_match(p, g, side, am.pos ? am.bi : -1);
}

// The match from a given assignment: 4 lanes per (image, anchor) like ml_match_kernel, so that a non-foreground anchor's d_mc row is
// zeroed by the same 16-byte stores.  An entry is foreground only if it is a row of its own image below n_gt; anything else is
// background and is never used as an index.
__global__ __launch_bounds__(256) void ml_assigned_kernel(const MaskLossP p, const int* __restrict__ assigned) {
  const long g = (long)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int side = threadIdx.x & 3;
  if (g >= (long)p.l.N * p.l.A) return;
  const int n = (int)(g / p.l.A);
  const int v = assigned[g];
  const int g0 = max(p.l.gt_off[n], 0), g1 = min(p.l.gt_off[n + 1], p.G);
  store_match(p, g, side, v >= g0 && v < g1 ? v : -1);
}

__global__ __launch_bounds__(256) void ml_list_kernel(const MaskLossP p) {
  __shared__ int s_n;
  __shared__ int red[4][2];
  __shared__ int wtot[4];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = p.l.A;
  if (tid == 0) s_n = -1;
  __syncthreads();
  for (int n = tid; n < p.l.N; n += 256)
    if (p.l.gt_off[n] <= g && g < p.l.gt_off[n + 1]) s_n = n;   // at most one n
  __syncthreads();
  const int n = s_n;
  if (n < 0) {                                                  // a row of no image
    if (tid == 0) { p.start[g] = 0; p.cnt[g] = 0; p.img[g] = -1; }
    return;
  }
  const int* m = p.match + (long)n * A;
  int lt = 0, eq = 0;
  for (int a = tid; a < A; a += 256) {
    const int v = m[a];
    lt += (v >= 0 && v < g) ? 1 : 0;
    eq += (v == g) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { lt += __shfl_xor(lt, o, 64); eq += __shfl_xor(eq, o, 64); }
  if (lane == 0) { red[wave][0] = lt; red[wave][1] = eq; }
  __syncthreads();
  const int start = red[0][0] + red[1][0] + red[2][0] + red[3][0];
  const int cnt = red[0][1] + red[1][1] + red[2][1] + red[3][1];
  if (tid == 0) { p.start[g] = start; p.cnt[g] = cnt; p.img[g] = n; }
  if (cnt == 0) return;
  int* dst = p.list + (long)n * A + start;
  int running = 0;
  for (int base = 0; base < A && running < cnt; base += 256) {  // block-uniform bounds
    const int a = base + tid;
    const bool f = a < A && m[a] == g;
    const unsigned long long bal = __ballot(f);
    const int pre = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wave; ++w) woff += wtot[w];
    if (f) dst[running + woff + pre] = a;
    running += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void ml_count_kernel(const MaskLossP p) {
  __shared__ int red[4];
  int s = 0;
  for (int g = threadIdx.x; g < p.G; g += 256) s += p.cnt[g];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *p.n_pos = red[0] + red[1] + red[2] + red[3];
}

template <bool GRAD>
__global__ __launch_bounds__(256) void ml_value_kernel(const MaskLossP p) {
  __shared__ float s_loss[4][16];
  __shared__ float s_d[4][16][NM + 1];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, j = lane >> 4;
  const int cnt = p.cnt[g];
  if ((int)blockIdx.y * 16 >= cnt) return;
  const int n = p.img[g], A = p.l.A;
  const int* list = p.list + (long)n * A + p.start[g];
  const BoxQ q = box_of(p, g);
  const int bw = max(q.xe - q.xs, 0), bh = max(q.ye - q.ys, 0);
  const int npx = bw * bh, npg = (npx + 15) >> 4;
  const int np = *p.n_pos;
  const float norm = np > 0 ? (float)np : (float)p.l.N;
  const float kg = p.weight / (norm * q.area);
  const float* pr = p.protos + (long)n * p.hp * p.wp * NM;
  const float* tg = p.gtm + (long)n * p.S * p.S;

  for (int rg = blockIdx.y; rg * 16 < cnt; rg += gridDim.y) {
    // B operand of the logits product: MC^T, n = positive `col`, k-step ks <-> channel 8 j + ks
    const int row = rg * 16 + col;
    const bool rvalid = row < cnt;
    const int a = list[rvalid ? row : rg * 16];
    float bm[8];
    {
      const float* mp = p.mc + (long)n * p.mbs + (long)a * p.mas + (long)(j * 8) * p.mcs;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) bm[ks] = rvalid ? mp[ks * p.mcs] : 0.f;
    }
    float lsum = 0.f;
    f32x4 accd[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int pg = wave; pg < npg; pg += 4) {
      // A operand: P, m = pixel `col` of the group, channels 8 j .. 8 j + 7
      float pa[8];
      {
        const int idx = pg * 16 + col;
        const bool pv = idx < npx;
        const int yy = pv ? idx / bw : 0, xx = pv ? idx - yy * bw : 0;
        const float* pp = pr + ((long)(q.ys + yy) * p.wp + (q.xs + xx)) * NM + j * 8;
        float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
        if (pv) { v0 = ld4(pp); v1 = ld4(pp + 4); }
        pa[0] = v0.x; pa[1] = v0.y; pa[2] = v0.z; pa[3] = v0.w; pa[4] = v1.x; pa[5] = v1.y; pa[6] = v1.z; pa[7] = v1.w;
      }
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[ks], bm[ks], acc, 0, 0, 0);
      // acc[r] = logit of positive `col` at pixel 4 j + r of the group
      float rr[4];
      long poff[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int idx = pg * 16 + 4 * j + r;
        const bool pv = idx < npx;
        const int yy = pv ? idx / bw : 0, xx = pv ? idx - yy * bw : 0;
        const int y = q.ys + yy, x = q.xs + xx;
        const bool in = pv && rvalid && q.inside(x, y);
        poff[r] = pv ? ((long)y * p.wp + x) * NM : -1;
        float rv = 0.f;
        if (in) {
          const float t = tg[(long)(y * p.ry) * p.S + x * p.rx];
          lsum += bce_logits(acc[r], t);
          rv = kg * (sigmoid(acc[r]) - t);
        }
        rr[r] = rv;
      }
      if constexpr (GRAD) {
        // d_mc += R . P: A = R (m = positive `col`, k-step r <-> pixel 4 j + r: the registers above), B = P (n = channel nt * 16 + col)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            const float bp = poff[r] >= 0 ? pr[poff[r] + nt * 16 + col] : 0.f;
            accd[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(rr[r], bp, accd[nt], 0, 0, 0);
          }
        }
      }
    }
    // per positive: the four lane groups in a fixed (symmetric) order, then the waves in order
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    if (lane < 16) s_loss[wave][lane] = lsum;
    if constexpr (GRAD) {
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_d[wave][4 * j + r][nt * 16 + col] = accd[nt][r];
    }
    __syncthreads();
    if (tid < 16 && rg * 16 + tid < cnt)
      p.loss_pos[(long)n * A + p.start[g] + rg * 16 + tid] = ((s_loss[0][tid] + s_loss[1][tid]) + (s_loss[2][tid] + s_loss[3][tid])) / q.area;
    if constexpr (GRAD) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int i = tid + u * 256, r = i >> 5, c = i & 31;
        if (rg * 16 + r < cnt) {
          const float v = (s_d[0][r][c] + s_d[1][r][c]) + (s_d[2][r][c] + s_d[3][r][c]);
          float* d = p.d_mc + ((long)n * A + list[rg * 16 + r]) * NM + c;
          *d = p.acc_dmc ? *d + v : v;
        }
      }
    }
    __syncthreads();
  }
}

template <typename T> struct store4;
template <> struct store4<float> {
  static __device__ __forceinline__ void run(float* d, f32x4 v, bool acc) {
    f32x4* q = reinterpret_cast<f32x4*>(d);
    *q = acc ? *q + v : v;
  }
};
template <> struct store4<bf16_t> {
  static __device__ __forceinline__ void run(bf16_t* d, f32x4 v, bool acc) {
    uint2* q = reinterpret_cast<uint2*>(d);
    if (acc) {
      const uint2 o = *q;
      v += f32x4{__uint_as_float(o.x << 16), __uint_as_float(o.x & 0xffff0000u), __uint_as_float(o.y << 16), __uint_as_float(o.y & 0xffff0000u)};
    }
    *q = uint2{(uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16), (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16)};
  }
};
template <> struct store4<f16_t> {
  static __device__ __forceinline__ void run(f16_t* d, f32x4 v, bool acc) {
    uint2* q = reinterpret_cast<uint2*>(d);
    if (acc) {
      const uint2 o = *q;
      v += f32x4{h_lo(o.x), h_hi(o.x), h_lo(o.y), h_hi(o.y)};
    }
    *q = uint2{pk_h2(v[0], v[1]), pk_h2(v[2], v[3])};
  }
};

template <typename T>
__global__ __launch_bounds__(256) void ml_dprotos_kernel(const MaskLossP p, int tiles_x) {
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, j = lane >> 4;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * 16, y0 = ty * 16 + wave * 4;            // this wave: rows y0 .. y0 + 3, pixel x0 + col
  const int x = x0 + col;
  const int A = p.l.A;
  const float* pr = p.protos + (long)n * p.hp * p.wp * NM;
  const float* tg = p.gtm + (long)n * p.S * p.S;
  // B operand of the logits product: P, n = pixel `col` of row cg, channels 8 j .. 8 j + 7
  float pb[4][8], t[4];
#pragma unroll
  for (int cg = 0; cg < 4; ++cg) {
    const int y = y0 + cg;
    const bool pv = x < p.wp && y < p.hp;
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
    t[cg] = 0.f;
    if (pv) {
      const float* pp = pr + ((long)y * p.wp + x) * NM + j * 8;
      v0 = ld4(pp); v1 = ld4(pp + 4);
      t[cg] = tg[(long)(y * p.ry) * p.S + x * p.rx];
    }
    pb[cg][0] = v0.x; pb[cg][1] = v0.y; pb[cg][2] = v0.z; pb[cg][3] = v0.w; pb[cg][4] = v1.x; pb[cg][5] = v1.y; pb[cg][6] = v1.z; pb[cg][7] = v1.w;
  }
  f32x4 accp[4][2];
#pragma unroll
  for (int cg = 0; cg < 4; ++cg) accp[cg][0] = accp[cg][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int np = *p.n_pos;
  const float norm = np > 0 ? (float)np : (float)p.l.N;
  const int g0 = p.l.gt_off[n], g1 = min(p.l.gt_off[n + 1], p.G);
  for (int g = g0; g < g1; ++g) {
    const int cnt = p.cnt[g];
    if (cnt == 0) continue;
    const BoxQ q = box_of(p, g);
    if (q.xe <= x0 || q.xs >= x0 + 16 || q.ye <= y0 || q.ys >= y0 + 4) continue;     // wave-uniform
    bool in[4];
    bool any = false;
#pragma unroll
    for (int cg = 0; cg < 4; ++cg) {
      in[cg] = x < p.wp && y0 + cg < p.hp && q.inside(x, y0 + cg);
      any = any || in[cg];
    }
    if (__ballot(any) == 0ull) continue;
    const float kg = p.weight / (norm * q.area);
    const int* list = p.list + (long)n * A + p.start[g];
    for (int rg = 0; rg * 16 < cnt; ++rg) {
      // A operands: MC for the logits (m = positive `col`, channels 8 j + ks) and MC^T for d_protos^T (m = channel mt * 16 + col,
      // k-step r <-> positive 4 j + r)
      float am[8], a3[2][4];
      {
        const int row = rg * 16 + col;
        const bool rv = row < cnt;
        const int a = list[rv ? row : rg * 16];
        const float* mp = p.mc + (long)n * p.mbs + (long)a * p.mas + (long)(j * 8) * p.mcs;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) am[ks] = rv ? mp[ks * p.mcs] : 0.f;
      }
      bool rvalid[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rg * 16 + 4 * j + r;
        rvalid[r] = row < cnt;
        const int a = list[rvalid[r] ? row : rg * 16];
        const float* mp = p.mc + (long)n * p.mbs + (long)a * p.mas;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) a3[mt][r] = rvalid[r] ? mp[(long)(mt * 16 + col) * p.mcs] : 0.f;
      }
#pragma unroll
      for (int cg = 0; cg < 4; ++cg) {
        if (__ballot(in[cg]) == 0ull) continue;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(am[ks], pb[cg][ks], acc, 0, 0, 0);
        // acc[r] = logit of positive 4 j + r at this lane's pixel of row cg
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float rr = (in[cg] && rvalid[r]) ? kg * (sigmoid(acc[r]) - t[cg]) : 0.f;
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) accp[cg][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a3[mt][r], rr, accp[cg][mt], 0, 0, 0);
        }
      }
    }
  }
  // accp[cg][mt][r] = d_protos[channel mt * 16 + 4 j + r] at pixel (x, y0 + cg): four consecutive channels per store
  T* out = reinterpret_cast<T*>(p.d_protos) + (long)n * p.hp * p.wp * NM;
  if (x < p.wp) {
#pragma unroll
    for (int cg = 0; cg < 4; ++cg) {
      const int y = y0 + cg;
      if (y >= p.hp) continue;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) store4<T>::run(out + ((long)y * p.wp + x) * NM + mt * 16 + 4 * j, accp[cg][mt], p.acc_dprotos != 0);
    }
  }
}

__global__ __launch_bounds__(256) void ml_finalize_kernel(const MaskLossP p) {
  __shared__ float red[4][1];
  const int A = p.l.A;
  float s[1] = {0.f};
  for (int n = 0; n < p.l.N; ++n) {
    int k = 0;
    for (int g = p.l.gt_off[n]; g < min(p.l.gt_off[n + 1], p.G); ++g) k += p.cnt[g];
    const float* lp = p.loss_pos + (long)n * A;
    for (int i = threadIdx.x; i < k; i += 256) s[0] += lp[i];
  }
  block_sum_f32<1>(s, red);
  if (threadIdx.x == 0) {
    const int np = *p.n_pos;
    const float norm = np > 0 ? (float)np : (float)p.l.N;
    p.out[0] = s[0] / norm;
    p.out[1] = (float)np;
  }
}

inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

}  // namespace

// match, list, loss_pos, start, cnt, img: N * A words each (n_gt <= N * A), + the positive count
extern "C" int64_t mtbt_mask_loss_workspace_bytes(int N, int A, int hp, int wp, int nm) {
  if (N <= 0 || A <= 0 || hp <= 0 || wp <= 0 || nm != NM) return 0;
  return 6 * align16((int64_t)N * A * 4) + 16;
}

extern "C" int mtbt_sizeof_mask_loss_args(void) { return (int)sizeof(mtbt_mask_loss_args); }

// One body for both entry points: without `by_assignment` it decodes and matches (ml_match_kernel), with it the match is taken from the
// assignment (ml_assigned_kernel; the maps give the anchor count only).  Everything behind the match is the same launch sequence.
static int run_mask_loss(const mtbt_mask_loss_args* a, const int32_t* assigned, bool by_assignment, void* stream) {
  if (!a || !a->gt_xyxy || !a->gt_off || !a->mc || !a->protos || !a->gt_masks || !a->out || !a->workspace) return MTBT_EINVAL;
  if (by_assignment && !assigned) return MTBT_EINVAL;
  if (a->n_levels < 1 || a->n_levels > 3 || a->N <= 0 || a->hp <= 0 || a->wp <= 0) return MTBT_EINVAL;
  if (!by_assignment && (a->reg_max <= 0 || a->reg_max > 64)) return MTBT_EINVAL;
  if (a->nm != NM || a->n_gt < 0) return MTBT_EINVAL;
  const int S = (int)a->img_size;
  if (S <= 0 || (float)S != a->img_size || S % a->hp || S % a->wp) return MTBT_EINVAL;
  if (a->dprotos_dtype != MTBT_F32 && a->dprotos_dtype != MTBT_BF16 && a->dprotos_dtype != MTBT_F16) return MTBT_EINVAL;
  MaskLossP p;
  if (int rc = fill_levels(a, by_assignment ? 0 : 4 * a->reg_max, p.l)) return rc;
  const long A = p.l.A;
  const long NA = (long)a->N * A;
  if (NA > 0x7fffffffL / NM || a->n_gt > NA || a->N > 65535) return MTBT_EINVAL;
  if (a->workspace_bytes < mtbt_mask_loss_workspace_bytes(a->N, (int)A, a->hp, a->wp, a->nm)) return MTBT_EINVAL;
  if (!aligned16(a->gt_xyxy) || !aligned16(a->protos) || !aligned16(a->workspace) || (a->d_mc && !aligned16(a->d_mc)) ||
      (a->d_protos && !aligned16(a->d_protos)))
    return MTBT_EALIGN;
  p.l.N = a->N; p.l.nc = 0; p.l.reg_max = a->reg_max;
  p.l.gt_xyxy = a->gt_xyxy; p.l.gt_cls = nullptr; p.l.gt_off = a->gt_off;
  p.l.iou_thresh = a->iou_thresh; p.l.smoothing = 0.f; p.l.training = 0; p.l.partial = nullptr;
  p.mc = a->mc; p.mbs = a->mc_batch_stride; p.mas = a->mc_anchor_stride; p.mcs = a->mc_channel_stride;
  p.protos = a->protos; p.gtm = a->gt_masks;
  p.hp = a->hp; p.wp = a->wp; p.S = S; p.ry = S / a->hp; p.rx = S / a->wp;
  p.sx = (float)((double)a->wp / (double)S); p.sy = (float)((double)a->hp / (double)S);
  p.weight = a->weight; p.G = a->n_gt;
  char* w = reinterpret_cast<char*>(a->workspace);
  const int64_t seg = align16(NA * 4);
  p.match = reinterpret_cast<int*>(w); p.list = reinterpret_cast<int*>(w + seg); p.loss_pos = reinterpret_cast<float*>(w + 2 * seg);
  p.start = reinterpret_cast<int*>(w + 3 * seg); p.cnt = reinterpret_cast<int*>(w + 4 * seg); p.img = reinterpret_cast<int*>(w + 5 * seg);
  p.n_pos = reinterpret_cast<int*>(w + 6 * seg);
  p.d_mc = a->d_mc; p.acc_dmc = a->accumulate_dmc; p.d_protos = a->d_protos; p.acc_dprotos = a->accumulate_dprotos;
  p.out = a->out;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long mb = (NA + 63) / 64;
  if (by_assignment) hipLaunchKernelGGL(ml_assigned_kernel, dim3((unsigned)mb), dim3(256), 0, s, p, assigned);
  else hipLaunchKernelGGL(ml_match_kernel, dim3((unsigned)mb), dim3(256), 0, s, p);
  if (p.G > 0) hipLaunchKernelGGL(ml_list_kernel, dim3((unsigned)p.G), dim3(256), 0, s, p);
  hipLaunchKernelGGL(ml_count_kernel, dim3(1), dim3(256), 0, s, p);
  if (p.G > 0) {
    if (p.d_mc) hipLaunchKernelGGL(ml_value_kernel<true>, dim3((unsigned)p.G, VALUE_GRID_X), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(ml_value_kernel<false>, dim3((unsigned)p.G, VALUE_GRID_X), dim3(256), 0, s, p);
  }
  if (p.d_protos) {
    const int tiles_x = (a->wp + 15) / 16, tiles_y = (a->hp + 15) / 16;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)a->N);
    if (a->dprotos_dtype == MTBT_F32) hipLaunchKernelGGL(ml_dprotos_kernel<float>, grid, dim3(256), 0, s, p, tiles_x);
    else if (a->dprotos_dtype == MTBT_BF16) hipLaunchKernelGGL(ml_dprotos_kernel<bf16_t>, grid, dim3(256), 0, s, p, tiles_x);
    else hipLaunchKernelGGL(ml_dprotos_kernel<f16_t>, grid, dim3(256), 0, s, p, tiles_x);
  }
  hipLaunchKernelGGL(ml_finalize_kernel, dim3(1), dim3(256), 0, s, p);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}

extern "C" int mtbt_instance_mask_loss(const mtbt_mask_loss_args* a, void* stream) { return run_mask_loss(a, nullptr, false, stream); }

extern "C" int mtbt_instance_mask_loss_assigned(const mtbt_mask_loss_args* a, const int32_t* assigned, void* stream) {
  return run_mask_loss(a, assigned, true, stream);
}
