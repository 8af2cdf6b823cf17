// Measurements of regions of bit-packed planes or label maps: mtbt_measure_regions (contract and THE MEASURE RULE in include/mtbt_hip.h),
// feeding `postprocess.measure_regions` / `measure_components` / `region_properties` / `measure_detections`.
//
// Packed layout as in components.hip: a plane is H rows of pitch = 8 * ceil(W / 64) bytes, pixel X is bit X & 7 of byte X >> 3, planes are
// 8-byte aligned and every access to one is an 8-byte load.  Bits X >= W are masked off where a row word is read.
//
// The hull of a region is the hull of, per LATTICE row Y (0 .. H), the leftmost and the rightmost corner of its pixels in the pixel rows
// Y - 1 and Y: at most 2 (H + 1) candidates.  The workspace holds them, per (plane of the launch group, region): R[Y] = the largest x1 + 1
// and L[Y] = the largest 16385 - x0 over the pixel runs x0 .. x1 touching lattice row Y, both raised by integer atomicMax from zero
// ("no pixel"), so one memset prepares them.
//
// mz_plane_kernel   plane mode, one thread per row word: area and perimeter are popcounts of the word against its four neighbours, sum X
//                   and sum X^2 come from popcounts against the six bit-position masks and their 21 pairwise products; summed over the
//                   workgroup, then seven 64-bit atomicAdds.  Bound: five 8-byte loads per 64 pixels.
// mz_label_kernel   label mode, one wave per 64 pixels of a row: the lanes that open a run of equal labels (ballots of "differs from the
//                   left lane") add the run's closed-form sums and its exposed sides (popcounts of four ballots under the run's mask) to
//                   their region: seven atomicAdds and up to four atomicMax per run.  Bound: the label map three times (row, above, below).
// mz_hull_kernel    one workgroup per (region, plane).  The present lattice rows are compacted in place, in row order (ballot prefix);
//                   thread 0 walks the right chain down and thread 64 the left chain up, each a monotone-chain stack kept in place over the
//                   list it reads (a pop while the turn is not strictly clockwise on the screen); the hull is the start, the right stack,
//                   the left stack.  Then over hull vertices only, all threads: area2, the farthest pair (one 64-bit key: d2, then the
//                   smallest i, then the smallest j), the extent across it, and per edge the farthest vertex and the shadow of the hull
//                   on it; the edges are compared as exact fractions (measure_exact.h).  Bound: the two serial walks (one dependent load
//                   per popped point), then h^2 / 256 pair evaluations per thread, from LDS when h <= 4096.
// No floating point anywhere in this file.  Measured times: DESIGN.md §8.
#include "bitplane.h"
#include "measure_exact.h"

namespace {

typedef long long i64;

constexpr int WT = 256;                   // threads of every workgroup here
constexpr int WW = WT / 64;               // waves per workgroup
constexpr int MAX_REGIONS = 65536;
constexpr int HCAP = 4096;                // hull vertices a workgroup keeps in LDS
constexpr int XOFF = PLANE_MAX_DIM + 1;   // L[Y] holds XOFF - x0 >= 1
constexpr u64 BIAS = 1ull << 40;          // added to a cross product (|.| < 2^31) so that it orders as an unsigned word

struct MzP {
  const u64* src;        // [n][H][nw] or null
  const int* labels;     // [n][H][W] or null
  int* tab;              // [planes of the group][C][2][H + 1]: R, then L
  u64* sums;             // [n][C][8]
  int* n_hull; int* hull; i64* hull_area2; i64* caliper; int* caliper_at;
  int plane0, H, W, nw, C, Vh;
};

int64_t tab_bytes_per_plane(int64_t H, int64_t C) { return C * 2 * (H + 1) * 4; }

__device__ __forceinline__ u64 row_word(const u64* plane, int y, int w, int H, int W, int nw) {   // zero outside the plane
  if (y < 0 || y >= H || w < 0 || w >= nw) return 0ull;
  return plane[(size_t)y * nw + w] & valid_bits(w, W);
}

__device__ __forceinline__ void add_u64(u64* p, u64 v) { if (v) atomicAdd(p, v); }
// a plain read may be stale, but only low (the words only grow): it can cost an atomic, never lose one
__device__ __forceinline__ void raise(int* p, int v) { if (*p < v) atomicMax(p, v); }

__device__ __forceinline__ void touch_rows(int* tab, int H, int y, int x0, int x1) {   // a run x0 .. x1 of pixel row y
  raise(tab + y, x1 + 1);
  raise(tab + y + 1, x1 + 1);
  raise(tab + (H + 1) + y, XOFF - x0);
  raise(tab + (H + 1) + y + 1, XOFF - x0);
}

// ---------------------------------------------------------------------------------------------------------------- plane mode
__global__ __launch_bounds__(WT) void mz_plane_kernel(const MzP p) {
  __shared__ u64 red[WW][7];
  const int pl = blockIdx.z;
  const size_t plane = (size_t)(p.plane0 + pl);
  const u64* src = p.src + plane * p.H * p.nw;
  const unsigned words = (unsigned)p.H * (unsigned)p.nw, t = blockIdx.x * WT + threadIdx.x;
  u64 v[7] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  if (t < words) {
    const int y = (int)(t / (unsigned)p.nw), w = (int)(t - (unsigned)y * (unsigned)p.nw);
    const u64 cur = row_word(src, y, w, p.H, p.W, p.nw);
    if (cur) {
      const u64 up = row_word(src, y - 1, w, p.H, p.W, p.nw), dn = row_word(src, y + 1, w, p.H, p.W, p.nw);
      const u64 lf = row_word(src, y, w - 1, p.H, p.W, p.nw), rt = row_word(src, y, w + 1, p.H, p.W, p.nw);
      const u64 area = (u64)__popcll(cur);
      const u64 per = (u64)(__popcll(cur & ~up) + __popcll(cur & ~dn) + __popcll(cur & ~((cur << 1) | (lf >> 63))) +
                            __popcll(cur & ~((cur >> 1) | (rt << 63))));
      const u64 M[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
                        0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};   // the positions with bit k set
      u64 s1 = 0ull, s2 = 0ull;                                  // sum b and sum b^2 over the set bit positions b
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        s1 += (u64)__popcll(cur & M[k]) << k;
#pragma unroll
        for (int l = 0; l < 6; ++l) s2 += (u64)__popcll(cur & M[k] & M[l]) << (k + l);
      }
      const u64 X0 = (u64)w * 64ull, sx = area * X0 + s1;
      v[0] = area; v[1] = per; v[2] = sx; v[3] = (u64)y * area;
      v[4] = area * X0 * X0 + 2ull * X0 * s1 + s2; v[5] = (u64)y * sx; v[6] = (u64)y * (u64)y * area;
      touch_rows(p.tab + (size_t)pl * 2 * (p.H + 1), p.H, y, (int)X0 + __ffsll((i64)cur) - 1, (int)X0 + 63 - __clzll((i64)cur));
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    if (lane == 0) red[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 7) {
    u64 s = 0ull;
#pragma unroll
    for (int w = 0; w < WW; ++w) s += red[w][threadIdx.x];
    add_u64(p.sums + plane * 8 + threadIdx.x, s);
  }
}

// ---------------------------------------------------------------------------------------------------------------- label mode
__global__ __launch_bounds__(WT) void mz_label_kernel(const MzP p) {
  const int pl = blockIdx.z;
  const size_t plane = (size_t)(p.plane0 + pl);
  const int* lab = p.labels + plane * p.H * p.W;
  const unsigned segs = (unsigned)p.H * (unsigned)p.nw, g = blockIdx.x * WW + (threadIdx.x >> 6);
  if (g >= segs) return;                                       // the whole wave
  const int lane = threadIdx.x & 63;
  const int y = (int)(g / (unsigned)p.nw), w = (int)(g - (unsigned)y * (unsigned)p.nw), x = w * 64 + lane;
  const bool in = x < p.W;
  const int* row = lab + (size_t)y * p.W;
  const int L = in ? row[x] : 0;
  const int U = (in && y > 0) ? row[x - p.W] : 0, D = (in && y + 1 < p.H) ? row[x + p.W] : 0;   // 0: outside the plane, no region's label
  const int lin = __shfl_up(L, 1, 64), rin = __shfl_down(L, 1, 64);
  int Lf = lin, Rt = rin;
  if (lane == 0) Lf = (x > 0 && in) ? row[x - 1] : 0;
  if (lane == 63) Rt = (x + 1 < p.W) ? row[x + 1] : 0;
  const bool reg = L >= 1 && L <= p.C;
  const u64 ahead = __ballot(reg && (lane == 0 || lin != L)), atail = __ballot(reg && (lane == 63 || rin != L));
  const u64 e_up = __ballot(reg && U != L), e_dn = __ballot(reg && D != L), e_lf = __ballot(reg && Lf != L), e_rt = __ballot(reg && Rt != L);
  if (!((ahead >> lane) & 1ull)) return;
  const int e = lane + __ffsll((i64)(atail >> lane)) - 1;      // the run lane .. e; a tail at or after an open run always exists
  const u64 rm = low_bits(e + 1) & ~low_bits(lane);
  const i64 x0 = x, x1 = w * 64 + e, len = x1 - x0 + 1;
  const u64 per = (u64)(__popcll(e_up & rm) + __popcll(e_dn & rm) + __popcll(e_lf & rm) + __popcll(e_rt & rm));
  const u64 sx = (u64)((x0 + x1) * len / 2);
  const u64 sxx = (u64)(x1 * (x1 + 1) * (2 * x1 + 1) / 6 - (x0 - 1) * x0 * (2 * x0 - 1) / 6);   // squares up to x1 less those up to x0 - 1
  const size_t r = plane * p.C + (size_t)(L - 1);
  u64* s = p.sums + r * 8;
  add_u64(s + 0, (u64)len); add_u64(s + 1, per); add_u64(s + 2, sx); add_u64(s + 3, (u64)y * (u64)len);
  add_u64(s + 4, sxx); add_u64(s + 5, (u64)y * sx); add_u64(s + 6, (u64)y * (u64)y * (u64)len);
  touch_rows(p.tab + ((size_t)pl * p.C + (size_t)(L - 1)) * 2 * (p.H + 1), p.H, y, (int)x0, (int)x1);
}

// ---------------------------------------------------------------------------------------------------------------- hull and calipers
__device__ __forceinline__ int px(int q) { return q & 0xFFFF; }   // a lattice point is x | y << 16
__device__ __forceinline__ int py(int q) { return q >> 16; }
// > 0 when a -> b -> c turns clockwise on the screen (y down): the sense E -> S -> W -> N
__device__ __forceinline__ i64 turn(int a, int b, int c) {
  return (i64)(px(b) - px(a)) * (py(c) - py(b)) - (i64)(py(b) - py(a)) * (px(c) - px(b));
}

__global__ __launch_bounds__(WT) void mz_hull_kernel(const MzP p) {
  __shared__ int hp[HCAP];
  __shared__ unsigned wcnt[WW];
  __shared__ int s_n[2];
  __shared__ u64 s_key, s_hi, s_lo, s_area2;
  __shared__ u64 bw_h[WT], bw_len[WT], br_h[WT], br_t[WT], br_len[WT];
  __shared__ i64 br_tmin[WT];
  __shared__ int bw_i[WT], bw_v[WT], br_i[WT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pl = blockIdx.z, H = p.H;
  const size_t reg = (size_t)(p.plane0 + pl) * p.C + blockIdx.x;
  int* hull = p.hull ? p.hull + reg * (size_t)p.Vh * 2 : nullptr;
  int* RT = p.tab + ((size_t)pl * p.C + blockIdx.x) * 2 * (H + 1);
  int* LT = RT + (H + 1);

  // the present lattice rows, compacted in place in row order: a batch is read whole before any of it is overwritten
  int m = 0;
  if (p.sums[reg * 8] != 0ull) {
    for (int base = 0; base <= H; base += WT) {
      const int Y = base + tid;
      const int rv = Y <= H ? RT[Y] : 0, lv = Y <= H ? LT[Y] : 0;
      const u64 bal = __ballot(rv != 0);
      if (lane == 0) wcnt[wave] = (unsigned)__popcll(bal);
      __syncthreads();
      int off = m, tot = 0;
#pragma unroll
      for (int w = 0; w < WW; ++w) { if (w < wave) off += (int)wcnt[w]; tot += (int)wcnt[w]; }
      if (rv != 0) {
        const int pos = off + __popcll(bal & low_bits(lane));
        RT[pos] = rv | (Y << 16);
        LT[pos] = (XOFF - lv) | (Y << 16);
      }
      m += tot;
      __syncthreads();
    }
  }
  if (m < 2) {                                                 // an empty region: every word zero (one pixel already has two lattice rows)
    if (tid == 0) { p.n_hull[reg] = 0; p.hull_area2[reg] = 0; }
    if (tid < 8) { p.caliper[reg * 8 + tid] = 0; p.caliper_at[reg * 8 + tid] = 0; }
    if (hull) for (int i = tid; i < 2 * p.Vh; i += WT) hull[i] = 0;
    return;
  }

  const int P0 = LT[0], Q = RT[m - 1];                         // the first and the last point in (y, x) order: vertices for certain
  if (tid == 0) { s_key = 0ull; s_hi = 0ull; s_lo = ~0ull; s_area2 = 0ull; }
  __syncthreads();
  const int steps = 2 * (H + 1) + 2;                           // a step pushes or pops, and a point is pushed once
  if (tid == 0) {                                              // P0, then down the right side to Q; the stack is RT[0 .. sz)
    int sz = 0, i = 0, ta = P0, tb = P0, c = RT[0];
    for (int st = 0; st < steps && i < m; ++st) {
      if (sz >= 1 && turn(ta, tb, c) <= 0) { --sz; tb = ta; ta = sz >= 2 ? RT[sz - 2] : P0; continue; }
      RT[sz++] = c; ta = tb; tb = c;
      if (++i < m) c = RT[i];
    }
    s_n[0] = sz;
  } else if (tid == 64) {                                      // Q, then up the left side to P0 (which closes it); the stack is LT[m - sz .. m)
    int sz = 0, j = m - 1, ta = Q, tb = Q, c = LT[m - 1];
    for (int st = 0; st < steps; ++st) {
      if (sz >= 1 && turn(ta, tb, c) <= 0) { --sz; tb = ta; ta = sz >= 2 ? LT[m - sz + 1] : Q; continue; }
      if (j == 0) break;
      LT[m - 1 - sz] = c; ++sz; ta = tb; tb = c;
      c = LT[--j];
    }
    s_n[1] = sz;
  }
  __syncthreads();
  const int na = s_n[0], nb = s_n[1], h = 1 + na + nb;         // <= 2 (H + 1)
  const bool in_lds = h <= HCAP;
  auto stacked = [&](int i) -> int { return i == 0 ? P0 : (i <= na ? RT[i - 1] : LT[m - 1 - (i - 1 - na)]); };
  if (in_lds) for (int i = tid; i < h; i += WT) hp[i] = stacked(i);
  __syncthreads();
  auto pt = [&](int i) -> int { return in_lds ? hp[i] : stacked(i); };

  if (hull) for (int i = tid; i < p.Vh; i += WT) {
    const int q = i < h ? pt(i) : 0;
    hull[2 * i] = px(q); hull[2 * i + 1] = py(q);
  }
  // area2, and the farthest pair as one key: d2, then the smallest i, then the smallest j
  u64 a2 = 0ull, key = 0ull;
  for (int i = tid; i < h; i += WT) {
    const int a = pt(i), b = pt(i + 1 == h ? 0 : i + 1);
    a2 += (u64)((i64)px(a) * py(b) - (i64)px(b) * py(a));
    for (int j = i + 1; j < h; ++j) {
      const int q = pt(j);
      const i64 dx = px(q) - px(a), dy = py(q) - py(a);
      const u64 k = ((u64)(dx * dx + dy * dy) << 32) | ((u64)(0xFFFF - i) << 16) | (u64)(0xFFFF - j);
      key = k > key ? k : key;
    }
  }
  atomicAdd(&s_area2, a2);
  atomicMax(&s_key, key);
  __syncthreads();
  const int ia = 0xFFFF - (int)((s_key >> 16) & 0xFFFFull), ib = 0xFFFF - (int)(s_key & 0xFFFFull);
  const int A = pt(ia), B = pt(ib);
  {
    const i64 ux = px(B) - px(A), uy = py(B) - py(A);
    u64 hi = 0ull, lo = ~0ull;
    for (int i = tid; i < h; i += WT) {
      const int q = pt(i);
      const u64 c = (u64)(ux * (py(q) - py(A)) - uy * (px(q) - px(A))) + BIAS;
      hi = c > hi ? c : hi; lo = c < lo ? c : lo;
    }
    if (lo <= hi) { atomicMax(&s_hi, hi); atomicMin(&s_lo, lo); }
  }
  // per edge: the farthest vertex and the shadow of the hull on the edge; the best edge of this thread by exact fractions
  int wi = -1, wv = 0, ri = -1;
  u64 wh = 0ull, wl = 1ull, rh = 0ull, rt = 0ull, rl = 1ull;
  i64 rtmin = 0;
  for (int i = tid; i < h; i += WT) {
    const int a = pt(i), b = pt(i + 1 == h ? 0 : i + 1);
    const i64 ex = px(b) - px(a), ey = py(b) - py(a);
    const u64 len2 = (u64)(ex * ex + ey * ey);
    i64 hmax = -1, tmin = 0, tmax = 0;
    int vq = 0;
    for (int j = 0; j < h; ++j) {
      const int q = pt(j);
      const i64 qx = px(q) - px(a), qy = py(q) - py(a);
      i64 cr = ex * qy - ey * qx;
      cr = cr < 0 ? -cr : cr;
      const i64 dt = ex * qx + ey * qy;
      if (cr > hmax) { hmax = cr; vq = j; }
      if (j == 0) { tmin = dt; tmax = dt; } else { tmin = dt < tmin ? dt : tmin; tmax = dt > tmax ? dt : tmax; }
    }
    const u64 hh = (u64)hmax, tt = (u64)(tmax - tmin);
    if (wi < 0 || mx_cmp_width(hh, len2, wh, wl) < 0) { wi = i; wv = vq; wh = hh; wl = len2; }
    if (ri < 0 || mx_cmp_rect(hh, tt, len2, rh, rt, rl) < 0) { ri = i; rh = hh; rt = tt; rl = len2; rtmin = tmin; }
  }
  bw_i[tid] = wi; bw_v[tid] = wv; bw_h[tid] = wh; bw_len[tid] = wl;
  br_i[tid] = ri; br_h[tid] = rh; br_t[tid] = rt; br_len[tid] = rl; br_tmin[tid] = rtmin;
  __syncthreads();
  if (tid == 0) {
    int b = 0;                                                 // thread 0 owns edge 0: h >= 4
    for (int t = 1; t < WT; ++t) {
      if (bw_i[t] < 0) continue;
      const int c = mx_cmp_width(bw_h[t], bw_len[t], bw_h[b], bw_len[b]);
      if (c < 0 || (c == 0 && bw_i[t] < bw_i[b])) b = t;
    }
    p.n_hull[reg] = h;
    p.hull_area2[reg] = (i64)s_area2;
    i64* cal = p.caliper + reg * 8;
    int* at = p.caliper_at + reg * 8;
    cal[0] = (i64)(s_key >> 32); cal[1] = (i64)(s_hi - s_lo); cal[2] = (i64)bw_h[b]; cal[3] = (i64)bw_len[b];
    at[0] = px(A); at[1] = py(A); at[2] = px(B); at[3] = py(B); at[4] = bw_i[b]; at[5] = bw_v[b]; at[7] = 0;
  } else if (tid == 64) {
    int b = 0;
    for (int t = 1; t < WT; ++t) {
      if (br_i[t] < 0) continue;
      const int c = mx_cmp_rect(br_h[t], br_t[t], br_len[t], br_h[b], br_t[b], br_len[b]);
      if (c < 0 || (c == 0 && br_i[t] < br_i[b])) b = t;
    }
    i64* cal = p.caliper + reg * 8;
    cal[4] = (i64)br_h[b]; cal[5] = (i64)br_t[b]; cal[6] = br_tmin[b]; cal[7] = (i64)br_len[b];
    p.caliper_at[reg * 8 + 6] = br_i[b];
  }
}

bool shape_ok(int n, int H, int W) { return n >= 0 && plane_dims_ok(H, W); }

}  // namespace

extern "C" int mtbt_sizeof_measure_args(int which) { return which == 0 ? (int)sizeof(mtbt_measure_args) : -1; }

extern "C" int64_t mtbt_measure_workspace_bytes(int n, int H, int W, int max_regions) {
  if (!shape_ok(n, H, W) || max_regions < 1 || max_regions > MAX_REGIONS) return MTBT_EINVAL;
  if (n == 0) return 0;
  const int64_t per = tab_bytes_per_plane(H, max_regions);
  return up16((int64_t)chunk_of(n, per) * per);
}

extern "C" int mtbt_measure_regions(const mtbt_measure_args* args, void* stream) {
  if (!args) return MTBT_EINVAL;
  const mtbt_measure_args& a = *args;
  if (!shape_ok(a.n, a.H, a.W) || !plane_pitch_ok(a.W, a.pitch)) return MTBT_EINVAL;
  if (a.max_regions < 1 || a.max_regions > MAX_REGIONS || a.max_hull < 4 || a.reserved[0] != 0 || a.reserved[1] != 0) return MTBT_EINVAL;
  if ((!a.packed && !a.labels) || (!a.labels && a.max_regions != 1)) return MTBT_EINVAL;
  if (!a.sums || !a.n_hull || !a.hull_area2 || !a.caliper || !a.caliper_at) return MTBT_EINVAL;
  const int64_t need = mtbt_measure_workspace_bytes(a.n, a.H, a.W, a.max_regions);
  if (a.workspace_bytes < need || (need > 0 && !a.workspace)) return MTBT_EINVAL;
  if (!aligned_n(a.packed, 8) || !aligned_n(a.sums, 8) || !aligned_n(a.hull_area2, 8) || !aligned_n(a.caliper, 8) ||
      !aligned_n(a.workspace, 16) || !aligned_n(a.labels, 4) || !aligned_n(a.n_hull, 4) || !aligned_n(a.hull, 4) || !aligned_n(a.caliper_at, 4))
    return MTBT_EALIGN;
  if (a.n == 0) return MTBT_OK;

  MzP p = {};
  p.src = reinterpret_cast<const u64*>(a.packed);
  p.labels = a.labels;
  p.tab = reinterpret_cast<int*>(a.workspace);
  p.sums = reinterpret_cast<u64*>(a.sums);
  p.n_hull = a.n_hull; p.hull = a.hull; p.hull_area2 = reinterpret_cast<i64*>(a.hull_area2);
  p.caliper = reinterpret_cast<i64*>(a.caliper); p.caliper_at = a.caliper_at;
  p.H = a.H; p.W = a.W; p.nw = (int)plane_words(a.W); p.C = a.max_regions; p.Vh = a.max_hull;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(a.sums, 0, (size_t)a.n * p.C * 64, s) != hipSuccess) return MTBT_ELAUNCH;
  const int64_t per = tab_bytes_per_plane(a.H, p.C), words = (int64_t)a.H * p.nw;
  const int chunk = chunk_of(a.n, per);
  for (int p0 = 0; p0 < a.n; p0 += chunk) {                    // the groups take the workspace in turn, in stream order
    const unsigned c = (unsigned)(a.n - p0 < chunk ? a.n - p0 : chunk);
    p.plane0 = p0;
    if (hipMemsetAsync(a.workspace, 0, (size_t)c * (size_t)per, s) != hipSuccess) return MTBT_ELAUNCH;
    if (a.labels) hipLaunchKernelGGL(mz_label_kernel, dim3((unsigned)((words + WW - 1) / WW), 1, c), dim3(WT), 0, s, p);
    else hipLaunchKernelGGL(mz_plane_kernel, dim3((unsigned)((words + WT - 1) / WT), 1, c), dim3(WT), 0, s, p);
    MTBT_LAUNCH_CHECK();
    hipLaunchKernelGGL(mz_hull_kernel, dim3((unsigned)p.C, 1, c), dim3(WT), 0, s, p);
    MTBT_LAUNCH_CHECK();
  }
  return MTBT_OK;
}
