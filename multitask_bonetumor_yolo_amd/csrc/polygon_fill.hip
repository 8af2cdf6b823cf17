// Polygons -> bit-packed planes (mtbt_fill_polygons; the fill rule and the contract are in include/mtbt_hip.h), feeding
// `postprocess.fill_polygons`, `yolo_seg_planes` and the polygon ground truth of `preprocess.augment_samples_seg`.
//
// Packed layout as everywhere (mask_eval.hip): a plane is a run of H * pitch / 8 64-bit words, 8-byte aligned, padding bits zero.
//
// fill_polygons_kernel  grid (blocks of 256 consecutive words of a plane, planes).  A thread owns ONE 64-bit word: row Y, pixels
//                       64 * word .. 64 * word + 63.  The block walks its plane's polygons; a polygon's edges come through LDS in
//                       chunks of 256: thread i of the chunk reads vertex i and its successor (the last joins the first), clamps
//                       them, orients the edge upward (ay < by), drops it when it is horizontal or crosses none of the block's
//                       scanlines, and appends the rest to the chunk's buffer through an LDS counter (the order inside a polygon is
//                       free: XOR commutes, so the result does not depend on it).  Two edge buffers and three counters rotate, so a
//                       chunk costs one barrier.  Every thread then reads the kept edges at a wave-uniform address; a crossing
//                       edge toggles the pixels X < t of the word, t = ceil(num / den) with num = (bx-ax)(yc-ay) + (ax-8)(by-ay),
//                       den = 16 (by-ay).  Because "left of the edge" is X * den < num, the word is toggled whole when its last
//                       pixel is left, not at all when its first is not, and only a word the edge passes through pays the 64-bit
//                       division.  The running word `w` of a polygon lives in a register across its chunks; at the polygon's end
//                       acc |= w.  Then the clip rectangle and the padding mask, one 8-byte store, and the records: LDS atomics per
//                       block, one global integer atomic per record and block with a set pixel.
//                       Bound: LDS edge reads x words of the band; with the band filter a block of a large plane sees a few edges
//                       of a polygon, not all of them.
// finish_box_kernel     the box is gathered as maxima of (W - X, H - Y, X + 1, Y + 1) over zeroed memory (an empty plane stays
//                       all zero); one thread per plane turns the first two back into minima.
#include "bitplane.h"

namespace {

constexpr int PT = 256;          // threads of a block = words of its band = edges of a chunk
constexpr int LIM = 1 << 24;     // coordinates are clamped to [-LIM, LIM]: every product below stays under 2^52

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(PT) void fill_polygons_kernel(const mtbt_fill_polygons_args p, const int nw, const int plane0) {
  __shared__ int4 s_edge[2][PT];
  __shared__ int s_count[3];
  __shared__ unsigned s_area;
  __shared__ int s_box[4];
  const int tid = threadIdx.x, pl = plane0 + (int)blockIdx.y;
  const long words = (long)p.H * nw;                                   // < 2^31 / 64 + H
  const long g0 = (long)blockIdx.x * PT, g = g0 + tid;
  const bool live = g < words;
  const long gl = live ? g : words - 1;
  const int Y = (int)(gl / nw), word = (int)(gl - (long)Y * nw);
  const long yc = 16l * Y + 8;
  const long yc_lo = 16l * (g0 / nw) + 8, yc_hi = 16l * ((min(g0 + PT, words) - 1) / nw) + 8;   // the block's first and last scanline
  const long X0 = 64l * word, X1 = X0 + 63;

  if (tid < 3) s_count[tid] = 0;
  if (tid < 4) s_box[tid] = 0;
  if (tid == 0) s_area = 0u;
  __syncthreads();

  const int p0 = clampi(p.plane_offsets[pl], 0, p.n_polys), p1 = clampi(p.plane_offsets[pl + 1], 0, p.n_polys);
  u64 acc = 0ull;
  int k = 0;                                                           // chunks so far: picks the buffers
  for (int q = p0; q < p1; ++q) {
    const int v0 = clampi(p.poly_offsets[q], 0, p.n_vertices), v1 = clampi(p.poly_offsets[q + 1], 0, p.n_vertices);
    const int nv = v1 - v0;
    if (nv < 3) continue;                                              // block-uniform
    u64 w = 0ull;
    for (int e0 = 0; e0 < nv; e0 += PT, ++k) {
      int4* buf = s_edge[k & 1];
      int* cnt = &s_count[k % 3];
      if (tid == 0) s_count[(k + 1) % 3] = 0;                          // read last two chunks ago, with two barriers since
      const int e = e0 + tid;
      if (e < nv) {
        const int* va = p.vertices + 2l * (v0 + e);
        const int* vb = p.vertices + 2l * (v0 + (e + 1 == nv ? 0 : e + 1));
        int ax = clampi(va[0], -LIM, LIM), ay = clampi(va[1], -LIM, LIM);
        int bx = clampi(vb[0], -LIM, LIM), by = clampi(vb[1], -LIM, LIM);
        if (ay > by) {
          const int tx = ax, ty = ay;
          ax = bx; ay = by; bx = tx; by = ty;
        }
        if (ay != by && (long)ay <= yc_hi && (long)by > yc_lo) buf[atomicAdd(cnt, 1)] = make_int4(ax, ay, bx, by);
      }
      __syncthreads();
      const int ne = *cnt;
      for (int i = 0; i < ne; ++i) {
        const int4 ed = buf[i];
        if ((long)ed.y <= yc && yc < (long)ed.w) {                     // (ay <= yc) != (by <= yc) with ay < by
          const long dy = (long)ed.w - ed.y;
          const long num = ((long)ed.z - ed.x) * (yc - ed.y) + ((long)ed.x - 8) * dy, den = 16l * dy;
          u64 m;
          if (X1 * den < num) m = ~0ull;                               // the last pixel of the word is left of the edge
          else if (X0 * den >= num) m = 0ull;                          // the first is not
          else m = low_bits((long)(((u64)num + (u64)den - 1ull) / (u64)den) - X0);   // num > X0 * den >= 0
          w ^= m;
        }
      }
    }
    acc |= w;
  }

  int cx0 = 0, cy0 = 0, cx1 = p.W, cy1 = p.H;
  if (p.clip) {
    const int* c = p.clip + 4l * pl;
    cx0 = max(c[0], 0); cy0 = max(c[1], 0); cx1 = min(c[2], p.W); cy1 = min(c[3], p.H);
  }
  acc &= (Y >= cy0 && Y < cy1) ? (low_bits((long)cx1 - X0) & ~low_bits((long)cx0 - X0)) : 0ull;
  if (!live) acc = 0ull;
  if (live) reinterpret_cast<u64*>(p.out)[(long)pl * words + g] = acc;

  if (!p.area && !p.box) return;
  if (acc) {
    atomicAdd(&s_area, (unsigned)__popcll(acc));
    atomicMax(&s_box[0], p.W - ((int)X0 + (__ffsll((long long)acc) - 1)));
    atomicMax(&s_box[1], p.H - Y);
    atomicMax(&s_box[2], (int)X0 + 64 - __clzll((long long)acc));
    atomicMax(&s_box[3], Y + 1);
  }
  __syncthreads();
  if (s_area == 0u) return;
  if (tid == 0 && p.area) atomicAdd(p.area + pl, s_area);
  if (tid < 4 && p.box) atomicMax(p.box + 4l * pl + tid, s_box[tid]);
}

__global__ __launch_bounds__(PT) void finish_box_kernel(int* box, const int n, const int H, const int W) {
  const int pl = blockIdx.x * PT + threadIdx.x;
  if (pl >= n) return;
  int* b = box + 4l * pl;
  if (b[2] > 0) {          // not empty: b[0] = W - min X, b[1] = H - min Y
    b[0] = W - b[0];
    b[1] = H - b[1];
  }
}

}  // namespace

extern "C" int mtbt_sizeof_fill_polygons_args(int which) { return which == 0 ? (int)sizeof(mtbt_fill_polygons_args) : -1; }

extern "C" int mtbt_fill_polygons(const mtbt_fill_polygons_args* a, void* stream) {
  if (!a || !a->out || !a->poly_offsets || !a->plane_offsets) return MTBT_EINVAL;
  const mtbt_fill_polygons_args& p = *a;
  if (p.n < 0 || p.n_polys < 0 || p.n_vertices < 0 || (p.n_vertices > 0 && !p.vertices)) return MTBT_EINVAL;
  if (!plane_area_ok(p.H, p.W) || !plane_pitch_ok(p.W, p.pitch)) return MTBT_EINVAL;
  if (!aligned8(p.out) || !aligned_to(p.vertices) || !aligned_to(p.poly_offsets) || !aligned_to(p.plane_offsets) ||
      !aligned_to(p.clip) || !aligned_to(p.area) || !aligned_to(p.box))
    return MTBT_EALIGN;
  if (p.n == 0) return MTBT_OK;
  const int nw = p.pitch >> 3;
  const int64_t words = (int64_t)p.H * nw, blocks = (words + PT - 1) / PT;   // < 2^31 / (64 * 256) + H: fits the grid
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (p.area && hipMemsetAsync(p.area, 0, (size_t)p.n * sizeof(uint32_t), s) != hipSuccess) return MTBT_ELAUNCH;
  if (p.box && hipMemsetAsync(p.box, 0, (size_t)p.n * 4 * sizeof(int32_t), s) != hipSuccess) return MTBT_ELAUNCH;
  for (int plane0 = 0; plane0 < p.n; plane0 += 32768) {
    hipLaunchKernelGGL(fill_polygons_kernel, dim3((unsigned)blocks, (unsigned)(p.n - plane0 < 32768 ? p.n - plane0 : 32768)), dim3(PT), 0, s, p, nw, plane0);
    MTBT_LAUNCH_CHECK();
  }
  if (p.box) {
    hipLaunchKernelGGL(finish_box_kernel, dim3((unsigned)((p.n + PT - 1) / PT)), dim3(PT), 0, s, p.box, p.n, p.H, p.W);
    MTBT_LAUNCH_CHECK();
  }
  return MTBT_OK;
}
