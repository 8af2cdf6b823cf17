// Surface-distance records of pairs of bit-packed planes: mtbt_surface_distances (contract in include/mtbt_hip.h), feeding
// `metrics.SurfaceDistanceMetrics` (Hausdorff, its percentile, average symmetric surface distance, normalised surface Dice).
//
// Packed layout as in mask_eval.hip: a plane is H rows of pitch = 8 * ceil(W / 64) bytes, pixel X is bit X & 7 of byte X >> 3, planes
// are 8-byte aligned and every access to one is an 8-byte load.  Bits X >= W are masked off where a row word is read.
// Everything but sum_d is integer arithmetic: the squared distance between two pixels is an integer below 2^29 (H, W <= 16384).
//
// The entry point takes the pairs in chunks of at most CHUNK and runs four kernels per chunk; the workspace holds one chunk's
// edge planes, column distances, row offsets and d^2 lists.
//
// surface_edges_kernel   one wave per (pair, side, column of 64-bit words), lane = pixel column.  Row y's edge word comes from the
//                        words of rows y - 1, y, y + 1 and the two neighbour words (4-neighbour rule, outside the image = unset);
//                        lane 0 stores it.  A downward and an upward sweep leave g(y, x) = vertical distance to the nearest edge
//                        pixel of column x as uint16 (0xFFFF: the column has none).  The row words are wave-uniform loads, the g
//                        stores 128 contiguous bytes per wave.  Bound: the latency of the 2 H dependent sweep steps.
// surface_scan_kernel    one workgroup per (pair, side): popcounts of the edge rows -> exclusive row offsets and |edge set|.
//                        Compaction is by this prefix: no atomics anywhere.
// surface_rows_kernel    one workgroup per (pair, direction, row) with an edge pixel in it; the OTHER side's g row is staged in
//                        LDS (2 W bytes).  A lane per edge pixel scans outward, dx = 0, 1, 2, ... on both sides, keeping
//                        best = min(dx^2 + g^2), and stops at dx^2 >= best: exact, and the work is bounded by the answer.
//                        Neighbouring lanes read neighbouring uint16 (two lanes per bank word: a broadcast).  d^2 goes to
//                        list[offset[row] + rank in row]: the directed lists are in row-major order, B->A right behind A->B.
//                        Skipped for a pair with an empty side.  Latency-bound and divergent.
// surface_select_kernel  one workgroup per (pair, segment: A->B, B->A, pooled): max, count <= tol2, sum of sqrt in fp64 (thread t
//                        adds items t, t + 256, ... in order, then a fixed tree: the same bits on every run) and the order
//                        statistics by bitwise search from the top bit of the maximum down: v | 1 << b is kept when
//                        count(list < v | 1 << b) <= k.  The statistic at k + 1 costs one more pass (count <= v, least item > v).
#include "bitplane.h"

namespace {

constexpr int RT = 256;                         // threads of the scan, row and select workgroups
constexpr int RW = RT / 64;
constexpr unsigned NONE16 = 0xFFFFu;

struct Layout {   // byte offsets of one chunk's sections in the workspace, each 16-byte aligned
  int64_t edge, g, rowoff, tot, list, total;
};

Layout layout_of(int64_t c, int64_t H, int64_t W) {
  const int64_t pitch = plane_pitch(W), Wp = pitch * 8;
  Layout l;
  int64_t off = 0;
  l.edge = off;   off = up16(off + c * 2 * H * pitch);
  l.g = off;      off = up16(off + c * 2 * H * Wp * 2);
  l.rowoff = off; off = up16(off + c * 2 * H * 4);
  l.tot = off;    off = up16(off + c * 2 * 4);
  l.list = off;   off = up16(off + c * 2 * H * W * 4);
  l.total = off;
  return l;
}

int chunk_of(int n, int H, int W) { return ::chunk_of(n, layout_of(1, H, W).total); }   // pairs per launch group

struct SurfP {
  const u64* a;
  const u64* b;
  u64* edge;          // [c][2][H][words_x]
  uint16_t* g;        // [c][2][H][Wp]
  unsigned* rowoff;   // [c][2][H]
  unsigned* tot;      // [c][2]
  unsigned* list;     // [c][2 H W]
  unsigned* n_edge;
  unsigned* max_d2;
  unsigned* n_within;
  double* sum_d;
  unsigned* rank_d2;
  double q[4];
  int pair0, H, W, words_x;
  unsigned tol2;
  int Q;
};

// ---------------------------------------------------------------------------------------------------------------- edges + columns
__global__ __launch_bounds__(64) void surface_edges_kernel(const SurfP p) {
  const int wx = blockIdx.x, side = blockIdx.y, pr = blockIdx.z, lane = threadIdx.x;
  const int H = p.H, nw = p.words_x, Wp = nw * 64;
  const u64* src = (side ? p.b : p.a) + (size_t)(p.pair0 + pr) * H * nw;
  u64* edge = p.edge + (size_t)(pr * 2 + side) * H * nw;
  uint16_t* g = p.g + (size_t)(pr * 2 + side) * H * Wp + wx * 64 + lane;
  const u64 vc = valid_bits(wx, p.W), vr = wx + 1 < nw ? valid_bits(wx + 1, p.W) : 0ull;
  const bool has_l = wx > 0, has_r = wx + 1 < nw;

  u64 up = 0ull, cur = src[wx] & vc;
  unsigned dist = NONE16;
  for (int y = 0; y < H; ++y) {
    const u64* row = src + (size_t)y * nw;
    const u64 down = y + 1 < H ? row[nw + wx] & vc : 0ull;
    const u64 l = has_l ? row[wx - 1] : 0ull;             // a word left of the last one has no padding bits
    const u64 r = has_r ? row[wx + 1] & vr : 0ull;
    const u64 e = cur & ~(up & down & ((cur << 1) | (l >> 63)) & ((cur >> 1) | (r << 63)));
    if (lane == 0) edge[(size_t)y * nw + wx] = e;
    dist = ((e >> lane) & 1ull) ? 0u : (dist == NONE16 ? NONE16 : dist + 1u);   // < H <= 16384: never reaches 0xFFFF by counting
    g[(size_t)y * Wp] = (uint16_t)dist;
    up = cur;
    cur = down;
  }
  dist = NONE16;
  for (int y = H - 1; y >= 0; --y) {                     // a lane reads back only what it stored itself
    const unsigned gv = g[(size_t)y * Wp];
    dist = gv == 0u ? 0u : (dist == NONE16 ? NONE16 : dist + 1u);
    if (dist < gv) g[(size_t)y * Wp] = (uint16_t)dist;
  }
}

// ---------------------------------------------------------------------------------------------------------------- row offsets
__global__ __launch_bounds__(RT) void surface_scan_kernel(const SurfP p) {
  __shared__ unsigned part[RT];
  const int side = blockIdx.x, pr = blockIdx.y, tid = threadIdx.x;
  const int H = p.H, nw = p.words_x;
  const u64* edge = p.edge + (size_t)(pr * 2 + side) * H * nw;
  unsigned* rowoff = p.rowoff + (size_t)(pr * 2 + side) * H;
  const int per = (H + RT - 1) / RT, y0 = min(H, tid * per), y1 = min(H, y0 + per);   // thread t owns rows y0 .. y1
  unsigned mine = 0u;
  for (int y = y0; y < y1; ++y)
    for (int w = 0; w < nw; ++w) mine += (unsigned)__popcll(edge[(size_t)y * nw + w]);
  part[tid] = mine;
  __syncthreads();
  unsigned before = 0u, total = 0u;
  for (int t = 0; t < RT; ++t) {
    const unsigned v = part[t];
    before += t < tid ? v : 0u;
    total += v;
  }
  for (int y = y0; y < y1; ++y) {
    rowoff[y] = before;
    for (int w = 0; w < nw; ++w) before += (unsigned)__popcll(edge[(size_t)y * nw + w]);
  }
  if (tid == 0) {
    p.tot[pr * 2 + side] = total;
    p.n_edge[(size_t)(p.pair0 + pr) * 2 + side] = total;
  }
}

// ---------------------------------------------------------------------------------------------------------------- row pass
__global__ __launch_bounds__(RT) void surface_rows_kernel(const SurfP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  uint16_t* gl = reinterpret_cast<uint16_t*>(lds_raw);   // the other side's g row: Wp entries
  const int y = blockIdx.x, d = blockIdx.y, pr = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = p.H, W = p.W, nw = p.words_x, Wp = nw * 64;
  const unsigned n_src = p.tot[pr * 2 + d], n_oth = p.tot[pr * 2 + 1 - d];
  if (n_src == 0u || n_oth == 0u) return;                // an undefined pair: nothing is listed
  const unsigned* rowoff = p.rowoff + (size_t)(pr * 2 + d) * H;
  const unsigned roff = rowoff[y], rend = y + 1 < H ? rowoff[y + 1] : n_src;
  if (rend == roff) return;                              // no edge pixel in this row (uniform over the workgroup)

  const uint4* gsrc = reinterpret_cast<const uint4*>(p.g + ((size_t)(pr * 2 + 1 - d) * H + y) * Wp);   // Wp * 2 bytes, 128-byte aligned
  for (int i = tid; i < Wp / 8; i += RT) reinterpret_cast<uint4*>(lds_raw)[i] = gsrc[i];
  __syncthreads();

  const u64* erow = p.edge + ((size_t)(pr * 2 + d) * H + y) * nw;
  unsigned* out = p.list + (size_t)pr * 2 * H * W + (d ? p.tot[pr * 2] : 0u) + roff;
  unsigned prefix = 0u;
  for (int w = 0; w < nw; ++w) {
    const u64 e = erow[w];
    if ((w & (RW - 1)) == wave && ((e >> lane) & 1ull)) {
      const int x = w * 64 + lane;
      const unsigned g0 = gl[x];
      unsigned best = g0 == NONE16 ? 0xFFFFFFFFu : g0 * g0;
      const int reach = max(x, W - 1 - x);
      for (int dx = 1; dx <= reach; ++dx) {
        const unsigned dx2 = (unsigned)dx * (unsigned)dx;
        if (dx2 >= best) break;
        if (x - dx >= 0) {
          const unsigned v = gl[x - dx];
          if (v != NONE16) best = min(best, dx2 + v * v);
        }
        if (x + dx < W) {
          const unsigned v = gl[x + dx];
          if (v != NONE16) best = min(best, dx2 + v * v);
        }
      }
      out[prefix + (unsigned)__popcll(e & ((1ull << lane) - 1ull))] = best;
    }
    prefix += (unsigned)__popcll(e);
  }
}

// ---------------------------------------------------------------------------------------------------------------- select + reduce
__global__ __launch_bounds__(RT) void surface_select_kernel(const SurfP p) {
  __shared__ unsigned red[RW];
  __shared__ double dred[RT];
  const int seg = blockIdx.x, pr = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t pair = (size_t)(p.pair0 + pr);
  unsigned nA = p.tot[pr * 2], nB = p.tot[pr * 2 + 1];
  if (nA == 0u || nB == 0u) nA = nB = 0u;                // undefined: every record but n_edge is zero
  const unsigned first = seg == 1 ? nA : 0u, m = seg == 0 ? nA : (seg == 1 ? nB : nA + nB);
  const unsigned* list = p.list + (size_t)pr * 2 * p.H * p.W + first;

  unsigned mx = 0u, within = 0u;
  double sum = 0.0;
  for (unsigned i = tid; i < m; i += RT) {
    const unsigned v = list[i];
    mx = max(mx, v);
    within += v <= p.tol2 ? 1u : 0u;
    if (seg < 2) sum += sqrt((double)v);
  }
  mx = block_extreme_u32<RW, true>(mx, red, lane, wave);
  if (seg < 2) {
    within = block_sum_u32<RW>(within, red, lane, wave);
    dred[tid] = sum;
    __syncthreads();
    for (int s = RT / 2; s > 0; s >>= 1) {
      if (tid < s) dred[tid] += dred[tid + s];
      __syncthreads();
    }
    if (tid == 0) {
      p.max_d2[pair * 2 + seg] = mx;
      p.n_within[pair * 2 + seg] = within;
      p.sum_d[pair * 2 + seg] = dred[0];
    }
  }

  const int top = mx ? 31 - __clz(mx) : -1;              // no item has a bit above this one
  for (int qi = 0; qi < p.Q; ++qi) {
    unsigned lo_v = 0u, hi_v = 0u;
    if (m > 0u) {
      const unsigned k = (unsigned)floor(p.q[qi] * (double)(m - 1u));     // one IEEE product: the host forms the same one
      const unsigned k_hi = min(k + 1u, m - 1u);
      for (int b = top; b >= 0; --b) {
        const unsigned t = lo_v | (1u << b);
        unsigned c = 0u;
        for (unsigned i = tid; i < m; i += RT) c += list[i] < t ? 1u : 0u;
        if (block_sum_u32<RW>(c, red, lane, wave) <= k) lo_v = t;
      }
      unsigned c = 0u, nxt = 0xFFFFFFFFu;
      for (unsigned i = tid; i < m; i += RT) {
        const unsigned v = list[i];
        c += v <= lo_v ? 1u : 0u;
        if (v > lo_v) nxt = min(nxt, v);
      }
      c = block_sum_u32<RW>(c, red, lane, wave);
      nxt = block_extreme_u32<RW, false>(nxt, red, lane, wave);
      hi_v = c > k_hi ? lo_v : nxt;                      // c <= k_hi < m: an item above lo_v exists
    }
    if (tid == 0) {
      unsigned* r = p.rank_d2 + ((pair * p.Q + qi) * 3 + seg) * 2;
      r[0] = lo_v;
      r[1] = hi_v;
    }
  }
}

bool shape_ok(int n, int H, int W) { return n >= 0 && plane_dims_ok(H, W); }

}  // namespace

extern "C" int mtbt_sizeof_surface_args(int which) { return which == 0 ? (int)sizeof(mtbt_surface_args) : -1; }

extern "C" int64_t mtbt_surface_distances_workspace_bytes(int n, int H, int W) {
  if (!shape_ok(n, H, W)) return MTBT_EINVAL;
  if (n == 0) return 0;
  return layout_of(chunk_of(n, H, W), H, W).total;
}

extern "C" int mtbt_surface_distances(const mtbt_surface_args* args, void* stream) {
  if (!args) return MTBT_EINVAL;
  const mtbt_surface_args& a = *args;
  if (!shape_ok(a.n, a.H, a.W) || !plane_pitch_ok(a.W, a.pitch)) return MTBT_EINVAL;
  if (a.Q < 0 || a.Q > 4) return MTBT_EINVAL;
  for (int i = 0; i < a.Q; ++i)
    if (!(a.q[i] >= 0.0 && a.q[i] <= 1.0)) return MTBT_EINVAL;   // NaN fails both comparisons
  if (!a.a || !a.b || !a.n_edge || !a.max_d2 || !a.n_within || !a.sum_d || (a.Q > 0 && !a.rank_d2)) return MTBT_EINVAL;
  const int64_t need = mtbt_surface_distances_workspace_bytes(a.n, a.H, a.W);
  if (a.workspace_bytes < need || (need > 0 && !a.workspace)) return MTBT_EINVAL;
  if (!aligned_n(a.a, 8) || !aligned_n(a.b, 8) || !aligned_n(a.workspace, 16) || !aligned_n(a.n_edge, 4) || !aligned_n(a.max_d2, 4) ||
      !aligned_n(a.n_within, 4) || !aligned_n(a.sum_d, 8) || !aligned_n(a.rank_d2, 4))
    return MTBT_EALIGN;
  if (a.n == 0) return MTBT_OK;

  const int chunk = chunk_of(a.n, a.H, a.W);
  const Layout l = layout_of(chunk, a.H, a.W);
  unsigned char* ws = reinterpret_cast<unsigned char*>(a.workspace);
  SurfP p;
  p.a = reinterpret_cast<const u64*>(a.a);
  p.b = reinterpret_cast<const u64*>(a.b);
  p.edge = reinterpret_cast<u64*>(ws + l.edge);
  p.g = reinterpret_cast<uint16_t*>(ws + l.g);
  p.rowoff = reinterpret_cast<unsigned*>(ws + l.rowoff);
  p.tot = reinterpret_cast<unsigned*>(ws + l.tot);
  p.list = reinterpret_cast<unsigned*>(ws + l.list);
  p.n_edge = a.n_edge; p.max_d2 = a.max_d2; p.n_within = a.n_within; p.sum_d = a.sum_d; p.rank_d2 = a.rank_d2;
  for (int i = 0; i < 4; ++i) p.q[i] = i < a.Q ? a.q[i] : 0.0;
  p.H = a.H; p.W = a.W; p.words_x = a.pitch >> 3; p.tol2 = a.tol2; p.Q = a.Q;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned lds = (unsigned)p.words_x * 64u * 2u;   // <= 32 KiB
  for (int p0 = 0; p0 < a.n; p0 += chunk) {              // the chunks share the workspace: stream order keeps them apart
    const unsigned c = (unsigned)(a.n - p0 < chunk ? a.n - p0 : chunk);
    p.pair0 = p0;
    hipLaunchKernelGGL(surface_edges_kernel, dim3((unsigned)p.words_x, 2, c), dim3(64), 0, s, p);
    MTBT_LAUNCH_CHECK();
    hipLaunchKernelGGL(surface_scan_kernel, dim3(2, c), dim3(RT), 0, s, p);
    MTBT_LAUNCH_CHECK();
    hipLaunchKernelGGL(surface_rows_kernel, dim3((unsigned)p.H, 2, c), dim3(RT), lds, s, p);
    MTBT_LAUNCH_CHECK();
    hipLaunchKernelGGL(surface_select_kernel, dim3(3, c), dim3(RT), 0, s, p);
    MTBT_LAUNCH_CHECK();
  }
  return MTBT_OK;
}
