// Bit-packed planes -> polygons and COCO run lengths: mtbt_trace_contours and mtbt_rle_encode (contract and THE CONTOUR RULE in
// include/mtbt_hip.h), feeding `postprocess.trace_contours` / `contour_polygons` / `yolo_seg_rows` / `labelme_shapes` and `rle_encode` /
// `coco_segm_results`.
//
// Packed layout as in components.hip: a plane is H rows of pitch = 8 * ceil(W / 64) bytes, pixel X is bit X & 7 of byte X >> 3, planes are
// 8-byte aligned and every access to one is an 8-byte load.  Bits X >= W are masked off where a row word is read.
//
// CONTOURS.  A lattice vertex (x, y) sees the 2 x 2 pixels a = (x - 1, y - 1), b = (x, y - 1), c = (x - 1, y), d = (x, y).  The edge that
// LEAVES it heading E exists when d & ~b, S when c & ~d, W when a & ~c, N when b & ~a; the edge that ARRIVES heading E when c & ~a, S when
// a & ~b, W when b & ~d, N when d & ~c.  A PASS is a contour vertex together with the direction it is left in: pass_D = out_D & ~in_D
// (an edge whose predecessor goes the same way runs straight on; at a saddle both leaving edges are passes).  All of this is 64 vertices at a
// time from four row words and two shifts ("vertex word" wv holds the vertices 64 wv .. 64 wv + 63 of a lattice row).  The passes of a
// plane are numbered by (key, direction): the number of a pass is an exclusive prefix sum of popcounts -- no atomics.  The successor of
// a pass is the pass at the far end of its straight run: a bit scan along the row for E / W, a column walk for S / N.  The successor is a
// permutation of the passes whose cycles are the contours; their starts (the smallest E pass of a cycle; E passes are numbered in key
// order) and the distance of every pass to its start come from pointer jumping: a fixed ceil(log2(min(V, 2 H W + 2))) rounds of ping-ponged
// launches, each doubling the window a pass has seen.  A prefix sum over the passes of (is a start, length of its contour) gives a
// contour's index and offset at once, because pass order is key order.  Then every pass stores its vertex at offset + rank.
//
// ct_count_kernel    one thread per vertex word: the popcount of its four pass masks.  Count only: summed per workgroup, one integer
//                    atomicAdd on n_vertices.  Bound: four 8-byte loads per 64 vertices (neighbours share them in L1 / L2).
// ct_rowscan_kernel  one workgroup per plane: exclusive prefix over the vertex words (as cc_scan_kernel), n_vertices, and the plane's working
//                    count nv (0 when n_vertices > V: every later kernel then leaves the plane alone).
// ct_link_kernel     one wave per vertex word, lane = vertex: key | direction << 30 and the successor of every pass.  Bound: the run walks --
//                    a column walk is one 8-byte load per row of the run, dependent on nothing but divergent; the loop bounds are H and the
//                    words of a row.
// ct_jump_kernel     one thread per pass, one launch per round: (min start, distance to it) over the window [i, i + 2^k) and the pass 2^k
//                    further on, from the pair of the pass and of its current target.  Bound: two scattered 12-byte reads per pass and round.
// ct_tilesum_kernel  per tile of 2048 passes the number of starts and the vertices of their contours (length = distance of the start's
//                    successor to the start + 1).
// ct_tilescan_kernel one workgroup per plane: exclusive prefix over the tiles, n_contours, zeros in the table rows no contour owns.
// ct_starts_kernel   the prefix inside every tile: a start learns its contour's index and offset and opens its table rows.
// ct_scatter_kernel  one thread per pass: vertex row offset + rank, and the pass's share of area2 (horizontal passes only) and of the box (only
//                    where a plain read shows the bound would move) by integer atomics.
// Measured times and what is known about each bound: DESIGN.md §8.
//
// RUN LENGTHS.  A transition is a pixel that differs from its predecessor in column-major order (the pixel above; for row 0 the last
// pixel of the column to the left; unset before pixel (0, 0)): 64 columns at a time, word[y] ^ word[y - 1].  One wave walks the rows of a
// 128-row band of one word column, lane = column, and counts; a prefix over (column, band) in column-major order gives every band the
// number of the run it opens and the position of the transition before it; the second walk stores position differences.
#include "bitplane.h"

namespace {

constexpr int WT = 256;                   // threads of every workgroup here
constexpr int WW = WT / 64;               // waves per workgroup
constexpr int WORDS_PER_WAVE = 4;         // ct_link_kernel
constexpr int ITEMS = 8;                  // passes per thread of the tile kernels
constexpr int TILE = WT * ITEMS;
constexpr int MAX_CONTOURS = 65536;
constexpr int BAND = 128;                 // rows of a run-length band
constexpr unsigned NONE = 0xFFFFFFFFu;    // "no E pass seen yet" in the high half of a (start, distance) pair
constexpr unsigned KEY_MASK = 0x3FFFFFFFu;   // a key is below (16385)^2 < 2^30; the two bits above hold the direction

int64_t pass_capacity(int64_t H, int64_t W, int64_t V) {   // more passes than 2 H W + 2 no plane has
  const int64_t most = 2 * H * W + 2;
  return V < most ? V : most;
}

struct Layout {   // byte offsets of the sections of the workspace (all n planes), each 16-byte aligned
  int64_t wordoff, nv, key, nxt0, nxt_a, nxt_b, md_a, md_b, tsum, total;
};

Layout layout_of(int64_t n, int64_t H, int64_t W, int64_t V) {
  const int64_t nwv = W / 64 + 1, Ve = pass_capacity(H, W, V), ntiles = (Ve + TILE - 1) / TILE;
  Layout l;
  int64_t off = 0;
  l.wordoff = off; off = up16(off + n * (H + 1) * nwv * 4);
  l.nv = off;      off = up16(off + n * 4);
  l.key = off;     off = up16(off + n * Ve * 4);
  l.nxt0 = off;    off = up16(off + n * Ve * 4);
  l.nxt_a = off;   off = up16(off + n * Ve * 4);
  l.nxt_b = off;   off = up16(off + n * Ve * 4);
  l.md_a = off;    off = up16(off + n * Ve * 8);
  l.md_b = off;    off = up16(off + n * Ve * 8);
  l.tsum = off;    off = up16(off + n * ntiles * 8);
  l.total = off;
  return l;
}

struct CtP {
  const u64* src;        // [n][H][nw]
  unsigned* wordoff;     // [n][(H + 1) * nwv]: passes of the vertex word, then their exclusive prefix
  int* nv;               // [n]: n_vertices, or 0 when it exceeds V
  unsigned* key;         // [n][Ve]: key | direction << 30
  int* nxt0;             // [n][Ve]: the successor
  int* nxt_a; int* nxt_b;   // [n][Ve]: the pass 2^k further on, ping-ponged; after the rounds the spare one holds a start's contour index
  u64* md_a; u64* md_b;     // [n][Ve]: start << 32 | distance, ping-ponged; the spare one holds a start's length << 32 | offset
  uint2* tsum;           // [n][ntiles]
  int* n_vertices; int* n_contours; int* vertices; int* offset; int* count; u64* area2; int* box; int* start;
  int plane0, H, W, nw, nwv, conn8, C, V, Ve, ntiles;
};

// pixel word w of row y; zero outside the plane
__device__ __forceinline__ u64 row_word(const u64* plane, int y, int w, int H, int W, int nw) {
  if (y < 0 || y >= H || w < 0 || w >= nw) return 0ull;
  return plane[(size_t)y * nw + w] & valid_bits(w, W);
}

__device__ __forceinline__ unsigned pixel(const u64* plane, int x, int y, int H, int W, int nw) {
  if (x < 0 || x >= W || y < 0 || y >= H) return 0u;
  return (unsigned)(plane[(size_t)y * nw + (x >> 6)] >> (x & 63)) & 1u;
}

struct VMasks { u64 oE, oS, oW, oN, pE, pS, pW, pN; };   // leaving edges and passes of the 64 vertices of one vertex word

__device__ __forceinline__ VMasks vertex_masks(const u64* plane, int y, int wv, int H, int W, int nw) {
  const u64 upc = row_word(plane, y - 1, wv, H, W, nw), upl = row_word(plane, y - 1, wv - 1, H, W, nw);
  const u64 dnc = row_word(plane, y, wv, H, W, nw), dnl = row_word(plane, y, wv - 1, H, W, nw);
  const u64 b = upc, a = (upc << 1) | (upl >> 63), d = dnc, c = (dnc << 1) | (dnl >> 63);
  VMasks m;
  m.oE = d & ~b; m.oS = c & ~d; m.oW = a & ~c; m.oN = b & ~a;
  m.pE = m.oE & ~(c & ~a); m.pS = m.oS & ~(a & ~b); m.pW = m.oW & ~(b & ~d); m.pN = m.oN & ~(d & ~c);
  return m;
}

__device__ __forceinline__ unsigned passes_of(const VMasks& m) {
  return (unsigned)(__popcll(m.pE) + __popcll(m.pS) + __popcll(m.pW) + __popcll(m.pN));
}

__device__ __forceinline__ unsigned passes_below(const VMasks& m, int bit) {   // passes at the vertices of the word before `bit`
  const u64 lo = (1ull << bit) - 1ull;
  return (unsigned)(__popcll(m.pE & lo) + __popcll(m.pS & lo) + __popcll(m.pW & lo) + __popcll(m.pN & lo));
}

// ---------------------------------------------------------------------------------------------------------------- count
template <bool ONLY>
__global__ __launch_bounds__(WT) void ct_count_kernel(const CtP p) {
  __shared__ unsigned red[WW];
  const int pl = blockIdx.z;
  const size_t plane = (size_t)(p.plane0 + pl);
  const u64* src = p.src + plane * p.H * p.nw;
  const unsigned words = (unsigned)(p.H + 1) * (unsigned)p.nwv, t = blockIdx.x * WT + threadIdx.x;
  unsigned c = 0u;
  if (t < words) {
    const int y = (int)(t / (unsigned)p.nwv), wv = (int)(t - (unsigned)y * (unsigned)p.nwv);
    c = passes_of(vertex_masks(src, y, wv, p.H, p.W, p.nw));
    if (!ONLY) p.wordoff[plane * words + t] = c;
  }
  if (ONLY) {
    c = wave_sum_u32(c);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned s = 0u;
#pragma unroll
      for (int w = 0; w < WW; ++w) s += red[w];
      if (s) atomicAdd(p.n_vertices + plane, (int)s);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- word offsets
__global__ __launch_bounds__(WT) void ct_rowscan_kernel(const CtP p) {
  __shared__ unsigned part[WT];
  const int pl = blockIdx.x, tid = threadIdx.x;
  const size_t plane = (size_t)(p.plane0 + pl);
  const unsigned words = (unsigned)(p.H + 1) * (unsigned)p.nwv;
  unsigned* wo = p.wordoff + plane * words;
  const unsigned per = (words + WT - 1) / WT, i0 = min(words, tid * per), i1 = min(words, i0 + per);   // thread t owns the words i0 .. i1
  unsigned mine = 0u;
  for (unsigned i = i0; i < i1; ++i) mine += wo[i];
  part[tid] = mine;
  __syncthreads();
  unsigned before = 0u, total = 0u;
  for (int t = 0; t < WT; ++t) {
    const unsigned v = part[t];
    before += t < tid ? v : 0u;
    total += v;
  }
  for (unsigned i = i0; i < i1; ++i) {
    const unsigned v = wo[i];
    wo[i] = before;
    before += v;
  }
  if (tid == 0) {
    p.n_vertices[plane] = (int)total;
    p.nv[plane] = total <= (unsigned)p.V ? (int)total : 0;     // total <= 2 H W + 2, so nv <= Ve
  }
}

// ---------------------------------------------------------------------------------------------------------------- successors
// The far end of the straight run that leaves vertex (x, y) in direction D (0 E, 1 S, 2 W, 3 N).  Every loop is bounded by the words of a row
// or by H; the run ends inside the lattice because everything outside the plane is unset.
template <int D>
__device__ __forceinline__ void run_end(const u64* plane, const VMasks& m, int x, int y, int H, int W, int nw, int nwv, int& x2, int& y2) {
  const int wv = x >> 6, bit = x & 63;
  x2 = x; y2 = y;
  if (D == 0) {                                                 // the first vertex to the right that no E edge leaves
    u64 z = bit == 63 ? 0ull : ~m.oE & (~0ull << (bit + 1));
    int w2 = wv;
    while (!z && ++w2 < nwv) z = ~(row_word(plane, y, w2, H, W, nw) & ~row_word(plane, y - 1, w2, H, W, nw));
    x2 = z ? w2 * 64 + __ffsll((long long)z) - 1 : W;
  } else if (D == 2) {                                          // the first vertex to the left that no W edge leaves
    u64 z = ~m.oW & ((1ull << bit) - 1ull);
    int w2 = wv;
    while (!z && --w2 >= 0) {
      const u64 upc = row_word(plane, y - 1, w2, H, W, nw), upl = row_word(plane, y - 1, w2 - 1, H, W, nw);
      const u64 dnc = row_word(plane, y, w2, H, W, nw), dnl = row_word(plane, y, w2 - 1, H, W, nw);
      z = ~(((upc << 1) | (upl >> 63)) & ~((dnc << 1) | (dnl >> 63)));
    }
    x2 = z ? w2 * 64 + 63 - __clzll((long long)z) : 0;
  } else if (D == 1) {                                          // down while pixel (x - 1, y2) is set and (x, y2) is not
    // (one row a step: most runs are a row or two long, and a step of four rows with eight loads in flight measured SLOWER)
    for (y2 = y + 1; y2 < H; ++y2)
      if (!(pixel(plane, x - 1, y2, H, W, nw) & ~pixel(plane, x, y2, H, W, nw) & 1u)) break;
  } else {                                                      // up while pixel (x, y2 - 1) is set and (x - 1, y2 - 1) is not
    for (y2 = y - 1; y2 > 0; --y2)
      if (!(pixel(plane, x, y2 - 1, H, W, nw) & ~pixel(plane, x - 1, y2 - 1, H, W, nw) & 1u)) break;
  }
}

template <int D>
__device__ __forceinline__ void link_pass(const CtP& p, const u64* src, const unsigned* wo, size_t plane, const VMasks& m, int x, int y,
                                          unsigned idx) {
  int x2, y2;
  run_end<D>(src, m, x, y, p.H, p.W, p.nw, p.nwv, x2, y2);
  const int w2 = x2 >> 6, b2 = x2 & 63;
  const VMasks e = vertex_masks(src, y2, w2, p.H, p.W, p.nw);
  constexpr int R = (D + 1) & 3, L = (D + 3) & 3;
  const u64 outs[4] = {e.oE, e.oS, e.oW, e.oN};               // constant indices only: stays in registers
  const bool has_r = (outs[R] >> b2) & 1ull, has_l = (outs[L] >> b2) & 1ull;
  const int nd = has_r && has_l ? (p.conn8 ? L : R) : (has_r ? R : L);    // a saddle: 4 turns right, 8 turns left
  const unsigned here = (unsigned)((e.pE >> b2) & 1ull) | (unsigned)((e.pS >> b2) & 1ull) << 1 | (unsigned)((e.pW >> b2) & 1ull) << 2 |
                        (unsigned)((e.pN >> b2) & 1ull) << 3;
  const unsigned q = wo[(size_t)y2 * p.nwv + w2] + passes_below(e, b2) + (unsigned)__popc(here & ((1u << nd) - 1u));
  if (idx < (unsigned)p.Ve) {
    p.key[plane * p.Ve + idx] = (unsigned)(y * (p.W + 1) + x) | (unsigned)D << 30;
    p.nxt0[plane * p.Ve + idx] = (int)q;
  }
}

__global__ __launch_bounds__(WT) void ct_link_kernel(const CtP p) {
  const int lane = threadIdx.x & 63, pl = blockIdx.z;
  const size_t plane = (size_t)(p.plane0 + pl);
  if (p.nv[plane] == 0) return;                                // an empty plane, or one that does not fit V
  const u64* src = p.src + plane * p.H * p.nw;
  const unsigned words = (unsigned)(p.H + 1) * (unsigned)p.nwv;
  const unsigned* wo = p.wordoff + plane * words;
  for (int s = 0; s < WORDS_PER_WAVE; ++s) {
    const unsigned t = (blockIdx.x * WW + (threadIdx.x >> 6)) * WORDS_PER_WAVE + (unsigned)s;
    if (t >= words) return;
    const int y = (int)(t / (unsigned)p.nwv), wv = (int)(t - (unsigned)y * (unsigned)p.nwv);
    const VMasks m = vertex_masks(src, y, wv, p.H, p.W, p.nw);
    if (!(m.pE | m.pS | m.pW | m.pN)) continue;
    unsigned idx = wo[t] + passes_below(m, lane);
    const int x = wv * 64 + lane;
    if ((m.pE >> lane) & 1ull) link_pass<0>(p, src, wo, plane, m, x, y, idx++);
    if ((m.pS >> lane) & 1ull) link_pass<1>(p, src, wo, plane, m, x, y, idx++);
    if ((m.pW >> lane) & 1ull) link_pass<2>(p, src, wo, plane, m, x, y, idx++);
    if ((m.pN >> lane) & 1ull) link_pass<3>(p, src, wo, plane, m, x, y, idx++);
  }
}

// ---------------------------------------------------------------------------------------------------------------- pointer jumping
__device__ __forceinline__ u64 first_pair(unsigned key, unsigned i) {   // the window [i, i + 1): an E pass is a candidate start
  return (u64)((key >> 30) == 0u ? i : NONE) << 32;
}

// Round k: pair[i] covers the window [i, i + 2^k) of the cycle and nxt[i] is the pass 2^k further on.  The smaller start wins; among equal
// starts (the window has gone round the cycle) the first occurrence, so the distance stays below the cycle's length.
template <bool FIRST>
__global__ __launch_bounds__(WT) void ct_jump_kernel(const CtP p, const int* nxt_s, const u64* md_s, int* nxt_d, u64* md_d, unsigned span) {
  const size_t plane = (size_t)(p.plane0 + blockIdx.z), base = plane * p.Ve;
  const unsigned nv = (unsigned)p.nv[plane], i = blockIdx.x * WT + threadIdx.x;
  if (i >= nv) return;
  unsigned q = (unsigned)nxt_s[base + i];
  if (q >= nv) q = i;                                          // never taken: successors are pass numbers of this plane
  u64 a = FIRST ? first_pair(p.key[base + i], i) : md_s[base + i];
  const u64 b = FIRST ? first_pair(p.key[base + q], q) : md_s[base + q];
  if ((unsigned)(b >> 32) < (unsigned)(a >> 32)) a = b + span;
  md_d[base + i] = a;
  nxt_d[base + i] = nxt_s[base + q];
}

// ---------------------------------------------------------------------------------------------------------------- contours
// (is a start, vertices of its contour) of pass i: the start's successor is the pass furthest from the start.
__device__ __forceinline__ uint2 start_item(const CtP& p, const u64* md, size_t base, unsigned i, unsigned nv) {
  if (i >= nv || (unsigned)(md[base + i] >> 32) != i) return make_uint2(0u, 0u);
  unsigned q = (unsigned)p.nxt0[base + i];
  if (q >= nv) q = i;
  return make_uint2(1u, (unsigned)md[base + q] + 1u);
}

__global__ __launch_bounds__(WT) void ct_tilesum_kernel(const CtP p, const u64* md) {
  __shared__ unsigned red[2 * WW];
  const size_t plane = (size_t)(p.plane0 + blockIdx.z), base = plane * p.Ve;
  const unsigned nv = (unsigned)p.nv[plane], i0 = blockIdx.x * TILE + threadIdx.x * ITEMS;
  unsigned f = 0u, c = 0u;
  for (int j = 0; j < ITEMS; ++j) {
    const uint2 it = start_item(p, md, base, i0 + j, nv);
    f += it.x; c += it.y;
  }
  f = wave_sum_u32(f); c = wave_sum_u32(c);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = f; red[WW + (threadIdx.x >> 6)] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    f = 0u; c = 0u;
#pragma unroll
    for (int w = 0; w < WW; ++w) { f += red[w]; c += red[WW + w]; }
    p.tsum[plane * p.ntiles + blockIdx.x] = make_uint2(f, c);
  }
}

__global__ __launch_bounds__(WT) void ct_tilescan_kernel(const CtP p) {
  __shared__ unsigned part[WT];
  const int tid = threadIdx.x, nt = p.ntiles, C = p.C;
  const size_t plane = (size_t)(p.plane0 + blockIdx.x);
  uint2* ts = p.tsum + plane * nt;
  const int per = (nt + WT - 1) / WT, t0 = min(nt, tid * per), t1 = min(nt, t0 + per);
  unsigned f = 0u, c = 0u;
  for (int t = t0; t < t1; ++t) { f += ts[t].x; c += ts[t].y; }
  unsigned fb = 0u, cb = 0u, ftot = 0u;
  part[tid] = f;
  __syncthreads();
  for (int t = 0; t < WT; ++t) { fb += t < tid ? part[t] : 0u; ftot += part[t]; }
  __syncthreads();
  part[tid] = c;
  __syncthreads();
  for (int t = 0; t < WT; ++t) cb += t < tid ? part[t] : 0u;
  for (int t = t0; t < t1; ++t) {
    const uint2 v = ts[t];
    ts[t] = make_uint2(fb, cb);
    fb += v.x; cb += v.y;
  }
  const bool over = (unsigned)p.n_vertices[plane] > (unsigned)p.V;
  if (tid == 0) p.n_contours[plane] = over ? -1 : (int)ftot;
  for (unsigned j = min(ftot, (unsigned)C) + tid; j < (unsigned)C; j += WT) {   // the rows no contour owns (all of them when the plane does not fit)
    const size_t r = plane * C + j;
    p.offset[r] = 0; p.count[r] = 0; p.area2[r] = 0ull; p.start[r] = 0;
    p.box[r * 4 + 0] = 0; p.box[r * 4 + 1] = 0; p.box[r * 4 + 2] = 0; p.box[r * 4 + 3] = 0;
  }
}

__global__ __launch_bounds__(WT) void ct_starts_kernel(const CtP p, const u64* md, int* cidx_out, u64* lo_out) {
  __shared__ unsigned pf[WT], pc[WT];
  const int tid = threadIdx.x;
  const size_t plane = (size_t)(p.plane0 + blockIdx.z), base = plane * p.Ve;
  const unsigned nv = (unsigned)p.nv[plane], i0 = blockIdx.x * TILE + tid * ITEMS;
  uint2 it[ITEMS];
  unsigned f = 0u, c = 0u;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    it[j] = start_item(p, md, base, i0 + j, nv);
    f += it[j].x; c += it[j].y;
  }
  pf[tid] = f; pc[tid] = c;
  __syncthreads();
  const uint2 tb = p.tsum[plane * p.ntiles + blockIdx.x];
  unsigned fb = tb.x, cb = tb.y;
  if (f) {                                                     // only a thread that holds a start needs its prefix
    for (int t = 0; t < tid; ++t) { fb += pf[t]; cb += pc[t]; }
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      if (it[j].x) {
        const unsigned i = i0 + j;
        cidx_out[base + i] = (int)fb;
        lo_out[base + i] = (u64)it[j].y << 32 | cb;
        if (fb < (unsigned)p.C) {
          const size_t r = plane * p.C + fb;
          p.offset[r] = (int)cb; p.count[r] = (int)it[j].y; p.area2[r] = 0ull; p.start[r] = (int)(p.key[base + i] & KEY_MASK);
          p.box[r * 4 + 0] = p.W; p.box[r * 4 + 1] = p.H; p.box[r * 4 + 2] = 0; p.box[r * 4 + 3] = 0;
        }
        fb += 1u; cb += it[j].y;
      }
    }
  }
}

__global__ __launch_bounds__(WT) void ct_scatter_kernel(const CtP p, const u64* md, const int* cidx_in, const u64* lo_in) {
  const size_t plane = (size_t)(p.plane0 + blockIdx.z), base = plane * p.Ve;
  const unsigned nv = (unsigned)p.nv[plane], i = blockIdx.x * WT + threadIdx.x;
  if (i >= nv) return;
  const u64 a = md[base + i];
  unsigned s = (unsigned)(a >> 32), q = (unsigned)p.nxt0[base + i];
  const unsigned d = (unsigned)a;
  if (s >= nv) s = i;                                          // never taken: every cycle holds an E pass
  if (q >= nv) q = i;
  const u64 lo = lo_in[base + s];
  const unsigned len = (unsigned)(lo >> 32), pos = (unsigned)lo + (d ? len - d : 0u), w1 = (unsigned)p.W + 1u;
  const unsigned k = p.key[base + i] & KEY_MASK, kn = p.key[base + q] & KEY_MASK;
  const int y = (int)(k / w1), x = (int)(k - (unsigned)y * w1), yn = (int)(kn / w1), xn = (int)(kn - (unsigned)yn * w1);
  if (pos < nv) {                                              // two 4-byte stores: `vertices` is only 4-byte aligned
    int* v = p.vertices + (plane * p.V + pos) * 2;
    v[0] = x; v[1] = y;
  }
  const unsigned ci = (unsigned)cidx_in[base + s];
  if (ci < (unsigned)p.C) {
    const size_t r = plane * p.C + ci;
    // sum(x_i y_{i+1} - x_{i+1} y_i) = -2 * (integral of y dx) = sum over the HORIZONTAL edges of 2 y (x_i - x_{i+1}): a vertical edge adds nothing to
    // it, so only the E and W passes touch the word, and none of them on the row y = 0.  Two's complement: the sum is the signed one.
    if (y == yn && y != 0) atomicAdd(p.area2 + r, (u64)(2ll * y * (x - xn)));
    // A bound only moves one way: a pass whose coordinate the word already covers skips the atomic (a stale read can only make it issue one).
    int* box = p.box + r * 4;
    if (x < __hip_atomic_load(box + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(box + 0, x);
    if (y < __hip_atomic_load(box + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(box + 1, y);
    if (x > __hip_atomic_load(box + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(box + 2, x);
    if (y > __hip_atomic_load(box + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(box + 3, y);
  }
}

// ---------------------------------------------------------------------------------------------------------------- run lengths
struct RleP {
  const u64* src;        // [n][H][nw]
  unsigned* cnt;         // [n][W * nbands]: transitions of (column, band), then the number of the first run the band opens
  int* last;             // [n][W * nbands]: position of its last transition (-1: none), then of the last transition before the band
  unsigned* counts; int* n_runs;
  int plane0, H, W, nw, nbands, R;
};

// One wave per (word column, band), lane = column: walks the band's rows.  WRITE = false counts, WRITE = true stores the differences.
template <bool WRITE>
__global__ __launch_bounds__(WT) void rle_walk_kernel(const RleP p) {
  const int lane = threadIdx.x & 63, w = blockIdx.x, band = blockIdx.y * WW + (threadIdx.x >> 6), H = p.H, nw = p.nw;
  if (band >= p.nbands) return;
  const size_t plane = (size_t)(p.plane0 + blockIdx.z);
  const u64* src = p.src + plane * H * nw;
  const int x = w * 64 + lane, y0 = band * BAND, y1 = min(H, y0 + BAND);
  const size_t item = plane * ((size_t)p.W * p.nbands) + (size_t)x * p.nbands + band;
  const u64 vb = valid_bits(w, p.W);
  u64 prev;                                                    // bit x: the pixel before (x, y0) in column-major order
  if (y0 == 0) {
    const u64 lc = src[(size_t)(H - 1) * nw + w] & vb, ll = w > 0 ? src[(size_t)(H - 1) * nw + w - 1] : 0ull;   // a word to the left has no padding
    prev = (lc << 1) | (ll >> 63);
  } else {
    prev = src[(size_t)(y0 - 1) * nw + w] & vb;
  }
  const bool live = x < p.W;                                   // a padding column owns no item and stores nothing
  unsigned k = 0u;
  int at = -1;
  if (WRITE && live) { k = p.cnt[item]; at = p.last[item]; }
  for (int y = y0; y < y1; ++y) {
    const u64 cur = src[(size_t)y * nw + w] & vb;
    if (live && (((cur ^ prev) >> lane) & 1ull)) {
      const int pos = x * H + y;
      if (WRITE) {
        if (k < (unsigned)p.R) p.counts[plane * p.R + k] = (unsigned)(pos - at);
      }
      at = pos;
      ++k;
    }
    prev = cur;
  }
  if (!WRITE && live) { p.cnt[item] = k; p.last[item] = at; }
}

__global__ __launch_bounds__(WT) void rle_scan_kernel(const RleP p) {
  __shared__ unsigned part[WT];
  __shared__ int lastp[WT];
  const int tid = threadIdx.x;
  const size_t plane = (size_t)(p.plane0 + blockIdx.x);
  const unsigned items = (unsigned)p.W * (unsigned)p.nbands;
  unsigned* cnt = p.cnt + plane * items;
  int* last = p.last + plane * items;
  const unsigned per = (items + WT - 1) / WT, i0 = min(items, tid * per), i1 = min(items, i0 + per);
  unsigned mine = 0u;
  int mlast = 0;                                               // positions grow with the item: the last one seen is the largest
  for (unsigned i = i0; i < i1; ++i) { mine += cnt[i]; mlast = max(mlast, last[i]); }
  part[tid] = mine; lastp[tid] = mlast;
  __syncthreads();
  unsigned before = 0u, total = 0u;
  int lbefore = 0, lall = 0;                                   // no transition yet: the first run starts at position 0
  for (int t = 0; t < WT; ++t) {
    before += t < tid ? part[t] : 0u;
    total += part[t];
    lbefore = t < tid ? max(lbefore, lastp[t]) : lbefore;
    lall = max(lall, lastp[t]);
  }
  for (unsigned i = i0; i < i1; ++i) {
    const unsigned v = cnt[i];
    const int l = last[i];
    cnt[i] = before; last[i] = lbefore;
    before += v; lbefore = max(lbefore, l);
  }
  if (tid == 0) {
    p.n_runs[plane] = (int)total + 1;
    if (p.counts && total < (unsigned)p.R) p.counts[plane * p.R + total] = (unsigned)(p.H * p.W - lall);   // the run that reaches the end
  }
}

bool shape_ok(int n, int H, int W) { return n >= 0 && plane_dims_ok(H, W); }

int rounds_for(int64_t Ve) {                                   // the smallest K >= 1 with 2^K >= Ve: a window as long as the longest cycle
  int k = 1;
  while (((int64_t)1 << k) < Ve) ++k;
  return k;
}

int64_t rle_items(int H, int W) { return (int64_t)W * ((H + BAND - 1) / BAND); }

}  // namespace

extern "C" int mtbt_sizeof_contours_args(int which) {
  return which == 0 ? (int)sizeof(mtbt_contours_args) : (which == 1 ? (int)sizeof(mtbt_rle_args) : -1);
}

extern "C" int64_t mtbt_contours_workspace_bytes(int n, int H, int W, int max_vertices) {
  if (!shape_ok(n, H, W) || max_vertices < 0) return MTBT_EINVAL;
  if (n == 0) return 0;
  return layout_of(n, H, W, max_vertices).total;
}

extern "C" int mtbt_trace_contours(const mtbt_contours_args* args, void* stream) {
  if (!args) return MTBT_EINVAL;
  const mtbt_contours_args& a = *args;
  if (!shape_ok(a.n, a.H, a.W) || !plane_pitch_ok(a.W, a.pitch)) return MTBT_EINVAL;
  if ((a.connectivity != 4 && a.connectivity != 8) || !a.packed || !a.n_vertices) return MTBT_EINVAL;
  const bool count_only = !a.vertices && !a.offset && !a.count && !a.area2 && !a.box && !a.start;
  if (!count_only) {
    if (!a.vertices || !a.n_contours || !a.offset || !a.count || !a.area2 || !a.box || !a.start) return MTBT_EINVAL;
    if (a.max_contours < 1 || a.max_contours > MAX_CONTOURS || a.max_vertices < 0) return MTBT_EINVAL;
    const int64_t need = mtbt_contours_workspace_bytes(a.n, a.H, a.W, a.max_vertices);
    if (a.workspace_bytes < need || (need > 0 && !a.workspace)) return MTBT_EINVAL;
    if (!aligned_n(a.workspace, 16) || !aligned_n(a.n_contours, 4) || !aligned_n(a.vertices, 4) || !aligned_n(a.offset, 4) ||
        !aligned_n(a.count, 4) || !aligned_n(a.area2, 8) || !aligned_n(a.box, 4) || !aligned_n(a.start, 4))
      return MTBT_EALIGN;
  }
  if (!aligned_n(a.packed, 8) || !aligned_n(a.n_vertices, 4)) return MTBT_EALIGN;
  if (a.n == 0) return MTBT_OK;

  CtP p = {};
  p.src = reinterpret_cast<const u64*>(a.packed);
  p.n_vertices = a.n_vertices;
  p.H = a.H; p.W = a.W; p.nw = (int)plane_words(a.W); p.nwv = a.W / 64 + 1; p.conn8 = a.connectivity == 8;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t words = (int64_t)(a.H + 1) * p.nwv;
  const unsigned gw = (unsigned)((words + WT - 1) / WT);
  if (count_only) {
    if (hipMemsetAsync(a.n_vertices, 0, (size_t)a.n * 4, s) != hipSuccess) return MTBT_ELAUNCH;
    for (int p0 = 0; p0 < a.n; p0 += CHUNK) {
      const unsigned c = (unsigned)(a.n - p0 < CHUNK ? a.n - p0 : CHUNK);
      p.plane0 = p0;
      hipLaunchKernelGGL(ct_count_kernel<true>, dim3(gw, 1, c), dim3(WT), 0, s, p);
      MTBT_LAUNCH_CHECK();
    }
    return MTBT_OK;
  }

  const Layout l = layout_of(a.n, a.H, a.W, a.max_vertices);
  unsigned char* ws = reinterpret_cast<unsigned char*>(a.workspace);
  p.wordoff = reinterpret_cast<unsigned*>(ws + l.wordoff);
  p.nv = reinterpret_cast<int*>(ws + l.nv);
  p.key = reinterpret_cast<unsigned*>(ws + l.key);
  p.nxt0 = reinterpret_cast<int*>(ws + l.nxt0);
  p.nxt_a = reinterpret_cast<int*>(ws + l.nxt_a);
  p.nxt_b = reinterpret_cast<int*>(ws + l.nxt_b);
  p.md_a = reinterpret_cast<u64*>(ws + l.md_a);
  p.md_b = reinterpret_cast<u64*>(ws + l.md_b);
  p.tsum = reinterpret_cast<uint2*>(ws + l.tsum);
  p.n_contours = a.n_contours; p.vertices = a.vertices; p.offset = a.offset; p.count = a.count;
  p.area2 = reinterpret_cast<u64*>(a.area2); p.box = a.box; p.start = a.start;
  p.C = a.max_contours; p.V = a.max_vertices;
  p.Ve = (int)pass_capacity(a.H, a.W, a.max_vertices);
  p.ntiles = (p.Ve + TILE - 1) / TILE;
  const int K = rounds_for(p.Ve);
  const unsigned gl = (unsigned)((words + WW * WORDS_PER_WAVE - 1) / (WW * WORDS_PER_WAVE));
  const unsigned gp = (unsigned)(((int64_t)p.Ve + WT - 1) / WT);
  for (int p0 = 0; p0 < a.n; p0 += CHUNK) {                    // the groups own disjoint slices of the workspace
    const unsigned c = (unsigned)(a.n - p0 < CHUNK ? a.n - p0 : CHUNK);
    p.plane0 = p0;
    hipLaunchKernelGGL(ct_count_kernel<false>, dim3(gw, 1, c), dim3(WT), 0, s, p);
    MTBT_LAUNCH_CHECK();
    hipLaunchKernelGGL(ct_rowscan_kernel, dim3(c), dim3(WT), 0, s, p);
    MTBT_LAUNCH_CHECK();
    const u64* md = p.md_a;                                    // where the last round leaves the pairs; the other pair of buffers is spare
    int* spare_i = p.nxt_b;
    u64* spare_l = p.md_b;
    if (p.Ve > 0) {
      hipLaunchKernelGGL(ct_link_kernel, dim3(gl, 1, c), dim3(WT), 0, s, p);
      MTBT_LAUNCH_CHECK();
      hipLaunchKernelGGL(ct_jump_kernel<true>, dim3(gp, 1, c), dim3(WT), 0, s, p, (const int*)p.nxt0, (const u64*)nullptr, p.nxt_a, p.md_a, 1u);
      MTBT_LAUNCH_CHECK();
      for (int k = 1; k < K; ++k) {
        const bool to_b = k & 1;
        hipLaunchKernelGGL(ct_jump_kernel<false>, dim3(gp, 1, c), dim3(WT), 0, s, p, (const int*)(to_b ? p.nxt_a : p.nxt_b),
                           (const u64*)(to_b ? p.md_a : p.md_b), to_b ? p.nxt_b : p.nxt_a, to_b ? p.md_b : p.md_a, 1u << k);
        MTBT_LAUNCH_CHECK();
      }
      if (!(K & 1)) { md = p.md_b; spare_i = p.nxt_a; spare_l = p.md_a; }
      hipLaunchKernelGGL(ct_tilesum_kernel, dim3((unsigned)p.ntiles, 1, c), dim3(WT), 0, s, p, md);
      MTBT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ct_tilescan_kernel, dim3(c), dim3(WT), 0, s, p);
    MTBT_LAUNCH_CHECK();
    if (p.Ve > 0) {
      hipLaunchKernelGGL(ct_starts_kernel, dim3((unsigned)p.ntiles, 1, c), dim3(WT), 0, s, p, md, spare_i, spare_l);
      MTBT_LAUNCH_CHECK();
      hipLaunchKernelGGL(ct_scatter_kernel, dim3(gp, 1, c), dim3(WT), 0, s, p, md, (const int*)spare_i, (const u64*)spare_l);
      MTBT_LAUNCH_CHECK();
    }
  }
  return MTBT_OK;
}

extern "C" int64_t mtbt_rle_workspace_bytes(int n, int H, int W) {
  if (!shape_ok(n, H, W)) return MTBT_EINVAL;
  if (n == 0) return 0;
  return 2 * up16((int64_t)n * rle_items(H, W) * 4);
}

extern "C" int mtbt_rle_encode(const mtbt_rle_args* args, void* stream) {
  if (!args) return MTBT_EINVAL;
  const mtbt_rle_args& a = *args;
  if (!shape_ok(a.n, a.H, a.W) || !plane_pitch_ok(a.W, a.pitch)) return MTBT_EINVAL;
  if (!a.packed || !a.n_runs || (a.counts && a.max_runs < 0)) return MTBT_EINVAL;
  const int64_t need = mtbt_rle_workspace_bytes(a.n, a.H, a.W);
  if (a.workspace_bytes < need || (need > 0 && !a.workspace)) return MTBT_EINVAL;
  if (!aligned_n(a.packed, 8) || !aligned_n(a.workspace, 16) || !aligned_n(a.counts, 4) || !aligned_n(a.n_runs, 4)) return MTBT_EALIGN;
  if (a.n == 0) return MTBT_OK;

  RleP p = {};
  p.src = reinterpret_cast<const u64*>(a.packed);
  p.cnt = reinterpret_cast<unsigned*>(a.workspace);
  p.last = reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(a.workspace) + need / 2);
  p.counts = a.counts; p.n_runs = a.n_runs;
  p.H = a.H; p.W = a.W; p.nw = (int)plane_words(a.W); p.nbands = (a.H + BAND - 1) / BAND; p.R = a.counts ? a.max_runs : 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)p.nw, (unsigned)((p.nbands + WW - 1) / WW), 1);
  for (int p0 = 0; p0 < a.n; p0 += CHUNK) {
    const unsigned c = (unsigned)(a.n - p0 < CHUNK ? a.n - p0 : CHUNK);
    p.plane0 = p0;
    hipLaunchKernelGGL(rle_walk_kernel<false>, dim3(grid.x, grid.y, c), dim3(WT), 0, s, p);
    MTBT_LAUNCH_CHECK();
    hipLaunchKernelGGL(rle_scan_kernel, dim3(c), dim3(WT), 0, s, p);
    MTBT_LAUNCH_CHECK();
    if (a.counts && a.max_runs > 0) {
      hipLaunchKernelGGL(rle_walk_kernel<true>, dim3(grid.x, grid.y, c), dim3(WT), 0, s, p);
      MTBT_LAUNCH_CHECK();
    }
  }
  return MTBT_OK;
}
