// Connected components of bit-packed planes: mtbt_label_components and mtbt_select_components (contract in include/mtbt_hip.h), feeding
// `postprocess.label_components` / `filter_components` / `components_to_instances` and `metrics.LesionMetrics`.
//
// Packed layout as in mask_eval.hip / surface_dist.hip: a plane is H rows of pitch = 8 * ceil(W / 64) bytes, pixel X is bit X & 7 of
// byte X >> 3, planes are 8-byte aligned and every access to one is an 8-byte load.  Bits X >= W are masked off where a row word is read.
//
// Union-find by minimum index (Komura 2015; Playne & Hawick 2018) on the RUNS of set bits inside a 64-bit word: a pixel's node is the
// first pixel of its run within its word, a node's name is its flat index y * W + x, and parent[v] <= v always.  The root of a component
// is therefore its smallest flat index -- its first pixel in row-major order, which always starts a run -- whatever the order the
// unions ran in: every output is a pure function of the input.  Horizontal links inside a word cost nothing (they ARE the run);
// vertical, diagonal and word-crossing links are unions.  Ids are a prefix sum over the root flags in row-major order: no atomics
// there.  Integer atomics (min on parent; add / min / max on the records) cannot show their order.  No workgroup waits on another:
// the phases are kernels on the stream.
//
// Every "word" kernel runs one wave per 64-bit row word (lane = pixel column), WORDS_PER_WAVE consecutive words per wave, four waves
// per workgroup, grid (ceil(H * words_x / 32), 1, planes of the launch group): 16 planes of 640 x 640 are 3200 workgroups.
//
// cc_init_kernel     word kernel.  parent[v] = v for every run start.  Bound: one 8-byte load per wave and scattered 4-byte stores.
// cc_union_kernel    word kernel.  A lane whose pixel is set links its node to the node above (skipped when the lane to its left makes
//                    the same link), under 8-connectivity to the nodes above-left / above-right when the pixel straight above is
//                    unset (and the neighbour lane has no vertical link of its own), and lane 0 to the last run of the word to its
//                    left.  find = a chase of dependent agent-scope loads, union = atomicMin on a root.  Bound: the latency of those
//                    dependent chases (an L2 round trip per hop) times the depth of the trees; divergent.
// cc_roots_kernel    word kernel.  Root flags (parent[v] == v) as one ballot word per row word.  Bound: one 4-byte load per run.
// cc_scan_kernel     one workgroup per plane: popcounts of the root rows -> exclusive row offsets and n_components (as
//                    surface_scan_kernel), and the zeros of the record rows beyond n_components.
// cc_number_kernel   word kernel.  id of a root = row offset + roots before it in its row + 1; parent[root] = -id; the root's rows of the
//                    record tables start here (area 0, first, the box's y1 = first / W and the neutral elements of min / max).
// cc_label_kernel    word kernel.  A run start chases to its root (plain loads now: the unions ended at a kernel boundary), reads the id,
//                    leaves parent[v] = root for the next reader, and adds its run to the records with one atomic per field; the run's
//                    lanes take the id by a shuffle and store the label row (256 contiguous bytes per wave).  Bound: the chase latency,
//                    then the label stores (4 bytes per pixel).
// cc_choose_kernel   one workgroup per plane over the per-id areas: the k-th largest by the bitwise count search of
//                    surface_select_kernel (at most 31 passes), ties to the lower id by a prefix over the ids, the keep flag into bit 31
//                    of the area word, n_kept.
// cc_write_kernel    word kernel.  run start -> root -> id -> keep flag, a ballot per word, lane 0 stores the 8 bytes (padding zero).
#include "bitplane.h"

namespace {

constexpr int WT = 256;                   // threads of every workgroup here
constexpr int WW = WT / 64;               // waves per workgroup
constexpr int WORDS_PER_WAVE = 8;
constexpr int MAX_COMPONENTS = 65536;
constexpr unsigned KEEP = 0x80000000u;    // keep flag in the per-id area word (an area is below 2^31)

struct Layout {   // byte offsets of the sections of the workspace (all n planes), each 16-byte aligned
  int64_t parent, area, roots, rowoff, tot, total;
};

int64_t max_ids(int64_t H, int64_t W) { return (H * W + 1) / 2; }   // a checkerboard under 4-connectivity

Layout layout_of(int64_t n, int64_t H, int64_t W) {
  const int64_t nw = plane_words(W);
  Layout l;
  int64_t off = 0;
  l.parent = off; off = up16(off + n * H * W * 4);
  l.area = off;   off = up16(off + n * max_ids(H, W) * 4);
  l.roots = off;  off = up16(off + n * H * nw * 8);
  l.rowoff = off; off = up16(off + n * H * 4);
  l.tot = off;    off = up16(off + n * 4);
  l.total = off;
  return l;
}

struct CompP {
  const u64* src;       // [n][H][words_x]
  const u64* other;     // [n][H][words_x] or null
  int* parent;          // [n][H * W]: run starts only.  While the unions run: parent[v] <= v; after cc_number_kernel: -id at a root, else an ancestor
  unsigned* area_id;    // [n][max_ids]: area of id i at [i - 1]; bit 31 is the keep flag of the last mtbt_select_components
  u64* roots;           // [n][H][words_x]
  unsigned* rowoff;     // [n][H]
  unsigned* tot;        // [n]
  int* labels;          // [n][H][W] or null
  int* n_components;    // [n]
  unsigned* area;       // [n][C]
  int* box;             // [n][C][4]
  int* first;           // [n][C]
  unsigned* inter;      // [n][C] or null
  u64* out;             // select: [n][H][words_x]
  int* n_kept;          // select: [n]
  int plane0, H, W, words_x, conn8, C;
  unsigned ids_per_plane, min_area, keep_largest;
};

// first bit of the run of set bits of m that holds bit x (bit x is set)
__device__ __forceinline__ int run_start(u64 m, int x) {
  const u64 gaps = ~m & ((1ull << x) - 1ull);
  return gaps ? 64 - __clzll((long long)gaps) : 0;
}

__device__ __forceinline__ int ld_parent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int cc_find(const int* parent, int v) {
  // Terminates: parent[u] <= u for every node at every moment (set to u, then only lowered by atomicMin), so each step moves to a strictly
  // smaller index and a value read late is still an ancestor.
  int p = ld_parent(parent + v);
  while (p != v) {
    v = p;
    p = ld_parent(parent + v);
  }
  return v;
}

__device__ __forceinline__ void cc_union(int* parent, int a0, int b0) {
  int a = a0, b = b0;
  // Terminates: a parent value only ever decreases.  Each pass either ends or replaces the larger of (a, b) by a strictly smaller index
  // (old < a), and both are bounded below by 0.
  for (;;) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) break;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);      // a > b
    if (old == a) { a = b; break; }                // a was a root and now hangs under b
    a = old;                                       // a had a parent already: parent[a] = min(old, b), and old and b are still to be joined
  }
  if (a < a0) atomicMin(parent + a0, a);           // shorten the two paths just walked: a is an ancestor of both
  if (a < b0) atomicMin(parent + b0, a);
}

// the word task of this wave and step: false when past the end
__device__ __forceinline__ bool word_task(const CompP& p, int step, int& y, int& w) {
  const unsigned t = (blockIdx.x * WW + (threadIdx.x >> 6)) * WORDS_PER_WAVE + (unsigned)step;
  if (t >= (unsigned)p.H * (unsigned)p.words_x) return false;
  y = (int)(t / (unsigned)p.words_x);
  w = (int)(t - (unsigned)y * (unsigned)p.words_x);
  return true;
}

// ---------------------------------------------------------------------------------------------------------------- init
__global__ __launch_bounds__(WT) void cc_init_kernel(const CompP p) {
  const int lane = threadIdx.x & 63, pl = blockIdx.z, nw = p.words_x;
  const u64* src = p.src + (size_t)(p.plane0 + pl) * p.H * nw;
  int* parent = p.parent + (size_t)(p.plane0 + pl) * p.H * p.W;
  for (int s = 0; s < WORDS_PER_WAVE; ++s) {
    int y, w;
    if (!word_task(p, s, y, w)) return;
    const u64 m = src[(size_t)y * nw + w] & valid_bits(w, p.W);
    if (((m & ~(m << 1)) >> lane) & 1ull) {
      const int v = y * p.W + w * 64 + lane;
      parent[v] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- union
__global__ __launch_bounds__(WT) void cc_union_kernel(const CompP p) {
  const int lane = threadIdx.x & 63, pl = blockIdx.z, nw = p.words_x, W = p.W;
  const u64* src = p.src + (size_t)(p.plane0 + pl) * p.H * nw;
  int* parent = p.parent + (size_t)(p.plane0 + pl) * p.H * W;
  for (int s = 0; s < WORDS_PER_WAVE; ++s) {
    int y, w;
    if (!word_task(p, s, y, w)) return;
    const u64* row = src + (size_t)y * nw;
    const u64 m = row[w] & valid_bits(w, W);
    if (!((m >> lane) & 1ull)) continue;
    const int me = y * W + w * 64 + run_start(m, lane);
    if (lane == 0 && w > 0) {                                  // the word to the left has no padding bits
      const u64 l = row[w - 1];
      if (l >> 63) cc_union(parent, me, y * W + (w - 1) * 64 + run_start(l, 63));
    }
    if (y == 0) continue;
    const u64* above = row - nw;
    const u64 up = above[w] & valid_bits(w, W);
    const int base_up = (y - 1) * W + w * 64;
    const u64 both = m & up;
    if ((up >> lane) & 1ull) {
      if (!(((both << 1) >> lane) & 1ull)) cc_union(parent, me, base_up + run_start(up, lane));   // else the lane to the left links the same two runs
    } else if (p.conn8) {                                      // straight above is unset: the diagonals are two different runs
      const u64 ul = w > 0 ? above[w - 1] : 0ull;
      const u64 ur = w + 1 < nw ? above[w + 1] & valid_bits(w + 1, W) : 0ull;
      const u64 upl = (up << 1) | (ul >> 63), upr = (up >> 1) | (ur << 63);   // bit x: the pixel above-left / above-right of x
      if (((upl & ~(m << 1)) >> lane) & 1ull)                  // not when the pixel to my left is set: it lies below that one, in my run
        cc_union(parent, me, lane ? base_up + run_start(up, lane - 1) : base_up - 64 + run_start(ul, 63));
      if (((upr & ~(m >> 1)) >> lane) & 1ull)                  // likewise on the right
        cc_union(parent, me, lane < 63 ? base_up + run_start(up, lane + 1) : base_up + 64);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- root flags
__global__ __launch_bounds__(WT) void cc_roots_kernel(const CompP p) {
  const int lane = threadIdx.x & 63, pl = blockIdx.z, nw = p.words_x;
  const u64* src = p.src + (size_t)(p.plane0 + pl) * p.H * nw;
  const int* parent = p.parent + (size_t)(p.plane0 + pl) * p.H * p.W;
  u64* roots = p.roots + (size_t)(p.plane0 + pl) * p.H * nw;
  for (int s = 0; s < WORDS_PER_WAVE; ++s) {
    int y, w;
    if (!word_task(p, s, y, w)) return;
    const u64 m = src[(size_t)y * nw + w] & valid_bits(w, p.W);
    bool root = false;
    if (((m & ~(m << 1)) >> lane) & 1ull) {
      const int v = y * p.W + w * 64 + lane;
      root = parent[v] == v;
    }
    const u64 r = __ballot(root);
    if (lane == 0) roots[(size_t)y * nw + w] = r;
  }
}

// ---------------------------------------------------------------------------------------------------------------- row offsets
__global__ __launch_bounds__(WT) void cc_scan_kernel(const CompP p) {
  __shared__ unsigned part[WT];
  const int pl = blockIdx.x, tid = threadIdx.x, H = p.H, nw = p.words_x, C = p.C;
  const size_t plane = (size_t)(p.plane0 + pl);
  const u64* roots = p.roots + plane * H * nw;
  unsigned* rowoff = p.rowoff + plane * H;
  const int per = (H + WT - 1) / WT, y0 = min(H, tid * per), y1 = min(H, y0 + per);   // thread t owns rows y0 .. y1
  unsigned mine = 0u;
  for (int y = y0; y < y1; ++y)
    for (int w = 0; w < nw; ++w) mine += (unsigned)__popcll(roots[(size_t)y * nw + w]);
  part[tid] = mine;
  __syncthreads();
  unsigned before = 0u, total = 0u;
  for (int t = 0; t < WT; ++t) {
    const unsigned v = part[t];
    before += t < tid ? v : 0u;
    total += v;
  }
  for (int y = y0; y < y1; ++y) {
    rowoff[y] = before;
    for (int w = 0; w < nw; ++w) before += (unsigned)__popcll(roots[(size_t)y * nw + w]);
  }
  if (tid == 0) {
    p.tot[plane] = total;
    p.n_components[plane] = (int)total;
  }
  for (unsigned j = min(total, (unsigned)C) + tid; j < (unsigned)C; j += WT) {          // the rows no component owns
    const size_t r = plane * C + j;
    p.area[r] = 0u;
    p.first[r] = 0;
    p.box[r * 4 + 0] = 0; p.box[r * 4 + 1] = 0; p.box[r * 4 + 2] = 0; p.box[r * 4 + 3] = 0;
    if (p.inter) p.inter[r] = 0u;
  }
}

// ---------------------------------------------------------------------------------------------------------------- ids
__global__ __launch_bounds__(WT) void cc_number_kernel(const CompP p) {
  const int lane = threadIdx.x & 63, pl = blockIdx.z, nw = p.words_x, W = p.W;
  const size_t plane = (size_t)(p.plane0 + pl);
  const u64* roots = p.roots + plane * p.H * nw;
  int* parent = p.parent + plane * p.H * W;
  unsigned* area_id = p.area_id + plane * p.ids_per_plane;
  for (int s = 0; s < WORDS_PER_WAVE; ++s) {
    int y, w;
    if (!word_task(p, s, y, w)) return;
    const u64 r = roots[(size_t)y * nw + w];
    if (r == 0ull) continue;
    unsigned before = p.rowoff[plane * p.H + y];
    for (int j = 0; j < w; ++j) before += (unsigned)__popcll(roots[(size_t)y * nw + j]);
    if ((r >> lane) & 1ull) {
      const unsigned id = before + (unsigned)__popcll(r & ((1ull << lane) - 1ull)) + 1u;
      const int v = y * W + w * 64 + lane;
      parent[v] = -(int)id;
      area_id[id - 1u] = 0u;
      if (id <= (unsigned)p.C) {
        const size_t row = plane * p.C + (id - 1u);
        p.area[row] = 0u;
        p.first[row] = v;
        p.box[row * 4 + 0] = W; p.box[row * 4 + 1] = y; p.box[row * 4 + 2] = 0; p.box[row * 4 + 3] = 0;   // y1 = the first pixel's row
        if (p.inter) p.inter[row] = 0u;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- labels + records
__global__ __launch_bounds__(WT) void cc_label_kernel(const CompP p) {
  const int lane = threadIdx.x & 63, pl = blockIdx.z, nw = p.words_x, W = p.W;
  const size_t plane = (size_t)(p.plane0 + pl);
  const u64* src = p.src + plane * p.H * nw;
  const u64* other = p.other ? p.other + plane * p.H * nw : nullptr;
  int* parent = p.parent + plane * p.H * W;
  unsigned* area_id = p.area_id + plane * p.ids_per_plane;
  int* labels = p.labels ? p.labels + plane * p.H * W : nullptr;
  for (int s = 0; s < WORDS_PER_WAVE; ++s) {
    int y, w;
    if (!word_task(p, s, y, w)) return;
    const u64 vb = valid_bits(w, W), m = src[(size_t)y * nw + w] & vb;
    const bool set = (m >> lane) & 1ull;
    const int start = set ? run_start(m, lane) : lane;
    int id = 0;
    if (set && start == lane) {
      const int me = y * W + w * 64 + lane;
      int v = me, q = parent[v];
      // Terminates: a node that is not a root holds an ancestor's index, strictly below its own; a root holds -id.
      while (q >= 0) {
        v = q;
        q = parent[v];
      }
      id = -q;
      if (v != me) parent[me] = v;                             // a racing reader sees the old ancestor or the root: both lead to -id
      const u64 gaps = ~m & (~0ull << lane);                   // the run is [lane, end)
      const int end = gaps ? __ffsll((long long)gaps) - 1 : 64;
      const unsigned len = (unsigned)(end - lane);
      atomicAdd(area_id + (id - 1), len);
      if (id <= p.C) {
        const size_t row = plane * p.C + (size_t)(id - 1);
        atomicAdd(p.area + row, len);
        atomicMin(p.box + row * 4 + 0, w * 64 + lane);
        atomicMax(p.box + row * 4 + 2, w * 64 + end);
        atomicMax(p.box + row * 4 + 3, y + 1);
        if (other) {
          const u64 run = (end == 64 ? ~0ull : (1ull << end) - 1ull) & (~0ull << lane);
          const unsigned c = (unsigned)__popcll(other[(size_t)y * nw + w] & run);   // run lies inside the valid bits
          if (c) atomicAdd(p.inter + row, c);
        }
      }
    }
    id = __shfl(id, start, 64);
    if (labels && w * 64 + lane < W) labels[(size_t)y * W + w * 64 + lane] = set ? id : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------- select
__global__ __launch_bounds__(WT) void cc_choose_kernel(const CompP p) {
  __shared__ unsigned red[WW];
  const int pl = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t plane = (size_t)(p.plane0 + pl);
  unsigned* list = p.area_id + plane * p.ids_per_plane;
  const unsigned m = p.tot[plane], k = p.keep_largest;
  const bool ranked = k > 0u && k < m;                         // otherwise every component is among the k largest

  unsigned T = 0u, allow = 0u;
  if (ranked) {
    unsigned mx = 0u;
    for (unsigned i = tid; i < m; i += WT) mx = max(mx, list[i] & ~KEEP);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor(mx, o, 64));    __syncthreads();
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = max(max(red[0], red[1]), max(red[2], red[3]));
    // the k-th largest area = the item at ascending rank m - k: the largest T with count(list < T) <= m - k.  At most 31 passes.
    for (int b = 31 - __clz(mx | 1u); b >= 0; --b) {
      const unsigned t = T | (1u << b);
      unsigned c = 0u;
      for (unsigned i = tid; i < m; i += WT) c += (list[i] & ~KEEP) < t ? 1u : 0u;
      if (block_sum_u32<WW>(c, red, lane, wave) <= m - k) T = t;
    }
    unsigned above = 0u;
    for (unsigned i = tid; i < m; i += WT) above += (list[i] & ~KEEP) > T ? 1u : 0u;
    allow = k - block_sum_u32<WW>(above, red, lane, wave);         // >= 1 components of area T are kept: those of the lowest ids
  }

  unsigned kept = 0u, ties_before = 0u;
  for (unsigned base = 0u; base < m; base += WT) {             // ids in order, WT at a time (m is uniform: every thread takes every barrier)
    const unsigned i = base + tid;
    const unsigned a = i < m ? list[i] & ~KEEP : 0u;
    const bool tie = ranked && i < m && a == T;
    const u64 bal = __ballot(tie);
    __syncthreads();
    if (lane == 0) red[wave] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned rank = ties_before + (unsigned)__popcll(bal & ((1ull << lane) - 1ull)), all = 0u;
#pragma unroll
    for (int w = 0; w < WW; ++w) {
      rank += w < wave ? red[w] : 0u;
      all += red[w];
    }
    ties_before += all;
    if (i < m) {
      const bool keep = a >= p.min_area && (!ranked || a > T || (tie && rank < allow));
      list[i] = a | (keep ? KEEP : 0u);
      kept += keep ? 1u : 0u;
    }
  }
  kept = block_sum_u32<WW>(kept, red, lane, wave);
  if (tid == 0) p.n_kept[plane] = (int)kept;
}

__global__ __launch_bounds__(WT) void cc_write_kernel(const CompP p) {
  const int lane = threadIdx.x & 63, pl = blockIdx.z, nw = p.words_x, W = p.W;
  const size_t plane = (size_t)(p.plane0 + pl);
  const u64* src = p.src + plane * p.H * nw;
  const int* parent = p.parent + plane * p.H * W;
  const unsigned* area_id = p.area_id + plane * p.ids_per_plane;
  u64* out = p.out + plane * p.H * nw;
  for (int s = 0; s < WORDS_PER_WAVE; ++s) {
    int y, w;
    if (!word_task(p, s, y, w)) return;
    const u64 m = src[(size_t)y * nw + w] & valid_bits(w, W);
    const bool set = (m >> lane) & 1ull;
    const int start = set ? run_start(m, lane) : lane;
    int keep = 0;
    if (set && start == lane) {
      int q = parent[y * W + w * 64 + lane];
      if (q >= 0) q = parent[q];                               // cc_label_kernel left every run start pointing at its root
      keep = (int)(area_id[-q - 1] >> 31);
    }
    keep = __shfl(keep, start, 64);
    const u64 o = __ballot(set && keep);
    if (lane == 0) out[(size_t)y * nw + w] = o;
  }
}

bool shape_ok(int n, int H, int W) { return n >= 0 && plane_dims_ok(H, W) && plane_area_ok(H, W); }

void set_workspace(CompP& p, void* workspace, int n, int H, int W) {
  const Layout l = layout_of(n, H, W);
  unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
  p.parent = reinterpret_cast<int*>(ws + l.parent);
  p.area_id = reinterpret_cast<unsigned*>(ws + l.area);
  p.roots = reinterpret_cast<u64*>(ws + l.roots);
  p.rowoff = reinterpret_cast<unsigned*>(ws + l.rowoff);
  p.tot = reinterpret_cast<unsigned*>(ws + l.tot);
  p.ids_per_plane = (unsigned)max_ids(H, W);
  p.H = H; p.W = W; p.words_x = (int)plane_words(W);
}

unsigned word_blocks(int H, int words_x) {
  const int64_t per = (int64_t)WW * WORDS_PER_WAVE;
  return (unsigned)(((int64_t)H * words_x + per - 1) / per);
}

}  // namespace

extern "C" int mtbt_sizeof_components_args(int which) {
  return which == 0 ? (int)sizeof(mtbt_components_args) : (which == 1 ? (int)sizeof(mtbt_select_components_args) : -1);
}

extern "C" int64_t mtbt_components_workspace_bytes(int n, int H, int W) {
  if (!shape_ok(n, H, W)) return MTBT_EINVAL;
  if (n == 0) return 0;
  return layout_of(n, H, W).total;
}

extern "C" int mtbt_label_components(const mtbt_components_args* args, void* stream) {
  if (!args) return MTBT_EINVAL;
  const mtbt_components_args& a = *args;
  if (!shape_ok(a.n, a.H, a.W) || !plane_pitch_ok(a.W, a.pitch)) return MTBT_EINVAL;
  if ((a.connectivity != 4 && a.connectivity != 8) || a.max_components < 1 || a.max_components > MAX_COMPONENTS) return MTBT_EINVAL;
  if (!a.packed || !a.n_components || !a.area || !a.box || !a.first) return MTBT_EINVAL;
  if ((a.other != nullptr) != (a.inter != nullptr)) return MTBT_EINVAL;
  const int64_t need = mtbt_components_workspace_bytes(a.n, a.H, a.W);
  if (a.workspace_bytes < need || (need > 0 && !a.workspace)) return MTBT_EINVAL;
  if (!aligned_n(a.packed, 8) || !aligned_n(a.other, 8) || !aligned_n(a.workspace, 16) || !aligned_n(a.labels, 4) ||
      !aligned_n(a.n_components, 4) || !aligned_n(a.area, 4) || !aligned_n(a.box, 4) || !aligned_n(a.first, 4) || !aligned_n(a.inter, 4))
    return MTBT_EALIGN;
  if (a.n == 0) return MTBT_OK;

  CompP p = {};
  set_workspace(p, a.workspace, a.n, a.H, a.W);
  p.src = reinterpret_cast<const u64*>(a.packed);
  p.other = reinterpret_cast<const u64*>(a.other);
  p.labels = a.labels; p.n_components = a.n_components; p.area = a.area; p.box = a.box; p.first = a.first; p.inter = a.inter;
  p.conn8 = a.connectivity == 8; p.C = a.max_components;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned gx = word_blocks(p.H, p.words_x);
  for (int p0 = 0; p0 < a.n; p0 += CHUNK) {                    // the groups own disjoint slices of the workspace
    const unsigned c = (unsigned)(a.n - p0 < CHUNK ? a.n - p0 : CHUNK);
    p.plane0 = p0;
    hipLaunchKernelGGL(cc_init_kernel, dim3(gx, 1, c), dim3(WT), 0, s, p);
    MTBT_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_union_kernel, dim3(gx, 1, c), dim3(WT), 0, s, p);
    MTBT_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_roots_kernel, dim3(gx, 1, c), dim3(WT), 0, s, p);
    MTBT_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_scan_kernel, dim3(c), dim3(WT), 0, s, p);
    MTBT_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_number_kernel, dim3(gx, 1, c), dim3(WT), 0, s, p);
    MTBT_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_label_kernel, dim3(gx, 1, c), dim3(WT), 0, s, p);
    MTBT_LAUNCH_CHECK();
  }
  return MTBT_OK;
}

extern "C" int mtbt_select_components(const mtbt_select_components_args* args, void* stream) {
  if (!args) return MTBT_EINVAL;
  const mtbt_select_components_args& a = *args;
  if (!shape_ok(a.n, a.H, a.W) || !plane_pitch_ok(a.W, a.pitch) || a.keep_largest < 0) return MTBT_EINVAL;
  if (!a.packed || !a.out || !a.n_kept) return MTBT_EINVAL;
  const int64_t need = mtbt_components_workspace_bytes(a.n, a.H, a.W);
  if (a.workspace_bytes < need || (need > 0 && !a.workspace)) return MTBT_EINVAL;
  if (!aligned_n(a.packed, 8) || !aligned_n(a.out, 8) || !aligned_n(a.workspace, 16) || !aligned_n(a.n_kept, 4)) return MTBT_EALIGN;
  if (a.n == 0) return MTBT_OK;

  CompP p = {};
  set_workspace(p, a.workspace, a.n, a.H, a.W);
  p.src = reinterpret_cast<const u64*>(a.packed);
  p.out = reinterpret_cast<u64*>(a.out);
  p.n_kept = a.n_kept;
  p.min_area = a.min_area; p.keep_largest = (unsigned)a.keep_largest;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned gx = word_blocks(p.H, p.words_x);
  for (int p0 = 0; p0 < a.n; p0 += CHUNK) {
    const unsigned c = (unsigned)(a.n - p0 < CHUNK ? a.n - p0 : CHUNK);
    p.plane0 = p0;
    hipLaunchKernelGGL(cc_choose_kernel, dim3(c), dim3(WT), 0, s, p);
    MTBT_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_write_kernel, dim3(gx, 1, c), dim3(WT), 0, s, p);
    MTBT_LAUNCH_CHECK();
  }
  return MTBT_OK;
}
