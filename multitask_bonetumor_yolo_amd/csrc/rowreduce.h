// The fixed-order reductions of the training step (bn_train.hip, pointwise_bwd.hip, train_ops.hip, resample_bwd.hip, optim.hip, wgrad.hip,
// pointwise.hip, conv_igemm.hip).  Nothing here uses an atomic, and THE ORDER OF THE ADDITIONS IS THE CONTRACT -- a step is reproducible
// bit for bit because of it:
//   rows_reduce    a thread adds its rows in ascending order, starting from 0.f; the row groups are then added in row-group order, starting
//                  from 0.f.  The row loop is unrolled four deep for the loads only: unrolling never re-associates a sum.
//   column_sums    lane l adds rows l, l + 64, ... in ascending order, starting from 0.f; then the wave butterfly (wave_sum: offsets 32 .. 1)
//   block_tree_sum the 256-thread LDS halving tree: red[t] += red[t + o] for o = 128, 64, .. 1
//   fold4          four row groups: ((r0 + r1) + r2) + r3
// Level 1 = per-workgroup partial rows in a workspace, level 2 = one wave per output element over those rows.
#pragma once
#include "common.h"

namespace {

constexpr int ROWS_PER_BLOCK = 256;   // pixels per workgroup in the first level

// rows p, p + step, ... < p1 of one 8-channel piece into the NS sums s; `load(p, ch)` returns what a row needs from memory (by value) and
// `terms(raw, t)` turns it into the row's NS x 8 addends.  Four rows' loads are issued before their arithmetic.
template <int NS, typename Load, typename Terms>
__device__ __forceinline__ void rows_accumulate(long p, long p1, int step, int ch, float (&s)[NS][8], Load load, Terms terms) {
  using Raw = decltype(load(p, ch));
  auto add = [&](const Raw& raw) {
    float t[NS][8];
    terms(raw, t);
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int n = 0; n < NS; ++n) s[n][k] += t[n][k];
  };
  for (; p + 3 * step < p1; p += 4 * step) {
    Raw raw[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) raw[u] = load(p + u * step, ch);
#pragma unroll
    for (int u = 0; u < 4; ++u) add(raw[u]);
  }
  for (; p < p1; p += step) add(load(p, ch));
}

// First level: NS sums per 8-channel piece (16-byte chunk) over the pixels [p0, p1) of a 256-thread workgroup.  With at most 256 pieces
// per pixel the threads split into 256 / chunks row groups that walk the pixels in parallel and are then added in row-group order through
// LDS; wider rows (mtbt_channel_sum has no cap on C) give every thread whole columns of pieces, serial over the rows.  `store(ch, tot)`
// receives the NS x 8 totals of piece ch.  In the grouped path a thread's piece is threadIdx.x % chunks for all its rows, so a caller may
// take the piece's constants once, before the call.
template <int NS, typename Load, typename Terms, typename Store>
__device__ __forceinline__ void rows_reduce(long p0, long p1, int chunks, Load load, Terms terms, Store store) {
  __shared__ float red[256 * 8 * NS];
  const int tid = threadIdx.x;
  if (chunks > 256) {
    for (int ch = tid; ch < chunks; ch += 256) {
      float s[NS][8] = {};
      rows_accumulate<NS>(p0, p1, 1, ch, s, load, terms);
      store(ch, s);
    }
    return;
  }
  const int rpp = 256 / chunks, rg = tid / chunks, ch = tid - rg * chunks;
  if (rg < rpp) {
    float s[NS][8] = {};
    rows_accumulate<NS>(p0 + rg, p1, rpp, ch, s, load, terms);
#pragma unroll
    for (int n = 0; n < NS; ++n)
#pragma unroll
      for (int k = 0; k < 8; ++k) red[(rg * chunks + ch) * 8 * NS + n * 8 + k] = s[n][k];
  }
  __syncthreads();
  if (rg == 0) {
    float tot[NS][8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
      for (int n = 0; n < NS; ++n) tot[n][k] = 0.f;
      for (int g = 0; g < rpp; ++g)
#pragma unroll
        for (int n = 0; n < NS; ++n) tot[n][k] += red[(g * chunks + ch) * 8 * NS + n * 8 + k];
    }
    store(ch, tot);
  }
}

// Second level, one wave per output element: the lanes stride over the rows of N columns of a [rows][pitch] partial matrix and are combined
// by the butterfly; every lane gets the N sums.  (A serial loop per element took longer than the first level once there were ~1000 rows.)
template <int N>
__device__ __forceinline__ void column_sums(const float* __restrict__ partial, int rows, int pitch, const int (&col)[N], float (&s)[N]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int n = 0; n < N; ++n) s[n] = 0.f;
  for (int b = lane; b < rows; b += 64)
#pragma unroll
    for (int n = 0; n < N; ++n) s[n] += partial[(long)b * pitch + col[n]];
#pragma unroll
  for (int n = 0; n < N; ++n) s[n] = wave_sum(s[n]);
}

// out[c] (+)= the sum of column c0 + c of a [blocks][pitch] partial matrix, c < C
__global__ __launch_bounds__(256) void channel_sum_final(const float* __restrict__ partial, int blocks, int pitch, int c0, int C, float* __restrict__ out,
                                                         int accumulate) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;                     // whole waves leave together
  float s[1];
  column_sums<1>(partial, blocks, pitch, {c0 + c}, s);
  if ((threadIdx.x & 63) == 0) out[c] = accumulate ? out[c] + s[0] : s[0];
}

// The sum of one value per thread over a 256-thread workgroup by the LDS halving tree; every thread gets it.  ONE call per kernel: there
// is no barrier after the last read, so a second call would overwrite red[] under a thread that still reads it.
__device__ __forceinline__ float block_tree_sum(float s) {
  __shared__ float red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// second level of the scalar sums (mtbt_sumsq, the BiFPN weight gradient): one workgroup over the n workgroup partials; *out (+)= the sum
__global__ __launch_bounds__(256) void scalar_final(const float* __restrict__ partial, int n, float* __restrict__ out, int accumulate) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
  s = block_tree_sum(s);
  if (threadIdx.x == 0) *out = accumulate ? *out + s : s;
}

// A workgroup of 64 columns (lane = column) x 4 row groups (wave = row group): the four row groups' sums of a column, added in row-group
// order; every thread gets its column's total.  ONE call per kernel (no barrier after the reads, as in block_tree_sum).
__device__ __forceinline__ float fold4(float s) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63;
  red[threadIdx.x >> 6][lane] = s;
  __syncthreads();
  return ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// Pre-reduction of a TALL partial matrix, in place.  The one-wave-per-column second levels read a column with one 4-byte access per row:
// every access is its own 64-byte sector, which 15 other waves fetch again -- at the 3 200 .. 51 200 partial rows the conv epilogues write
// for the 80^2 / 160^2 maps of a batch-32 step that is 16x the matrix in L2 traffic and 200+ dependent trips per lane (round 3: the second
// levels took 12 - 15 us on average, 3.3 ms per step together).  Here a workgroup is 16 row lanes x 16 columns (a wave reads four whole
// sectors per instruction), owns `per` consecutive rows and leaves their column sums in ITS OWN first row -- the only row of the matrix it
// may overwrite without a reader still waiting for it.  The caller then runs the second level over S rows of pitch per * pitch.
__global__ __launch_bounds__(256) void colsum_tile_kernel(float* __restrict__ partial, int rows, int pitch, int c0, int cols, int per) {
  __shared__ float red[16][17];
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  const int r0 = blockIdx.y * per, r1 = min(rows, r0 + per);
  float s = 0.f;
  if (c < cols) {
    const float* col = partial + c0 + c;
    int r = r0 + rl;
    for (; r + 48 < r1; r += 64) {
      const float v0 = col[(long)r * pitch], v1 = col[(long)(r + 16) * pitch], v2 = col[(long)(r + 32) * pitch], v3 = col[(long)(r + 48) * pitch];
      s += v0; s += v1; s += v2; s += v3;
    }
    for (; r < r1; r += 16) s += col[(long)r * pitch];
  }
  red[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && c < cols) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][cl];
    partial[(long)r0 * pitch + c0 + c] = t;
  }
}

// host side: reduce `partial` ([rows][pitch], columns [c0, c0 + cols)) in place when it is tall; returns the (rows, pitch) the second level
// is to use.  Deterministic (fixed segment boundaries and orders).
static inline void colsum_prereduce(float* partial, long& rows, int& pitch, int c0, int cols, hipStream_t s) {
  if (rows <= 768 || rows > 0x7fffffffL) return;
  long S = (rows + 255) / 256;
  if (S > 48) S = 48;
  const long per = (rows + S - 1) / S;
  S = (rows + per - 1) / per;
  if (per * pitch > 0x7fffffffL) return;
  hipLaunchKernelGGL(colsum_tile_kernel, dim3((unsigned)((cols + 15) / 16), (unsigned)S), dim3(256), 0, s, partial, (int)rows, pitch, c0, cols, (int)per);
  rows = S;
  pitch = (int)(per * pitch);
}

}  // namespace
