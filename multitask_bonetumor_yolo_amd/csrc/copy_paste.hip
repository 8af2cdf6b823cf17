// Copy-paste augmentation between the canvases of a batch (mtbt_copy_paste; the rule and the contract are in include/mtbt_hip.h), feeding
// `preprocess.copy_paste_batch` and the `copy_paste=` option of the `*_samples_seg` functions.  The checks and the by-value table are in
// copy_paste_check.h (host C++ only).
//
// Packed layout as everywhere (mask_eval.hip): a plane is a run of S * pitch / 8 64-bit words, 8-byte aligned, padding bits zero.
//
// copy_paste_kernel   grid (blocks of 64 consecutive words of a canvas, canvases of the launch), 256 threads.  Two phases and one barrier.
//   words   (wave 0) a thread owns ONE 64-bit word position: row y', pixels 64 w .. 64 w + 63.  It forms the canvas's <= 16 translated
//           words T_e -- a funnel shift of two adjacent donor words at bit position 64 w - dx, or, mirrored, the bit reverse of the funnel at
//           S - 1 + dx - 64 w - 63 (which carries the 64 ceil(S/64) - S alignment when S is no multiple of 64); words and rows outside the
//           donor read as zero and every donor word is masked to x < S, so a set bit of T_e always names a donor pixel inside the canvas
//           whatever the padding bits hold.  Walking the entries top-down gives V_e = T_e & ~cover and, as four bit planes, the index of
//           the owning entry per pixel.  It stores V_e, then O_m = planes[m] & ~U for the canvas's old rows: 8-byte stores, consecutive
//           lanes at consecutive words.  Records: a wave reduction per plane, then one integer atomic per record from lane 0, and only for
//           planes with a set bit in the wave's 64 words.  cover, owner planes and the union of the output planes go to LDS (48 B a word).
//   pixels  (all waves) a thread owns 4 adjacent pixels of a word, 16 threads a word, consecutive threads at consecutive addresses: three
//           16-byte loads of the canvas's own pixels, then, for the pixels whose cover bit is set, three scalar loads each from the
//           donor address (a reversed but contiguous segment when mirrored), three 16-byte stores and the mask's.
// finish_kernel       one thread per output row: the box maxima (S - X, S - Y, X + 1, Y + 1) back to minima, then the label row.
//
// Every output byte is written exactly once; the input is only read.  Roof: the bytes of the canvases and planes, once in and once out,
// plus the donor pixels of the pasted area; the measured ratio to a plain copy of the same bytes is in DESIGN.md.
#include "bitplane.h"
#include "copy_paste_check.h"

namespace {

using copy_paste::Batch;
using copy_paste::Canvas;
using copy_paste::Entry;
constexpr int MAXE = copy_paste::MAX_ENTRIES;
constexpr int WORDS = 64;        // words of a block
constexpr int PT = 256;          // threads of a block: 16 per word in the pixel phase, four passes

struct Params {
  const float* images; const u64* planes; const float* rows_in;
  float* out_images; u64* out_planes; float* out_masks; float* rows_out;
  uint32_t* area_before; uint32_t* area; int32_t* box;
  int S, nw, M;
};

// word q of a donor row, zero outside the row, bits x >= S dropped
__device__ __forceinline__ u64 donor_word(const u64* __restrict__ row, int q, int nw, int S) {
  return (q < 0 || q >= nw) ? 0ull : (row[q] & low_bits(S - 64 * q));
}
// the 64 donor bits at positions p .. p + 63 (p may be negative or reach past the row)
__device__ __forceinline__ u64 window(const u64* __restrict__ row, int p, int nw, int S) {
  const int q = p >> 6, s = p & 63;                                    // arithmetic shift = floor
  const u64 lo = donor_word(row, q, nw, S);
  if (s == 0) return lo;
  return (lo >> s) | (donor_word(row, q + 1, nw, S) << (64 - s));
}

// area_before / area / box of output row `pl` from this wave's words: `before` and `after` are the lane's word of the plane before and after
// the layering.  Wave-uniform control flow: the whole of wave 0 calls it.
__device__ __forceinline__ void record(const Params& p, long pl, u64 before, u64 after, int X0, int Y, int lane) {
  if (__ballot(before != 0ull) == 0ull) return;                        // after is a subset of before
  const unsigned nb = wave_sum_u32((unsigned)__popcll(before));
  if (lane == 0) atomicAdd(p.area_before + pl, nb);
  if (__ballot(after != 0ull) == 0ull) return;
  const unsigned na = wave_sum_u32((unsigned)__popcll(after));
  const unsigned b0 = wave_max_u32(after ? (unsigned)(p.S - (X0 + __ffsll((long long)after) - 1)) : 0u);
  const unsigned b1 = wave_max_u32(after ? (unsigned)(p.S - Y) : 0u);
  const unsigned b2 = wave_max_u32(after ? (unsigned)(X0 + 64 - __clzll((long long)after)) : 0u);
  const unsigned b3 = wave_max_u32(after ? (unsigned)(Y + 1) : 0u);
  if (lane == 0) {
    atomicAdd(p.area + pl, na);
    atomicMax(p.box + 4 * pl + 0, (int)b0);
    atomicMax(p.box + 4 * pl + 1, (int)b1);
    atomicMax(p.box + 4 * pl + 2, (int)b2);
    atomicMax(p.box + 4 * pl + 3, (int)b3);
  }
}

__global__ __launch_bounds__(PT) void copy_paste_kernel(const Batch b, const Params p, const int first) {
  __shared__ Entry s_entry[MAXE];
  __shared__ u64 s_cover[WORDS], s_union[WORDS], s_own[4][WORDS];
  const int tid = threadIdx.x;
  const Canvas& cv = b.c[blockIdx.y];
  const int canvas = first + (int)blockIdx.y;
  const int S = p.S, nw = p.nw, n = cv.n;
  const long words = (long)S * nw;                                     // of a plane: <= 32768 * 512
  const long g0 = (long)blockIdx.x * WORDS;

  if (tid < WORDS) {                                                   // ---- words: exactly wave 0
    const long g = g0 + tid;
    const bool live = g < words;
    const long gl = live ? g : words - 1;
    const int Y = (int)(gl / nw), w = (int)(gl - (long)Y * nw), X0 = 64 * w;
    const u64 valid = live ? low_bits(S - X0) : 0ull;
    u64 cover = 0ull, own0 = 0ull, own1 = 0ull, own2 = 0ull, own3 = 0ull;
#pragma unroll
    for (int e = MAXE - 1; e >= 0; --e) {                              // top-down: the later entry lies above
      if (e < n) {                                                     // block-uniform
        const Entry en = cv.e[e];
        const long pl = (long)p.M + cv.paste0 + e;
        if (tid == 0) {
          s_entry[e] = en;
          if (blockIdx.x == 0 && p.rows_out) {                         // image and class of the pasted row; finish_kernel adds the box
            p.rows_out[6 * pl] = (float)canvas;
            p.rows_out[6 * pl + 1] = p.rows_in[6l * en.row + 1];
          }
        }
        u64 T = 0ull;
        const int y = Y - en.dy;
        if (y >= 0 && y < S) {
          const u64* row = p.planes + (long)en.row * words + (long)y * nw;
          T = ((en.src & 1) ? __brevll(window(row, S - 1 + en.dx - X0 - 63, nw, S)) : window(row, X0 - en.dx, nw, S)) & valid;
        }
        const u64 V = T & ~cover;
        cover |= T;
        if (e & 1) own0 |= V;
        if (e & 2) own1 |= V;
        if (e & 4) own2 |= V;
        if (e & 8) own3 |= V;
        if (live) p.out_planes[pl * words + g] = V;
        record(p, pl, T, V, X0, Y, tid);
      }
    }
    u64 all = cover;
    for (int m = cv.row0; m < cv.row1; ++m) {
      const u64 old = live ? (p.planes[(long)m * words + g] & valid) : 0ull;
      const u64 O = old & ~cover;
      if (live) p.out_planes[(long)m * words + g] = O;
      all |= old;
      record(p, m, old, O, X0, Y, tid);
    }
    s_cover[tid] = cover; s_union[tid] = all;
    s_own[0][tid] = own0; s_own[1][tid] = own1; s_own[2][tid] = own2; s_own[3][tid] = own3;
  }
  __syncthreads();

  const long plane_px = (long)S * S;
  const float* own_img = p.images + (long)canvas * 3 * plane_px;
  float* out_img = p.out_images + (long)canvas * 3 * plane_px;
#pragma unroll
  for (int pass = 0; pass < WORDS * 16 / PT; ++pass) {                 // ---- pixels
    const int q = pass * PT + tid, k = q >> 4, sub = q & 15;
    const long g = g0 + k;
    if (g >= words) continue;
    const int Y = (int)(g / nw), w = (int)(g - (long)Y * nw), X = 64 * w + 4 * sub;
    if (X >= S) continue;                                              // S % 4 == 0: the four pixels are inside together
    const long at = (long)Y * S + X;
    f32x4 c0 = *reinterpret_cast<const f32x4*>(own_img + at);
    f32x4 c1 = *reinterpret_cast<const f32x4*>(own_img + plane_px + at);
    f32x4 c2 = *reinterpret_cast<const f32x4*>(own_img + 2 * plane_px + at);
    const unsigned cov = (unsigned)(s_cover[k] >> (4 * sub)) & 15u;
    if (cov) {
      const unsigned o0 = (unsigned)(s_own[0][k] >> (4 * sub)) & 15u, o1 = (unsigned)(s_own[1][k] >> (4 * sub)) & 15u;
      const unsigned o2 = (unsigned)(s_own[2][k] >> (4 * sub)) & 15u, o3 = (unsigned)(s_own[3][k] >> (4 * sub)) & 15u;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (!((cov >> i) & 1u)) continue;
        const Entry en = s_entry[((o0 >> i) & 1u) | (((o1 >> i) & 1u) << 1) | (((o2 >> i) & 1u) << 2) | (((o3 >> i) & 1u) << 3)];
        const int x = (en.src & 1) ? S - 1 - (X + i - en.dx) : X + i - en.dx, y = Y - en.dy;   // inside [0, S)^2: the bit of T_e was set
        const float* d = p.images + (long)(en.src >> 1) * 3 * plane_px + (long)y * S + x;
        c0[i] = d[0];
        c1[i] = d[plane_px];
        c2[i] = d[2 * plane_px];
      }
    }
    *reinterpret_cast<f32x4*>(out_img + at) = c0;
    *reinterpret_cast<f32x4*>(out_img + plane_px + at) = c1;
    *reinterpret_cast<f32x4*>(out_img + 2 * plane_px + at) = c2;
    if (p.out_masks) {
      const unsigned u = (unsigned)(s_union[k] >> (4 * sub)) & 15u;
      *reinterpret_cast<f32x4*>(p.out_masks + (long)canvas * plane_px + at) =
          f32x4{(u & 1u) ? 1.f : 0.f, (u & 2u) ? 1.f : 0.f, (u & 4u) ? 1.f : 0.f, (u & 8u) ? 1.f : 0.f};
    }
  }
}

__global__ __launch_bounds__(PT) void finish_kernel(const Params p, const int n) {
  const int k = blockIdx.x * PT + threadIdx.x;
  if (k >= n) return;
  int* bx = p.box + 4l * k;
  int x1 = 0, y1 = 0;
  const int x2 = bx[2], y2 = bx[3];
  if (x2 > 0) {            // not empty: bx[0] = S - min X, bx[1] = S - min Y
    x1 = p.S - bx[0];
    y1 = p.S - bx[1];
  }
  bx[0] = x1;
  bx[1] = y1;
  if (!p.rows_out) return;
  float* r = p.rows_out + 6l * k;
  const unsigned area = p.area[k];
  if (k < p.M) {
    const float* in = p.rows_in + 6l * k;
    r[0] = in[0];
    r[1] = in[1];
    if (area == p.area_before[k]) {
      r[2] = in[2]; r[3] = in[3]; r[4] = in[4]; r[5] = in[5];
      return;
    }
  }
  const float fs = (float)p.S;
  r[2] = area ? __fdiv_rn((float)(x1 + x2), 2.f * fs) : 0.f;
  r[3] = area ? __fdiv_rn((float)(y1 + y2), 2.f * fs) : 0.f;
  r[4] = area ? __fdiv_rn((float)(x2 - x1), fs) : 0.f;
  r[5] = area ? __fdiv_rn((float)(y2 - y1), fs) : 0.f;
}

}  // namespace

extern "C" int mtbt_sizeof_copy_paste_args(int which) { return which == 0 ? (int)sizeof(mtbt_copy_paste_args) : -1; }

extern "C" int mtbt_copy_paste(const mtbt_copy_paste_args* a, void* stream) {
  const int status = copy_paste::check(a);
  if (status != MTBT_OK) return status;
  const mtbt_copy_paste_args& q = *a;
  if (q.B == 0) return MTBT_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int N = q.M + q.P;
  Params p{q.images, reinterpret_cast<const u64*>(q.planes), q.rows_in, q.out_images, reinterpret_cast<u64*>(q.out_planes), q.out_masks,
           N > 0 ? q.rows_out : nullptr, q.area_before, q.area, q.box, q.S, q.pitch >> 3, q.M};
  if (N > 0) {
    if (hipMemsetAsync(q.area_before, 0, (size_t)N * sizeof(uint32_t), s) != hipSuccess) return MTBT_ELAUNCH;
    if (hipMemsetAsync(q.area, 0, (size_t)N * sizeof(uint32_t), s) != hipSuccess) return MTBT_ELAUNCH;
    if (hipMemsetAsync(q.box, 0, (size_t)N * 4 * sizeof(int32_t), s) != hipSuccess) return MTBT_ELAUNCH;
  }
  const long words = (long)q.S * p.nw;
  const unsigned blocks = (unsigned)((words + WORDS - 1) / WORDS);     // <= 32768 * 512 / 64
  for (int first = 0; first < q.B; first += copy_paste::CHUNK) {
    const int nb = q.B - first < copy_paste::CHUNK ? q.B - first : copy_paste::CHUNK;
    Batch b;
    copy_paste::describe(q, first, nb, b);
    hipLaunchKernelGGL(copy_paste_kernel, dim3(blocks, (unsigned)nb), dim3(PT), 0, s, b, p, first);
    MTBT_LAUNCH_CHECK();
  }
  if (N > 0) {
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)((N + PT - 1) / PT)), dim3(PT), 0, s, p, N);
    MTBT_LAUNCH_CHECK();
  }
  return MTBT_OK;
}
