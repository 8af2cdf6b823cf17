// BatchNorm2d with BATCH statistics (module in train mode), NHWC, fused activation: forward and backward.
// Needed for drop-in parity of `forward(mode="train")`: the reference flips the Detect/Segment heads to train
// mode for that call (main_model.py:358-359), so their BatchNorms normalise with batch statistics
// and update running_mean / running_var (momentum, unbiased variance) even under Lightning validation.
//
// Forward:  xhat = (x - mean) * rstd, u = xhat * gamma + beta, y = act(u)
// Backward: du = dy * act'(u);  s1 = sum_p du;  s2 = sum_p du * xhat;  d beta = s1;  d gamma = s2
//   batch statistics:    dx = gamma * rstd * (du - s1 / M - xhat * s2 / M)
//   running statistics:  dx = gamma * rstd * du
// Deterministic: every sum is one of the fixed-order reductions of rowreduce.h (per-workgroup partial rows in a workspace, then one wave
// per channel); no atomics.
#include <type_traits>

#include "common.h"
#include "rowreduce.h"

namespace {

struct Row8 { float v[8]; };

// The per-channel constants of an 8-channel piece.  Where the piece a thread works on is the same for all its rows (the workgroup size is
// a multiple of the pieces per row) they are read ONCE per thread and the row loop holds only the 16-byte loads and the arithmetic, four
// rows deep.  (Round 3: with the four parameter vectors re-read and one row in flight per trip the backward statistics pass ran at
// 2.0 TB/s, SLOWER than the apply pass that also writes a tensor, and the forward apply at 2.5 TB/s.)
struct BnChan { float mu[8], rs[8], ga[8], be[8]; };
__device__ __forceinline__ BnChan bn_chan(const float* mean, const float* var, const float* gamma, const float* beta, float eps, int c0) {
  BnChan k;
  float va[8];
  ld8<float>(mean + c0, k.mu);
  ld8<float>(var + c0, va);
  ld8<float>(gamma + c0, k.ga);
  ld8<float>(beta + c0, k.be);
#pragma unroll
  for (int e = 0; e < 8; ++e) k.rs[e] = rsqrtf(va[e] + eps);
  return k;
}
// du = dy * act'(xhat * gamma + beta), xhat = (x - mean) * rstd.  ACT: the activation as a compile-time constant, or -1 = the run-time `act`
template <int ACT>
__device__ __forceinline__ void bn_du_k(const float (&a)[8], const float (&b)[8], const BnChan& k, int act, float (&du)[8], float (&xh)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    xh[e] = (b[e] - k.mu[e]) * k.rs[e];
    du[e] = a[e] * act_grad(xh[e] * k.ga[e] + k.be[e], ACT < 0 ? act : ACT);
  }
}

// The ACT x FIXED instantiation a launch takes: f(integral_constant<int, ACT>, integral_constant<bool, FIXED>).  The three activations of
// the network are compile-time constants on the fixed path; everything else reads the run-time `act` (ACT = -1).
template <typename F>
void bn_dispatch(int act, bool fixed, F f) {
  using std::integral_constant;
  if (!fixed) f(integral_constant<int, -1>{}, std::false_type{});
  else if (act == MTBT_ACT_SILU) f(integral_constant<int, MTBT_ACT_SILU>{}, std::true_type{});
  else if (act == MTBT_ACT_ELU) f(integral_constant<int, MTBT_ACT_ELU>{}, std::true_type{});
  else if (act == MTBT_ACT_NONE) f(integral_constant<int, MTBT_ACT_NONE>{}, std::true_type{});
  else f(integral_constant<int, -1>{}, std::true_type{});
}

// workgroups of an apply pass: FIXED takes four pieces per thread and trip and at most 2048 workgroups (8 per CU)
unsigned bn_apply_grid(long pieces, bool fixed, long general_cap) {
  const long per = fixed ? 1024 : 256, cap = fixed ? 2048 : general_cap;
  const long g = (pieces + per - 1) / per;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ---- forward statistics in a single pass: every workgroup reduces its ROWS_PER_BLOCK rows to a per-channel (mean_b, M2_b)
// with sums SHIFTED by the block's first row (no cancellation for |mean| >> sigma); the final kernel combines the blocks exactly
// (Chan et al.): mean = sum n_b mean_b / N, M2 = sum (M2_b + n_b (mean_b - mean)^2), one WAVE per channel striding over the blocks.
// One read of x for the statistics instead of two, and no serial loop over thousands of partial rows. ----
template <typename T>
__global__ __launch_bounds__(256) void bn_block_stats_kernel(const T* __restrict__ x, long pixels, int C, float* __restrict__ partial /* [blocks][2C] */) {
  __builtin_assume(C <= 2048);            // (the entry point refuses more: rows_reduce's branch for wider rows compiles away)
  const long r0 = (long)blockIdx.x * ROWS_PER_BLOCK;
  const long r1 = r0 + ROWS_PER_BLOCK < pixels ? r0 + ROWS_PER_BLOCK : pixels;
  const float nb = (float)(r1 - r0);
  float sh[8];                                  // of this thread's piece: tid % pieces in every row of rows_reduce's grouped path
  ld8<T>(x + r0 * C + threadIdx.x % (C >> 3) * 8, sh);
  float* dst = partial + (long)blockIdx.x * 2 * C;
  rows_reduce<2>(
      r0, r1, C >> 3, [&](long r, int ch) { Row8 v; ld8<T>(x + r * C + ch * 8, v.v); return v; },
      [&](const Row8& v, float (&t)[2][8]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = v.v[e] - sh[e]; t[0][e] = d; t[1][e] = d * d; }
      },
      [&](int ch, const float (&tot)[2][8]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float ts = tot[0][e], tq = tot[1][e];
          const float md = ts / nb;                     // mean of the shifted values
          dst[ch * 8 + e] = sh[e] + md;                 // block mean
          dst[C + ch * 8 + e] = tq - ts * md;           // block M2 = sum d^2 - (sum d)^2 / n
        }
      });
}

// The tail of the three statistics kernels: channel c's mean and biased variance from (mu, M2), and the running updates (unbiased variance).
__device__ __forceinline__ void bn_write_stats(int c, float mu, float m2, long pixels, float* mean, float* var, float* running_mean, float* running_var,
                                               float momentum) {
  mean[c] = mu;
  var[c] = m2 / (float)pixels;
  if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mu;
  if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (pixels > 1 ? m2 / (float)(pixels - 1) : m2 / (float)pixels);
}
// ... from s1 = sum (x - shift), s2 = sum (x - shift)^2.  shift may BE running_mean: it is read before bn_write_stats updates that.
__device__ __forceinline__ void bn_write_stats_shifted(int c, float s1, float s2, const float* shift, long pixels, float* mean, float* var,
                                                       float* running_mean, float* running_var, float momentum) {
  const float n = (float)pixels;
  const float sh = shift ? shift[c] : 0.f;
  const float m1 = s1 / n;
  bn_write_stats(c, sh + m1, fmaxf(s2 - n * m1 * m1, 0.f), pixels, mean, var, running_mean, running_var, momentum);
}

// (its two sums are weighted by the blocks' row counts and the second needs the first's result: column_sums does not fit)
__global__ __launch_bounds__(256) void bn_combine_stats_kernel(const float* __restrict__ partial, int nblocks, int C, long pixels, float* __restrict__ mean,
                                                               float* __restrict__ var, float* __restrict__ running_mean,
                                                               float* __restrict__ running_var, float momentum) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;                                              // whole waves leave together
  const long last = pixels - (long)(nblocks - 1) * ROWS_PER_BLOCK;   // rows of the last block
  float sm = 0.f;
  for (int b = lane; b < nblocks; b += 64) sm += (b == nblocks - 1 ? (float)last : (float)ROWS_PER_BLOCK) * partial[(long)b * 2 * C + c];
  const float mu = wave_sum(sm) / (float)pixels;
  float m2 = 0.f;
  for (int b = lane; b < nblocks; b += 64) {
    const float d = partial[(long)b * 2 * C + c] - mu;
    m2 += partial[(long)b * 2 * C + C + c] + (b == nblocks - 1 ? (float)last : (float)ROWS_PER_BLOCK) * d * d;
  }
  m2 = wave_sum(m2);
  if (lane == 0) bn_write_stats(c, mu, m2, pixels, mean, var, running_mean, running_var, momentum);
}

// batch statistics straight from the conv epilogue's PARTIAL rows ([rows][pitch]: sum (x - s) in [0, C), sum (x - s)^2 in [C, 2C)): the
// second level of the column sums and the statistics in one launch
__global__ __launch_bounds__(256) void bn_stats_from_partials_kernel(const float* __restrict__ partial, int rows, int pitch, const float* __restrict__ shift,
                                                                     long pixels, int C, float* __restrict__ mean, float* __restrict__ var,
                                                                     float* __restrict__ running_mean, float* __restrict__ running_var, float momentum) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;                                   // whole waves leave together
  float s[2];
  column_sums<2>(partial, rows, pitch, {c, C + c}, s);
  if ((threadIdx.x & 63) == 0) bn_write_stats_shifted(c, s[0], s[1], shift, pixels, mean, var, running_mean, running_var, momentum);
}

// batch statistics from the column sums the producing conv's epilogue accumulated (mtbt_conv_args.colsum): sum (x - s), sum (x - s)^2
__global__ void bn_stats_from_sums_kernel(const float* __restrict__ sums, const float* __restrict__ shift, long pixels, int C, float* __restrict__ mean,
                                          float* __restrict__ var, float* __restrict__ running_mean, float* __restrict__ running_var, float momentum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) bn_write_stats_shifted(c, sums[c], sums[C + c], shift, pixels, mean, var, running_mean, running_var, momentum);
}

__global__ void bn_copy_stats_kernel(const float* __restrict__ rm, const float* __restrict__ rv, float* __restrict__ mean, float* __restrict__ var, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) { mean[c] = rm[c]; var[c] = rv[c]; }
}

// y = act((x - mean) * rstd * gamma + beta); y rows of y_ld elements.  FIXED (256 % (C / 8) == 0): a thread's 8-channel piece is the same in
// every trip of the grid-stride loop, so its constants are taken ONCE per thread, the pixel is a shift (C / 8 is a power of two; a 64-bit
// division per piece otherwise) and four pieces are in flight per trip.  Otherwise the plain grid-stride loop, bn_chan per piece.
template <typename T, int ACT, bool FIXED>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ mean, const float* __restrict__ var,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int act, long pixels, int C,
                                                       int y_ld) {
  const int CH8 = C >> 3;
  const long total = pixels * CH8, stride = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  auto one = [&](float (&v)[8], const BnChan& k, long pix, int cg) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = act_apply((v[e] - k.mu[e]) * k.rs[e] * k.ga[e] + k.be[e], ACT < 0 ? act : ACT);
    st8<T>(y + pix * y_ld + cg * 8, v);
  };
  if constexpr (FIXED) {
    const int cg = threadIdx.x % CH8;
    const int sh = 31 - __builtin_clz(CH8);
    const BnChan k = bn_chan(mean, var, gamma, beta, eps, cg * 8);
    for (; i + 3 * stride < total; i += 4 * stride) {
      float v[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) ld8<T>(x + (i + u * stride) * 8, v[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u) one(v[u], k, (i + u * stride) >> sh, cg);
    }
    for (; i < total; i += stride) {
      float v[8];
      ld8<T>(x + i * 8, v);
      one(v, k, i >> sh, cg);
    }
  } else {
    for (; i < total; i += stride) {
      const int cg = (int)(i % CH8);
      float v[8];
      ld8<T>(x + i * 8, v);
      one(v, bn_chan(mean, var, gamma, beta, eps, cg * 8), i / CH8, cg);
    }
  }
}

void launch_bn_apply(int dtype, const void* x, void* y, const float* mean, const float* var, const float* gamma, const float* beta, float eps, int act,
                     long pixels, int C, int y_ld, hipStream_t s) {
  const bool fixed = 256 % (C >> 3) == 0;
  const unsigned g = bn_apply_grid(pixels * (C >> 3), fixed, 8192);
  bn_dispatch(act, fixed, [&](auto A, auto F) {
    if (dtype == MTBT_F32)
      hipLaunchKernelGGL((bn_apply_kernel<float, decltype(A)::value, decltype(F)::value>), dim3(g), dim3(256), 0, s, (const float*)x, (float*)y, mean, var, gamma, beta, eps, act, pixels, C, y_ld);
    else
      hipLaunchKernelGGL((bn_apply_kernel<bf16_t, decltype(A)::value, decltype(F)::value>), dim3(g), dim3(256), 0, s, (const bf16_t*)x, (bf16_t*)y, mean, var, gamma, beta, eps, act, pixels, C, y_ld);
  });
}

// ---- backward.  Pass 1 forms per-workgroup partial (s1, s2) rows; pass 2 sums them (one wave per column); pass 3 recomputes du and writes
// dx.  dy may be a channel slice (row pitch dy_ld); x (the conv output the forward normalised) and dx are dense. ----
// bn_bwd_partial and bn_bwd_apply keep their own loops, and bn_du, the per-row form of bn_chan + bn_du_k that their serial / general
// branches call.  bn_bwd_partial is rows_reduce<2> written out (the same order of additions); through the template, and bn_bwd_apply over a
// walk shared with bn_apply_kernel, the same source compiled to a slower schedule of the loads and to other contractions of the products into
// the sums, that is other bits of d beta and dx (profiles/train_reductions_refactor.txt).
template <typename T>
__device__ __forceinline__ void bn_du(const T* dy, long dy_off, const T* x, long x_off, const float* mean, const float* var, const float* gamma,
                                      const float* beta, float eps, int act, int c0, float (&du)[8], float (&xh)[8], float (&gr)[8]) {
  float a[8], b[8], mu[8], va[8], ga[8], be[8];
  ld8<T>(dy + dy_off, a);
  ld8<T>(x + x_off, b);
  ld8<float>(mean + c0, mu);
  ld8<float>(var + c0, va);
  ld8<float>(gamma + c0, ga);
  ld8<float>(beta + c0, be);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float rstd = rsqrtf(va[e] + eps);
    xh[e] = (b[e] - mu[e]) * rstd;
    du[e] = a[e] * act_grad(xh[e] * ga[e] + be[e], act);
    gr[e] = ga[e] * rstd;
  }
}

// ACT: the activation as a compile-time constant (MTBT_ACT_NONE / SILU / ELU), or -1 = the run-time `act`
template <typename T, int ACT>
__global__ __launch_bounds__(256) void bn_bwd_partial(const T* __restrict__ dy, int dy_ld, const T* __restrict__ x, long P, int C,
                                                      const float* __restrict__ mean, const float* __restrict__ var,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int act,
                                                      float* __restrict__ partial /* [blocks][2C] */) {
  __shared__ float red[256 * 16];
  const int tid = threadIdx.x, chunks = C >> 3;
  const long p0 = (long)blockIdx.x * ROWS_PER_BLOCK, p1 = min(P, p0 + ROWS_PER_BLOCK);
  float* dst = partial + (long)blockIdx.x * 2 * C;
  if (chunks >= 256) {   // (C >= 2048: not used by this network; serial over the rows)
    for (int ch = tid; ch < chunks; ch += 256) {
      float s1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (long p = p0; p < p1; ++p) {
        float du[8], xh[8], gr[8];
        bn_du<T>(dy, p * dy_ld + ch * 8, x, p * C + ch * 8, mean, var, gamma, beta, eps, act, ch * 8, du, xh, gr);
#pragma unroll
        for (int k = 0; k < 8; ++k) { s1[k] += du[k]; s2[k] += du[k] * xh[k]; }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) { dst[ch * 8 + k] = s1[k]; dst[C + ch * 8 + k] = s2[k]; }
    }
    return;
  }
  const int rpp = 256 / chunks, rg = tid / chunks, ch = tid - rg * chunks;
  float s1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (rg < rpp) {
    const BnChan k = bn_chan(mean, var, gamma, beta, eps, ch * 8);
    const T* dyp = dy + ch * 8;
    const T* xp = x + ch * 8;
    long p = p0 + rg;
    for (; p + 3 * rpp < p1; p += 4 * rpp) {      // (rows are added in the same order as one at a time)
      float a[4][8], b[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) { ld8<T>(dyp + (p + u * rpp) * dy_ld, a[u]); ld8<T>(xp + (p + u * rpp) * C, b[u]); }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float du[8], xh[8];
        bn_du_k<ACT>(a[u], b[u], k, act, du, xh);
#pragma unroll
        for (int e = 0; e < 8; ++e) { s1[e] += du[e]; s2[e] += du[e] * xh[e]; }
      }
    }
    for (; p < p1; p += rpp) {
      float a[8], b[8], du[8], xh[8];
      ld8<T>(dyp + p * dy_ld, a); ld8<T>(xp + p * C, b);
      bn_du_k<ACT>(a, b, k, act, du, xh);
#pragma unroll
      for (int e = 0; e < 8; ++e) { s1[e] += du[e]; s2[e] += du[e] * xh[e]; }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { red[(rg * chunks + ch) * 16 + e] = s1[e]; red[(rg * chunks + ch) * 16 + 8 + e] = s2[e]; }
  }
  __syncthreads();
  if (rg == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float t1 = 0.f, t2 = 0.f;
      for (int g = 0; g < rpp; ++g) { t1 += red[(g * chunks + ch) * 16 + k]; t2 += red[(g * chunks + ch) * 16 + 8 + k]; }
      dst[ch * 8 + k] = t1;
      dst[C + ch * 8 + k] = t2;
    }
  }
}

// one wave per column of the [blocks][2C] partials: sums[0..C) = s1 = d beta, sums[C..2C) = s2 = d gamma
__global__ __launch_bounds__(256) void bn_bwd_final(const float* __restrict__ partial, int blocks, int pitch, int C, float* __restrict__ sums,
                                                    float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= 2 * C) return;
  float s[1];
  column_sums<1>(partial, blocks, pitch, {c}, s);
  if ((threadIdx.x & 63) == 0) {
    sums[c] = s[0];
    float* out = c < C ? (dbeta ? dbeta + c : nullptr) : (dgamma ? dgamma + (c - C) : nullptr);
    if (out) *out = accumulate ? *out + s[0] : s[0];
  }
}

// FIXED: 256 % (C / 8) == 0 -- a thread's 8-channel piece is the same in every trip of the grid-stride loop (constants hoisted, four
// rows in flight); otherwise the general loop
template <typename T, int ACT, bool FIXED>
__global__ __launch_bounds__(256) void bn_bwd_apply(const T* __restrict__ dy, int dy_ld, const T* __restrict__ x, T* __restrict__ dx, long P, int C,
                                                    const float* __restrict__ mean, const float* __restrict__ var,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int act,
                                                    const float* __restrict__ sums, int use_running) {
  const int chunks = C >> 3;
  const long n8 = P * chunks;
  const float invM = 1.0f / (float)P;
  if constexpr (FIXED) {
    const int ch = threadIdx.x % chunks;
    const int sh = 31 - __builtin_clz(chunks);           // chunks is a power of two here: pixel = piece >> sh (a 64-bit division per piece otherwise)
    const BnChan k = bn_chan(mean, var, gamma, beta, eps, ch * 8);
    float m1[8], m2[8], gr[8];
    if (use_running) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { m1[e] = 0.f; m2[e] = 0.f; }
    } else {
      ld8<float>(sums + ch * 8, m1);
      ld8<float>(sums + C + ch * 8, m2);
#pragma unroll
      for (int e = 0; e < 8; ++e) { m1[e] = m1[e] * invM; m2[e] = m2[e] * invM; }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) gr[e] = k.ga[e] * k.rs[e];
    const long stride = (long)gridDim.x * 256;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    auto one = [&](const float (&a)[8], const float (&b)[8], long idx) {
      float du[8], xh[8], o[8];
      bn_du_k<ACT>(a, b, k, act, du, xh);
      if (use_running) {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = gr[e] * du[e];
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = gr[e] * (du[e] - m1[e] - xh[e] * m2[e]);
      }
      st8<T>(dx + idx * 8, o);
    };
    for (; i + 3 * stride < n8; i += 4 * stride) {
      float a[4][8], b[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long idx = i + u * stride;
        ld8<T>(dy + (idx >> sh) * dy_ld + ch * 8, a[u]);
        ld8<T>(x + idx * 8, b[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) one(a[u], b[u], i + u * stride);
    }
    for (; i < n8; i += stride) {
      float a[8], b[8];
      ld8<T>(dy + (i >> sh) * dy_ld + ch * 8, a);
      ld8<T>(x + i * 8, b);
      one(a, b, i);
    }
    return;
  }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const int ch = (int)(i % chunks);
    const long p = i / chunks;
    float du[8], xh[8], gr[8], o[8];
    bn_du<T>(dy, p * dy_ld + ch * 8, x, i * 8, mean, var, gamma, beta, eps, act, ch * 8, du, xh, gr);
    if (use_running) {
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = gr[k] * du[k];
    } else {
      float s1[8], s2[8];
      ld8<float>(sums + ch * 8, s1);
      ld8<float>(sums + C + ch * 8, s2);
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = gr[k] * (du[k] - s1[k] * invM - xh[k] * (s2[k] * invM));
    }
    st8<T>(dx + i * 8, o);
  }
}

template <typename T>
void launch_bn_backward(const void* dy, int dy_ld, const void* x, void* dx, long P, int C, const float* stats, const float* gamma, const float* beta, float eps,
                        int act, int use_running, float* partial, float* sums, float* dgamma, float* dbeta, int accumulate, hipStream_t s) {
  const long blocks = (P + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  const float* mean = stats;
  const float* var = stats + C;
  const bool fixed = 256 % (C >> 3) == 0;
  const unsigned ga = bn_apply_grid(P * (C >> 3), fixed, 2048);
  bn_dispatch(act, fixed, [&](auto A, auto F) {
    hipLaunchKernelGGL((bn_bwd_partial<T, decltype(A)::value>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)dy, dy_ld, (const T*)x, P, C, mean, var, gamma, beta, eps, act,
                       partial);
    long rr = blocks;
    int pp = 2 * C;
    colsum_prereduce(partial, rr, pp, 0, 2 * C, s);
    hipLaunchKernelGGL(bn_bwd_final, dim3((unsigned)((2 * C + 3) / 4)), dim3(256), 0, s, partial, (int)rr, pp, C, sums, dgamma, dbeta, accumulate);
    hipLaunchKernelGGL((bn_bwd_apply<T, decltype(A)::value, decltype(F)::value>), dim3(ga), dim3(256), 0, s, (const T*)dy, dy_ld, (const T*)x, (T*)dx, P, C, mean, var, gamma, beta, eps, act, sums,
                       use_running);
  });
}

// what the three forward entry points ask of their common arguments
int bn_forward_check(const void* x, const void* y, int32_t y_pixel_stride, const float* gamma, const float* beta, const float* stats, int64_t pixels, int C,
                     int dtype, int act) {
  if (!x || !y || !gamma || !beta || !stats || pixels <= 0 || C <= 0 || C % 8 || C > 2048 || y_pixel_stride < C || y_pixel_stride % 8) return MTBT_EINVAL;
  if (dtype != MTBT_F32 && dtype != MTBT_BF16) return MTBT_EINVAL;
  if (act < MTBT_ACT_NONE || act > MTBT_ACT_GELU_POLY) return MTBT_EINVAL;
  if (!aligned16(x) || !aligned16(y) || !aligned16(gamma) || !aligned16(beta) || !aligned16(stats)) return MTBT_EALIGN;
  return MTBT_OK;
}

}  // namespace

extern "C" int64_t mtbt_bn_train_workspace_bytes(int64_t pixels, int C) {
  if (pixels <= 0 || C <= 0) return 0;
  const int64_t nb = (pixels + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  return (nb * 2 * C + 2 * (int64_t)C) * (int64_t)sizeof(float);
}

// General form (training lowering): x dense [pixels][C]; y rows of y_pixel_stride elements (a channel slice of a C2f concat buffer, or
// dense; may alias x when dense).  use_running != 0: normalise with running_mean / running_var (module in eval mode; nothing is updated).
// stats [2*C] receives the (mean, biased variance) the normalisation used -- what mtbt_bn_backward_nhwc reads.
extern "C" int mtbt_bn_forward_nhwc(const void* x, void* y, int32_t y_pixel_stride, const float* gamma, const float* beta, float* running_mean,
                                    float* running_var, float momentum, float eps, int act, int64_t pixels, int C, int dtype, int use_running,
                                    float* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  if (const int rc = bn_forward_check(x, y, y_pixel_stride, gamma, beta, stats, pixels, C, dtype, act)) return rc;
  if (use_running && (!running_mean || !running_var)) return MTBT_EINVAL;
  const long nb = (pixels + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  if (nb > 0x7fffffffL) return MTBT_EINVAL;
  float* mean = stats;
  float* var = stats + C;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (use_running) {
    hipLaunchKernelGGL(bn_copy_stats_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, running_mean, running_var, mean, var, C);
  } else {
    if (!workspace || !aligned16(workspace)) return MTBT_EALIGN;
    if (workspace_bytes < nb * 2 * C * (int64_t)sizeof(float)) return MTBT_EWORKSPACE;
    float* partial = reinterpret_cast<float*>(workspace);
    if (dtype == MTBT_F32) hipLaunchKernelGGL(bn_block_stats_kernel<float>, dim3((unsigned)nb), dim3(256), 0, s, (const float*)x, (long)pixels, C, partial);
    else hipLaunchKernelGGL(bn_block_stats_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, s, (const bf16_t*)x, (long)pixels, C, partial);
    hipLaunchKernelGGL(bn_combine_stats_kernel, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, s, partial, (int)nb, C, (long)pixels, mean, var, running_mean,
                       running_var, momentum);
  }
  launch_bn_apply(dtype, x, y, mean, var, gamma, beta, eps, act, (long)pixels, C, y_pixel_stride, s);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}

// The same with the statistics taken from column sums (mtbt_conv_args.colsum of the conv that produced x): sums [2C] = sum (x - shift),
// sum (x - shift)^2 over the `pixels` rows; shift [C] or NULL, and it may alias running_mean (each channel is read before it is updated).
extern "C" int mtbt_bn_forward_sums_nhwc(const void* x, void* y, int32_t y_pixel_stride, const float* gamma, const float* beta, float* running_mean,
                                         float* running_var, float momentum, float eps, int act, int64_t pixels, int C, int dtype,
                                         const float* sums, const float* shift, float* stats, void* stream) {
  if (!sums) return MTBT_EINVAL;
  if (const int rc = bn_forward_check(x, y, y_pixel_stride, gamma, beta, stats, pixels, C, dtype, act)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(bn_stats_from_sums_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, sums, shift, (long)pixels, C, stats, stats + C, running_mean,
                     running_var, momentum);
  launch_bn_apply(dtype, x, y, stats, stats + C, gamma, beta, eps, act, (long)pixels, C, y_pixel_stride, s);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}

// ... and from the conv's partial rows (mtbt_conv_colsum_layout gives rows / pitch): no separate second level.
extern "C" int mtbt_bn_forward_partials_nhwc(const void* x, void* y, int32_t y_pixel_stride, const float* gamma, const float* beta, float* running_mean,
                                             float* running_var, float momentum, float eps, int act, int64_t pixels, int C, int dtype,
                                             float* partial, int64_t rows, int32_t pitch, const float* shift, float* stats, void* stream) {
  if (!partial || rows <= 0 || rows > 0x7fffffffL || pitch < 2 * C) return MTBT_EINVAL;
  if (const int rc = bn_forward_check(x, y, y_pixel_stride, gamma, beta, stats, pixels, C, dtype, act)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  long rr = rows;
  int pp = pitch;
  colsum_prereduce(partial, rr, pp, 0, 2 * C, s);      // tall matrices: folded in place first (rowreduce.h)
  hipLaunchKernelGGL(bn_stats_from_partials_kernel, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, s, partial, (int)rr, pp, shift, (long)pixels, C, stats, stats + C,
                     running_mean, running_var, momentum);
  launch_bn_apply(dtype, x, y, stats, stats + C, gamma, beta, eps, act, (long)pixels, C, y_pixel_stride, s);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}

// x, y: dense NHWC [pixels][C] in `dtype` (y may alias x).  gamma/beta/running_*: fp32 [C] (running_* may be NULL).
// workspace: >= mtbt_bn_train_workspace_bytes; on return its last 2*C floats hold the batch mean and biased variance.
extern "C" int mtbt_bn_train_nhwc(const void* x, void* y, const float* gamma, const float* beta, float* running_mean,
                                  float* running_var, float momentum, float eps, int act, int64_t pixels, int C, int dtype,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  if (!workspace || pixels <= 0 || C <= 0) return MTBT_EINVAL;
  if (workspace_bytes < mtbt_bn_train_workspace_bytes(pixels, C)) return MTBT_EWORKSPACE;
  const long nb = (pixels + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  float* stats = reinterpret_cast<float*>(workspace) + nb * 2 * C;
  return mtbt_bn_forward_nhwc(x, y, C, gamma, beta, running_mean, running_var, momentum, eps, act, pixels, C, dtype, 0, stats, workspace,
                              workspace_bytes, stream);
}

extern "C" int64_t mtbt_bn_backward_workspace_bytes(int64_t pixels, int C) {
  if (pixels <= 0 || C <= 0) return 0;
  return (((pixels + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK) * 2 * (int64_t)C + 2 * (int64_t)C) * (int64_t)sizeof(float);
}

extern "C" int mtbt_bn_backward_nhwc(const void* dy, int32_t dy_pixel_stride, const void* x, const float* stats, const float* gamma, const float* beta,
                                     float eps, int act, int use_running, void* dx, float* dgamma, float* dbeta, int accumulate, int64_t pixels, int C,
                                     int dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!dy || !x || !stats || !gamma || !beta || !dx || !workspace || pixels <= 0 || C <= 0 || C % 8 || C > 2048) return MTBT_EINVAL;
  if (dy_pixel_stride < C || dy_pixel_stride % 8 || act < MTBT_ACT_NONE || act > MTBT_ACT_GELU_POLY) return MTBT_EINVAL;
  if (dtype != MTBT_F32 && dtype != MTBT_BF16) return MTBT_EINVAL;
  if (!aligned16(dy) || !aligned16(x) || !aligned16(dx) || !aligned16(stats) || !aligned16(gamma) || !aligned16(beta) || !aligned16(workspace)) return MTBT_EALIGN;
  if (workspace_bytes < mtbt_bn_backward_workspace_bytes(pixels, C)) return MTBT_EWORKSPACE;
  const long blocks = (pixels + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  if (blocks > 0x7fffffffL) return MTBT_EINVAL;
  float* partial = reinterpret_cast<float*>(workspace);
  float* sums = partial + blocks * 2 * C;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MTBT_F32)
    launch_bn_backward<float>(dy, dy_pixel_stride, x, dx, (long)pixels, C, stats, gamma, beta, eps, act, use_running, partial, sums, dgamma, dbeta, accumulate, s);
  else
    launch_bn_backward<bf16_t>(dy, dy_pixel_stride, x, dx, (long)pixels, C, stats, gamma, beta, eps, act, use_running, partial, sums, dgamma, dbeta, accumulate, s);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}
