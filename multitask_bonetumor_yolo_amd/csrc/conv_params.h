// Launch parameters of the implicit-GEMM conv kernel (host <-> device).
#pragma once

struct ConvP {
  const void* x;
  const void* w;
  void* y;
  const float* scale;
  const float* shift;
  const void* res;
  void* y2;  // optional pre-activation output, addressed like y
  long xbs, ybs, rbs;
  int ldx, ldy, ldr;
  int N, H, W, C, K, R, S, stride, pad, Ho, Wo;
  int act, out_mode, out_f32, vec_ok;
  int y_linear;  // output (and residual) batch stride == Ho*Wo*pixel stride: offset = pix*ld, no division
  int M;       // N*Ho*Wo (< 2^31)
  int ctiles;  // ceil(K / TC)
  int ptiles_per_xcd;  // ceil(ceil(M / TP) / 8)
  // optional per-channel column sums of the STORED output (bias gradients, BatchNorm batch statistics): partial rows [rows][cs_pitch]
  // of sum (v - cs_shift[k]) in [0, K) and, with cs_sq, of its square in [K, 2K); one row per (pixel tile, wave row), see conv_epilogue.h
  float* cs_part;
  const float* cs_shift;
  int cs_sq, cs_pitch;
  int debug;  // development ablation bits (MTBT_CONV_DEBUG): 1 = no DMA in the K loop, 2 = no fragment reads / MFMAs
};

// Development ablation bits (MTBT_CONV_DEBUG) are compiled in only with -DMTBT_CONV_ABLATION: run-time tests
// inside the K loop split it into dozens of basic blocks and keep the scheduler from batching the fragment reads.
#ifdef MTBT_CONV_ABLATION
#define MTBT_ABL(p, bit) ((p).debug & (bit))
#else
#define MTBT_ABL(p, bit) 0
#endif

// Batched launch (mtbt_conv2d_nhwc_batch): n convolutions of ONE shape as one grid.  `p` carries everything the members share (and member
// 0's pointers); the table holds what may differ.  The member index is a grid dimension (blockIdx.y), so it is wave-uniform: the selected
// row is read with scalar loads from the kernel-argument segment and the kernel bodies run unchanged on the patched ConvP.
#define MTBT_CONV_BATCH_MAX 8
struct ConvMember {
  const void* x;
  const void* w;
  void* y;
  const float* scale;
  const float* shift;
  const void* res;
  long xbs, ybs, rbs;
  int ldx, ldy, ldr;
  int vec_ok, y_linear, pad_;
};

struct ConvBatchP {
  ConvP p;
  ConvMember m[MTBT_CONV_BATCH_MAX];
};

#if defined(__HIPCC__)
// Host side of every conv launch: `kernel` for one call (q a ConvP, n = 1) or one batch (q a ConvBatchP, n members) on `ptiles` pixel
// tiles (in 8 XCD-contiguous ranges) of TC-channel tiles, 256 threads, `lds` bytes of dynamic LDS.  Fills q's tile counts.
inline ConvP& conv_of(ConvP& p) { return p; }
inline ConvP& conv_of(ConvBatchP& b) { return b.p; }
template <typename Kernel, typename Params>
int conv_launch_tiles(Kernel kernel, Params& q, int TC, long ptiles, int n, int lds, hipStream_t stream) {
  ConvP& p = conv_of(q);
  p.ctiles = (p.K + TC - 1) / TC;
  p.ptiles_per_xcd = (int)((ptiles + 7) / 8);
  const long blocks = (long)p.ptiles_per_xcd * 8 * p.ctiles;
  if (blocks <= 0 || blocks > 0x7fffffffL || n < 1 || n > MTBT_CONV_BATCH_MAX) return MTBT_EINVAL;
  if (int rc = mtbt_allow_lds(kernel, lds)) return rc;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), lds, stream, q);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}

__device__ __forceinline__ ConvP conv_member(const ConvBatchP& b, int i) {
  ConvP p = b.p;
  const ConvMember& m = b.m[i];
  p.x = m.x; p.w = m.w; p.y = m.y; p.scale = m.scale; p.shift = m.shift; p.res = m.res;
  p.xbs = m.xbs; p.ybs = m.ybs; p.rbs = m.rbs;
  p.ldx = m.ldx; p.ldy = m.ldy; p.ldr = m.ldr;
  p.vec_ok = m.vec_ok; p.y_linear = m.y_linear;
  return p;
}
#endif
