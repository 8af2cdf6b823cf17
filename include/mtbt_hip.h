/*
 * mtbt_hip.h -- C ABI of libmtbt_hip.so: the MI355X (gfx950) kernels behind the drop-in
 * `ConvNeXtBiFPNYOLO` module and its post-process.
 *
 * The reference has no FFI of its own: its operator API for this path is the `nn.Module`
 * (`/root/reference/src/main_model.py:300-393`) calling torch.nn operators.  Each entry point below
 * names the torch operator call sites (reference file:line) it replaces.  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (a torch tensor's storage);
 *   - `stream` is a hipStream_t passed as void* (the caller's current stream); launches are
 *     asynchronous, nothing here synchronises, allocates, reads environment variables or keeps mutable
 *     global state (the only process-wide effect is the idempotent, per-device, one-time opt-in of a few
 *     kernels to more than 64 KiB of dynamic LDS), so the library is re-entrant (autograd worker
 *     threads) and graph-capturable;
 *   - activations are NHWC ("channels last"): element (n,y,x,c) of a tensor with C channels lives at
 *     base + n*batch_stride + (y*W + x)*pixel_stride + c   (strides in ELEMENTS);
 *     pixel_stride >= C lets a tensor be a channel slice of a wider buffer (concat-free C2f);
 *   - return value: 0 = launched, <0 = MTBT_E* (nothing launched).  No exceptions cross the ABI.
 */
#ifndef MTBT_HIP_H
#define MTBT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTBT_OK 0
#define MTBT_EINVAL (-1)   /* bad argument / unsupported shape */
#define MTBT_EALIGN (-2)   /* pointer or stride not aligned as the kernel requires */
#define MTBT_ELAUNCH (-3)  /* hipLaunchKernel reported an error */
#define MTBT_EWORKSPACE (-4) /* caller workspace too small */

/* storage / arithmetic types */
#define MTBT_F32 0
#define MTBT_BF16 1
#define MTBT_F16 2 /* IEEE binary16 storage, v_mfma_f32_16x16x32_f16, fp32 accumulate, SATURATING stores (+-65504): the inference
                      kernels (conv, depthwise, stem, LayerNorm, fusion, GAP+FC, fused MLP, casts) -- BASELINE configs[4] */

/* fused epilogue activations */
#define MTBT_ACT_NONE 0
#define MTBT_ACT_SILU 1 /* main_model.py:136 ; ultralytics Conv */
#define MTBT_ACT_ELU 2  /* main_model.py:96 */
#define MTBT_ACT_GELU 3 /* timm Mlp act (erf form), main_model.py:21-26 [upstream] */
#define MTBT_ACT_DSILU 5 /* backward epilogues of mtbt_conv2d_nhwc: y = (conv * scale + shift) * act'(res), res = the kept PRE-activation */
#define MTBT_ACT_DELU 6
#define MTBT_ACT_DGELU 7 /* e.g. the ConvNeXt fc2 input gradient lands directly as d(fc1 pre-activation) */
#define MTBT_ACT_GELU_POLY 4 /* the same GELU as x * Phi(x) with Phi an odd degree-13 polynomial on [-4,4]: |error| <= 2.3e-4,
                              below bf16 resolution; no exp / rcp.  For bf16 outputs (the fp32 parity mode uses MTBT_ACT_GELU). */
#define MTBT_ACT_DGELU_POLY 8 /* backward epilogue for MTBT_ACT_GELU_POLY: the EXACT derivative of that polynomial form (no erf / exp) */

/* conv output addressing */
#define MTBT_OUT_NHWC 0
#define MTBT_OUT_CONVT2X2 1 /* ConvTranspose2d(k=2,s=2): GEMM row q*Cout+co -> pixel (2y+q/2, 2x+q%2), channel co */

/* Bumped whenever an argument struct or a signature below changes (round 1 = 1; round 2 added fields / positional arguments without
 * bumping it; round 3 starts at 3).  The library travels prebuilt: a binding built against another header must refuse to load. */
#define MTBT_ABI_VERSION 5
int mtbt_abi_version(void);
/* sizeof() of the argument structs as the LIBRARY was compiled: which = 0 mtbt_conv_args, 1 mtbt_fuse_args, 2 mtbt_decode_args,
 * 3 mtbt_mask_args, 4 mtbt_loss_args, 5 mtbt_prep_desc, 6 mtbt_raw_image, 7 mtbt_upconv_args, 8 mtbt_node_args, 9 mtbt_box_eval_args; -1 for any other value.  A binding compares them with its
 * own layout at load time (a stale prebuilt .so would otherwise read pointers from the wrong offsets). */
int mtbt_sizeof_args(int which);
/* "gfx950" */
const char* mtbt_target_arch(void);

/* ---------------------------------------------------------------------------------------------
 * Dense convolution as implicit GEMM on MFMA, fused affine + activation (+ residual) epilogue.
 *   y = act(conv(x, w) * scale[k] + shift[k]) (+ res)
 * Replaces every `nn.Conv2d(groups=1)` / `nn.Linear` / `nn.ConvTranspose2d(2,2)` + folded BatchNorm
 * + activation on the path: ConvBlock (main_model.py:113-141), C2f/Bottleneck (:42-59, :144-173),
 * DepthwiseConvBlock.pointwise (:84-93), BiFPN projections (:263-265), ConvNeXt downsample 2x2/2 and
 * MLP fc1/fc2 (+GELU, +layer-scale residual) (:21-26 [timm]), ultralytics Conv / Conv2d / Proto
 * (:324-328 [ultralytics]).
 * dtype MTBT_BF16: v_mfma_f32_16x16x32_bf16, fp32 accumulate.  MTBT_F32: v_mfma_f32_16x16x4_f32
 * (exact fp32 products and sums) -- the parity mode.
 * ------------------------------------------------------------------------------------------- */
typedef struct mtbt_conv_args {
  const void* x;       /* [N,H,W,C] dtype */
  const void* w;       /* [K][R][S][C] dtype (KRSC, C contiguous) */
  void* y;             /* [N,Ho,Wo,K] out_dtype (or ConvT scatter target) */
  const float* scale;  /* [K] or NULL (=1) */
  const float* shift;  /* [K] or NULL (=0) */
  const void* res;     /* residual, addressed like y, dtype; or NULL */
  int64_t x_batch_stride, y_batch_stride, res_batch_stride; /* elements */
  int32_t x_pixel_stride, y_pixel_stride, res_pixel_stride; /* elements */
  int32_t N, H, W, C;  /* input; C % (64 bytes / sizeof(dtype)) == 0 */
  int32_t K;           /* GEMM rows = output channels (4*Cout for CONVT2X2) */
  int32_t R, S;        /* filter */
  int32_t stride, pad; /* same in y and x */
  int32_t Ho, Wo;      /* conv output size (before the CONVT scatter) */
  int32_t dtype;       /* MTBT_F32 | MTBT_BF16 | MTBT_F16: x, w, res */
  int32_t out_dtype;   /* dtype of y: == dtype, or MTBT_F32 */
  int32_t act;         /* MTBT_ACT_* */
  int32_t out_mode;    /* MTBT_OUT_* */
  int32_t tile_hint;   /* 0 = heuristic; else (TC<<16)|TP to force a tile (tests / tuning); bit 25 = row-reuse direct 3x3
                          kernel, bit 26 = keep a 3x3 on the implicit-GEMM kernel, bit 27 = 64-byte K-steps, bits 28-30 ignored
                          (once the number of LDS stages: every kernel has two) */
  void* y2;            /* optional second output (training forward): the PRE-activation conv * scale + shift, addressed and typed
                          like y (no residual added); NULL = not written.  MTBT_OUT_NHWC only. */
  int32_t policy;      /* 0 = default kernel-selection policy; else 0x100 | bits (bit0 small 1x1 tiles, bit1 64x64 tiles for small k x k,
                          bit2 direct 3x3 kernel, bit3 row-reuse 3x3 everywhere, bit4 never, bit5 64-channel direct tiles): the host's
                          A/B knob, passed per call -- the library reads no environment variables and keeps no mutable global state */
  int32_t debug;       /* ablation bits, honoured by -DMTBT_CONV_ABLATION builds only */
  /* Optional per-channel COLUMN SUMS of the output the call stores (values as rounded to out_dtype), from the conv epilogue itself:
   *   colsum[k] (+)= sum_p (y[p][k] - colsum_shift[k]);   colsum_sq: colsum[K + k] (+)= sum_p (y[p][k] - colsum_shift[k])^2
   * Replaces a separate pass over y for nn.BatchNorm2d's batch statistics (main_model.py:95,126-136: the conv in front of the BatchNorm;
   * shift = the running mean keeps sum / sum of squares well conditioned) and for bias gradients (d fc1.bias = sum_p of the
   * fc2-dgrad * GELU' output, main_model.py:21-26 [timm Mlp]).  MTBT_OUT_NHWC only; colsum NULL = off.  Deterministic (fixed-order
   * partial rows in colsum_ws -- rows x pitch floats as reported by mtbt_conv_colsum_layout, never more than
   * mtbt_conv_colsum_workspace_bytes -- then one wave per channel). */
  float* colsum;             /* [K] or [2K] f32 */
  const float* colsum_shift; /* [K] f32 or NULL (= 0) */
  int32_t colsum_sq;         /* != 0: also the sum of squares */
  int32_t colsum_accumulate; /* != 0: add to colsum instead of overwriting */
  void* colsum_ws;
  int64_t colsum_ws_bytes;
} mtbt_conv_args;

int mtbt_conv2d_nhwc(const mtbt_conv_args* a, void* stream);
int64_t mtbt_conv_colsum_workspace_bytes(int64_t pixels /* N*Ho*Wo */, int K, int with_squares);
/* colsum may be NULL with colsum_ws set: only the partial rows are written (rows x pitch floats, a row = [sums (K) | sums of squares (K)]
 * of one pixel tile's wave row) for a consumer that reduces them itself; this reports the layout a call with the same arguments produces. */
int mtbt_conv_colsum_layout(const mtbt_conv_args* a, int64_t* rows, int32_t* pitch);
/* Which kernel and tile mtbt_conv2d_nhwc would run for these arguments (nothing is launched, no pointer is dereferenced):
 * choice[0] = 0 implicit GEMM / 1 direct 3x3 (LDS-resident halo) / 2 streaming head conv; [1] channel tile; [2] pixel tile (256 = the
 * 16 x 16 halo tile); [3] = 128-byte K-steps (implicit GEMM) or first formulation (direct).  For tests of the tile rules and tools. */
int mtbt_conv_kernel_choice(const mtbt_conv_args* a, int32_t* choice);

/* n convolutions of ONE shape (1 <= n <= 8) as one launch; result by result what n calls of mtbt_conv2d_nhwc give.
 * Members agree in N, H, W, C, K, R, S, stride, pad, Ho, Wo, dtype, out_dtype, act, out_mode (MTBT_OUT_NHWC only), tile_hint, policy,
 * debug and in which of scale / shift / res are NULL; they may differ in every pointer and in every batch / pixel stride (channel slices of
 * one buffer, fp32 maps of different pitch).  y2, colsum and colsum_ws must be NULL (training forms: single calls).  The output regions of
 * two members must not overlap (disjoint byte ranges, or channel slices of the same rows: equal pixel / batch stride, the batch stride a
 * multiple of the pixel stride); no member's output may be another member's input.
 * ONE kernel for the whole batch: the single call's rules with the workgroup count taken over all members.  The batched kernels exist for
 * the implicit GEMM with 128-byte K-steps (C * element size a multiple of 128) at 64x64, 128x128, 128x64 and 32x64 tiles, for the row-reuse
 * direct 3x3 at 64-channel tiles (K >= 96: set policy bit 5) and for the streaming head conv at K <= 32; a batch whose rules give
 * anything else returns MTBT_EINVAL (a tile_hint selects an instantiated tile).  Alignment rules per member (MTBT_EALIGN). */
int mtbt_conv2d_nhwc_batch(const mtbt_conv_args* calls, int n, void* stream);
/* The choice of mtbt_conv2d_nhwc_batch for these members, as mtbt_conv_kernel_choice reports it (nothing is launched); the same errors. */
int mtbt_conv_batch_kernel_choice(const mtbt_conv_args* calls, int n, int32_t* choice);

/* ---------------------------------------------------------------------------------------------
 * ConvNeXt stem: Conv2d(3,Cout,4,stride 4,bias) on the caller's NCHW fp32 image + LayerNorm2d.
 * Replaces timm `stem_0`/`stem_1` (main_model.py:21-26,34 [timm]).
 *   x [N,3,H,W] f32 NCHW contiguous;  w [Cout][48] f32 (c,ky,kx order = torch layout flattened);
 *   y [N,H/4,W/4,Cout] out_dtype NHWC dense.
 * ------------------------------------------------------------------------------------------- */
int mtbt_stem_conv4x4_ln(const float* x, const float* w, const float* bias, const float* ln_w,
                         const float* ln_b, float ln_eps, void* y, int N, int H, int W, int Cout,
                         int out_dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Depthwise k x k convolution (k in {3,7}, stride 1, pad k/2), NHWC dense, two epilogues:
 *   ln_w != NULL : + bias, then LayerNorm over C (ConvNeXt block conv_dw + norm, [timm])
 *   ln_w == NULL : * scale[c] + shift[c], then activation (ultralytics DWConv + BN + SiLU,
 *                  Detect.cv3, main_model.py:324 [ultralytics])
 *   w [k*k][C] (tap-major) in the activation dtype;  C % 8 == 0, C <= 768.
 * ------------------------------------------------------------------------------------------- */
int mtbt_dwconv_nhwc(const void* x, const void* w, const float* bias, const float* ln_w,
                     const float* ln_b, float ln_eps, const float* scale, const float* shift, int act,
                     void* y, int N, int H, int W, int C, int ksize, int dtype, void* stream);
/* Depthwise 3 x 3 with a depth multiplier M in {1, 2} (a grouped conv with groups = C and M * C outputs, regrouped): x [N,H,W,C] dense,
 * y [N,H,W,M*C] dense, w [9][M*C] tap-major, scale / shift [M*C]; output channel j reads input channel j mod C, then scale[j] * v + shift[j]
 * and the activation.  Channels [m*C, (m+1)*C) are bit-identical to mtbt_dwconv_nhwc (ksize 3, scale / shift form) on the m-th block of
 * w / scale / shift: two depthwise branches off one tensor as one launch.  C % 128 == 0, M * C <= 768. */
int mtbt_dwconv3x3_mult_nhwc(const void* x, const void* w, const float* scale, const float* shift, int act, void* y,
                             int N, int H, int W, int C, int M, int dtype, void* stream);
/* Which kernel, tile and grid mtbt_dwconv_nhwc (and mtbt_dwconv_nhwc_train: its extra outputs do not take part) would launch for this
 * shape; ln != 0 = the LayerNorm form.  Nothing is launched and there is no pointer to dereference: the launch code itself runs and
 * reports in place of the launch.  choice[0] tile height; [1] tile width; [2] outputs per lane row (8, or 4 on the half-width tile);
 * [3] chunks of 128 channels the kernel holds in registers (1, 2, 3, 6; 1 with C > 128 = the chunks as grid rows); [4] 1 = the full-tile
 * instantiation without bounds checks around the stores; [5] the activation compiled in (MTBT_ACT_*; -1 = the runtime argument);
 * [6] tiles; [7] gridDim.x = persistent workgroups per grid row; [8] gridDim.y.  The shape errors of mtbt_dwconv_nhwc.  For tests. */
int mtbt_dwconv_kernel_choice(int N, int H, int W, int C, int ksize, int ln, int act, int dtype, int32_t* choice);
/* The same for mtbt_dwconv3x3_mult_nhwc. */
int mtbt_dwconv3x3_mult_kernel_choice(int N, int H, int W, int C, int M, int act, int dtype, int32_t* choice);

/* LayerNorm over C of an NHWC dense tensor (timm LayerNorm2d in `stages_i.downsample.0`). */
int mtbt_layernorm_nhwc(const void* x, const float* w, const float* b, float eps, void* y,
                        int64_t pixels, int C, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BiFPN fusion node (main_model.py:211-213, :217-219, :228-232, :236-240):
 *   y = sum_i wgt[i] * resample_i(x_i), i < n_in <= 3, accumulated left to right in fp32.
 * resample: 0 identity, 1 bilinear x2 up (align_corners=False), 2 bilinear x0.5 (== 2x2 mean),
 *           3 nearest x2 up, 4 max-pool 2x2  (3,4: src/model.py:58-70).
 * add_weight_bug != 0 reproduces src/model.py:33-36 `sum(w_i + f_i)`.
 * All tensors NHWC dense with C channels; y is [N,H,W,C].
 * ------------------------------------------------------------------------------------------- */
typedef struct mtbt_fuse_args {
  const void* x[3];
  float wgt[3];
  int32_t resample[3];
  int32_t n_in;
  void* y;
  int32_t N, H, W, C; /* OUTPUT size; input i has H/2,W/2 (up), 2H,2W (down) or H,W */
  int32_t dtype;
  int32_t add_weight_bug;
  const float* wgt_dev; /* optional: n_in weights in DEVICE memory used instead of wgt[] (training: the fusion weights are
                           parameters that change every step, main_model.py:191-196) */
} mtbt_fuse_args;

int mtbt_bifpn_fuse(const mtbt_fuse_args* a, void* stream);

/* The whole BiFPN node in one launch (inference, 16-bit storage): the weighted sum above as the B-operand staging of the
 * DepthwiseConvBlock's 1x1 GEMM (main_model.py:62-102: depthwise k = 1 scale folded into the pointwise weight, BatchNorm folded, ELU):
 *   y[p][k] = act( sum_c w[k][c] * fuse(p)[c] + shift[k] )
 * fuse.y is ignored (the fused map never reaches memory; it is rounded to the storage type exactly as mtbt_bifpn_fuse stores it, so the
 * result equals the two-launch form up to the GEMM's accumulation order).  K == fuse.C in {128, 256}, fuse.dtype MTBT_BF16 | MTBT_F16,
 * add_weight_bug must be 0; the inputs' modes must be (identity, bilinear x2) or (identity, identity, 2x2 mean) -- the two node shapes of
 * BiFPNUnit.forward; anything else returns MTBT_EINVAL (use mtbt_bifpn_fuse + mtbt_conv2d_nhwc).  y [N,H,W,K] NHWC with pixel stride y_pixel_stride (batch stride H*W*y_pixel_stride). */
typedef struct mtbt_node_args {
  mtbt_fuse_args fuse;
  const void* w;       /* [K][C] dtype */
  const float* shift;  /* [K] */
  void* y;
  int32_t y_pixel_stride;
  int32_t K;
  int32_t act;         /* MTBT_ACT_NONE .. MTBT_ACT_GELU_POLY */
} mtbt_node_args;
int mtbt_bifpn_node_nhwc(const mtbt_node_args* a, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Two back-to-back 1x1 convolutions on the same pixels as ONE launch (pw_chain.hip; inference, 16-bit storage):
 *   t[p][m] = round16( act1( (sum_c w1[m][c] * x[p][c]) * scale1[m] + shift1[m] ) )       m < 256, C = 256
 *   y[p][k] =          act2( (sum_m w2[k][m] * t[p][m]) * scale2[k] + shift2[k] )
 * t never reaches memory: it is rounded to the storage type exactly as mtbt_conv2d_nhwc stores it and becomes the second GEMM's operand in
 * LDS.  Every output element goes through the reduction order and the epilogue arithmetic of mtbt_conv2d_nhwc, so the result is BIT-IDENTICAL
 * to the two launches (tests/test_gpu_pw_chain.py).  Two families:
 *   out_dtype == dtype:    K = 256, act2 any of MTBT_ACT_NONE | SILU | ELU                      (BiFPN node conv -> C2f cv1)
 *   out_dtype == MTBT_F32: K <= 32, act2 = MTBT_ACT_NONE, scale2 = NULL (bias only)             (class branch cv3[i][1][1] -> cv3[i][2])
 * act1 is MTBT_ACT_SILU or MTBT_ACT_ELU.  x [pixels][256] dense; y: pixel p at y + p * y_pixel_stride (elements of out_dtype), K channels -- a
 * channel slice of a wider buffer is fine.  scale1 / scale2 may be NULL (= 1), shift1 / shift2 may be NULL (= 0).  Anything else returns
 * MTBT_EINVAL / MTBT_EALIGN before a launch. */
typedef struct mtbt_pw_chain_args {
  const void* x;        /* [pixels][256] dtype */
  const void* w1;       /* [256][256] dtype */
  const float* scale1;  /* [256] or NULL */
  const float* shift1;  /* [256] or NULL */
  const void* w2;       /* [K][256] dtype */
  const float* scale2;  /* [K] or NULL */
  const float* shift2;  /* [K] or NULL */
  void* y;
  int64_t pixels;
  int32_t y_pixel_stride;
  int32_t C;            /* 256 */
  int32_t M;            /* 256: width of the intermediate tensor */
  int32_t K;
  int32_t dtype;        /* MTBT_BF16 | MTBT_F16 */
  int32_t out_dtype;    /* dtype | MTBT_F32 */
  int32_t act1;
  int32_t act2;
} mtbt_pw_chain_args;
int mtbt_pw_chain_nhwc(const mtbt_pw_chain_args* a, void* stream);
/* What mtbt_pw_chain_nhwc would do with these arguments; nothing is launched, no pointer is dereferenced.  0: it has no kernel for them (the
 * entry point returns an error).  1: it has one and the fused launch is the faster form.  2: it has one, but at this pixel count the two
 * launches measured faster (a pixel-count rule; the entry point still runs the call).  A lowering asks this before it fuses a site. */
int mtbt_pw_chain_supported(const mtbt_pw_chain_args* a);
int mtbt_sizeof_pw_chain_args(void);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm2d forward with BATCH statistics + activation (module in train mode): the reference flips the
 * Detect/Segment heads to train mode inside forward(mode="train") (main_model.py:358-359), so their
 * BatchNorms use batch statistics and update running_mean/var (momentum, unbiased variance) -- SURVEY F14.
 *   y = act((x - mean_batch) / sqrt(var_batch + eps) * gamma + beta);  x, y dense NHWC [pixels][C] (y may alias x).
 * Deterministic two-pass statistics.  workspace >= mtbt_bn_train_workspace_bytes(pixels, C); on return its
 * last 2*C floats hold (mean, biased var).  running_mean / running_var may be NULL.
 * ------------------------------------------------------------------------------------------- */
int64_t mtbt_bn_train_workspace_bytes(int64_t pixels, int C);
int mtbt_bn_train_nhwc(const void* x, void* y, const float* gamma, const float* beta, float* running_mean,
                       float* running_var, float momentum, float eps, int act, int64_t pixels, int C, int dtype,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* Global average pool over H*W then Linear(C, nout) (main_model.py:333-334, :364). y [N,nout] f32. */
int mtbt_gap_fc(const void* x, const float* w, const float* b, float* y, int N, int HW, int C,
                int nout, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Box decode (running_main_v3.py:264-290, :510-533 ; ultralytics Detect._inference/DFL/dist2bbox).
 * Per level l: map [N,h_l,w_l,no] f32 NHWC with pixel stride `map_pixel_stride[l]`, no = 4*reg_max+nc.
 *   ltrb = softmax(16 bins) . arange(16);  anchor = (x+.5, y+.5)
 *   xyxy : boxes = (anchor -/+ ltrb) * stride[l]          (trainer decode)
 *   xywh : boxes = ((x1y1+x2y2)/2, x2y2-x1y1) * stride[l]  (Detect eval; stride may be 0)
 * Outputs (any may be NULL): boxes [N,A,4], scores = sigmoid(cls) [N,A,nc], best score [N,A],
 * best label [N,A] (first max, as torch.max), and `preds_cat` [N, A, cat_stride] row-major with
 * (box4, sigmoid cls) written at columns 0..4+nc-1 (the caller views it as [N,4+nc(+nm),A]).
 * ------------------------------------------------------------------------------------------- */
typedef struct mtbt_decode_args {
  const float* map[3];
  int32_t h[3], w[3];
  int32_t map_pixel_stride[3];
  float stride[3];
  int32_t n_levels, N, nc, reg_max;
  int32_t xywh; /* 0: xyxy, 1: xywh */
  float* boxes;
  float* scores;
  float* best_score;
  int32_t* best_label;
  float* preds_cat;
  int32_t cat_stride;
} mtbt_decode_args;

int mtbt_decode_boxes(const mtbt_decode_args* a, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-image confidence filter + clamp + greedy NMS + top-k (running_main_v3.py:535-552 calling
 * torchvision.ops.nms [upstream]).  One workgroup per image.  For image n:
 *   cand = { a : best_score[n,a] > conf_th } in ascending a   (the reference's boolean-mask order)
 *   boxes clamped to [0, clamp_max]; order = stable descending sort of scores;
 *   greedy: keep i; suppress j if inter/(area_i+area_j-inter) > iou_th  (fp32, no FMA contraction);
 *   stop after top_k kept.
 * Outputs per image (row stride top_k): keep_idx = index into `cand` (== torchvision's return value),
 * keep_anchor = a, out_boxes [top_k,4] (clamped), out_scores, out_labels; counts[n] = #kept;
 * n_cand[n] = |cand|.  workspace: >= mtbt_nms_workspace_bytes(N, A) bytes.
 * ------------------------------------------------------------------------------------------- */
int64_t mtbt_nms_workspace_bytes(int N, int A);
int mtbt_nms_batched(const float* boxes, const float* best_score, const int32_t* best_label, int N, int A,
                     float conf_th, float iou_th, float clamp_max, int top_k, int64_t* keep_idx,
                     int32_t* keep_anchor, float* out_boxes, float* out_scores, int64_t* out_labels,
                     int32_t* counts, int32_t* n_cand, void* workspace, int64_t workspace_bytes,
                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * Prototype x coefficient mask assembly (test_model.py:80-85 intended form) and the trainer's
 * proto projector (running_main_v3.py:186, :251-257; evaluate_model.py:160-171), one kernel:
 *   low[n,k,y,x] = sum_c coeff[n,k,c] * protos[n,y,x,c] (+ bias)
 *   up = bilinear resize of low to (Hout,Wout), align_corners=False
 *   logits (f32, may be NULL) = up ;  masks (u8, may be NULL) = sigmoid(up) > 0.5
 * protos [N,hp,wp,nm] f32 NHWC dense.  coeff element (n,k,c) at coeff + n*coeff_batch_stride +
 * k*coeff_k_stride + c*coeff_c_stride (so mc[N,A,nm] rows gathered through `gather_idx[n,k]`
 * (anchor index, may be NULL => k itself) need no copy; projector: batch stride 0, K=1).
 * Only k < counts[n] (counts may be NULL => K) is computed; padded slots k >= counts[n] are written as zeros.
 * ------------------------------------------------------------------------------------------- */
typedef struct mtbt_mask_args {
  const float* protos;
  const float* coeff;
  int64_t coeff_batch_stride, coeff_k_stride, coeff_c_stride;
  const int32_t* gather_idx; /* [N,K] or NULL */
  const int32_t* counts;     /* [N] or NULL */
  float bias;
  int32_t N, K, nm, hp, wp, Hout, Wout;
  float* logits;  /* [N,K,Hout,Wout] or NULL */
  uint8_t* masks; /* [N,K,Hout,Wout] or NULL */
} mtbt_mask_args;

int mtbt_mask_assemble(const mtbt_mask_args* a, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Instance masks and boxes in the ORIGINAL image frame, masks one bit per pixel: the inverse of the top-left letterbox
 * (dataset_btxrdv2.py:109-134) applied to the post-process results, one launch for up to 32 images of different sizes.
 * A frame is (height H0, width W0, scale = S / max(H0, W0) as the letterbox returned it); `step` = (float)((double)scale / up)
 * is the number of prototype pixels per frame pixel (up = S / wp letterboxed pixels per prototype pixel, 4 for the models).
 * SUPPORTED RANGE 0 < step <= 1: the image's long side is at least the prototype grid's (>= 160 px at S = 640); anything
 * else returns MTBT_EINVAL.
 *   boxes_frame[n,k] = clamp(boxes[n,k] / scale_n, 0, (W0, H0, W0, H0))   true fp32 division; rows k >= counts[n] are zeros
 *   low[n,k,y,x]     = sum_c coeff[n,k,c] * protos[n,y,x,c]
 *   logit(n,k,Y,X)   = bilinear tap of low at the ORIGINAL pixel (torch's align_corners=False rule, all fp32, no S x S plane):
 *                      sx = max((X + 0.5f) * step - 0.5f, 0); x0 = min((int)sx, wp-1); x1 = min(x0+1, wp-1); lx = clamp(sx - x0, 0, 1);
 *                      the same for y with hp; v = (1-ly)*((1-lx)*low[y0,x0] + lx*low[y0,x1]) + ly*((1-lx)*low[y1,x0] + lx*low[y1,x1])
 *   bit(n,k,Y,X)     = v > 0, and with `crop` additionally x1f <= X < x2f && y1f <= Y < y2f of boxes_frame[n,k] (ultralytics crop_mask)
 * Packed layout: plane k of image n is H0 rows of pitch = 8 * ceil(W0 / 64) bytes at out + offset_n + k * H0 * pitch; pixel X is
 * bit X & 7 of byte X >> 3 (numpy.packbits(bitorder="little")); padding bits X >= W0 are 0; planes k >= counts[n] are zero.
 * EVERY byte of every plane is written by the launch (the buffer may be uninitialised); image n occupies K * H0 * pitch bytes,
 * e.g. 113 MB for a 3000 x 3000 image at K = 100 -- lower top_k for large images.
 * protos / coeff / gather_idx / counts as in mtbt_mask_args (nm must be 32); boxes [N,K,4] xyxy in letterboxed pixels (may be NULL
 * when neither crop nor boxes_frame is wanted); boxes_frame [N,K,4] or NULL.  The frame descriptors are read on the host and
 * travel in the kernel arguments: no copy, no synchronisation.
 * MTBT_EINVAL before any launch: NULL a / frames / protos / coeff / out, n_frames outside 1..32 or != N, step outside (0, 1],
 * pitch != 8 * ceil(width / 64), offset not a multiple of 16, a plane range past out_bytes, nm != 32, crop or boxes_frame without
 * boxes.  MTBT_EALIGN for protos / out not 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
typedef struct mtbt_frame {
  int32_t height, width; /* H0, W0 of the original image */
  float step;            /* prototype pixels per frame pixel: (float)((double)scale / up) */
  float scale;           /* the letterbox scale S / max(H0, W0): divides the boxes */
  int32_t pitch;         /* bytes per packed row: 8 * ceil(width / 64) */
  int32_t reserved;
  int64_t offset;        /* byte offset of this image's K planes in `out`, a multiple of 16 */
} mtbt_frame;

typedef struct mtbt_frame_mask_args {
  const float* protos;
  const float* coeff;
  int64_t coeff_batch_stride, coeff_k_stride, coeff_c_stride;
  const int32_t* gather_idx; /* [N,K] or NULL */
  const int32_t* counts;     /* [N] or NULL */
  const float* boxes;        /* [N,K,4] letterboxed xyxy, or NULL */
  float* boxes_frame;        /* [N,K,4] or NULL */
  uint8_t* out;              /* packed planes of all images */
  int64_t out_bytes;
  int32_t N, K, nm, hp, wp;
  int32_t crop;
} mtbt_frame_mask_args;

int mtbt_masks_to_frames(const mtbt_frame_mask_args* a, const mtbt_frame* frames, int n_frames, void* stream);
/* sizeof() of the two structs above as the library was compiled: which = 0 mtbt_frame, 1 mtbt_frame_mask_args; -1 otherwise */
int mtbt_sizeof_frame_args(int which);

/* ---------------------------------------------------------------------------------------------
 * Weighted boxes fusion (Solovyev, Wang, Gabruseva 2021, "avg" confidence with the count correction) of M detection lists of the same
 * N images: the views of test-time augmentation, the models of an ensemble.  The reference has NO counterpart; this arithmetic is the
 * project's own definition (tests/fuse_reference.py restates it in numpy).  One launch, one workgroup per image, no host
 * synchronisation, deterministic; every fp32 operation is a separate correctly rounded one (no FMA contraction), in the order written.
 * Source m (0 <= m < n_sources = M <= 8) is exactly what mtbt_nms_batched writes, never modified: boxes[m] [N,K,4] xyxy in the img_size
 * frame of that source's VIEW, scores[m] [N,K], labels[m] int64 [N,K], counts[m] int32 [N], anchors[m] int32 [N,K] or NULL;
 * orient[m] is the view's code as in mtbt_augment_batch (bit 0 flips x, bit 1 flips y, bit 2 transposes), weight[m] > 0.
 * N, K are the same for every source, M * K <= 4096.  For image n, S = img_size:
 *   1. candidates, m ascending then k ascending below min(counts[m][n], K):  s = scores[m][n,k] * weight[m], kept iff s > skip_thr;
 *      index c = m K + k.  The box is un-oriented as two corner points (the continuous form of the augmentation's pixel rule):
 *      x <- S - x on both x if bit 0; y <- S - y on both y if bit 1; then x <-> y if bit 2; then each axis re-sorted to (min, max).
 *   2. order: ascending 64-bit keys ~orderable(s) << 32 | c  (the NMS key: stable descending s, ties to ascending c).
 *   3. greedy clustering in that order.  For candidate j and every existing cluster of the same label, in ascending cluster index:
 *      ovr = inter / (area_i + area_j - inter) of the NMS, i = the cluster's current fused box, j = the candidate's box.  The winner is
 *      the largest ovr (best starts at -inf, a cluster wins iff ovr > best: a NaN never wins, ties stay with the lowest index).
 *      best > iou_thr: j JOINS the winner:  Ss += s;  Sx1 += s * x1 (multiply, then add; the same for y1, x2, y2);  n += 1;
 *                      fused = (Sx1 / Ss, Sy1 / Ss, Sx2 / Ss, Sy2 / Ss).
 *      otherwise j OPENS the next cluster:  Ss = s;  Sx1 = s * x1, ...;  n = 1;  fused = the box itself (copied, not divided);
 *                      label = j's label;  lead = c  (the leader is the highest-scoring member).  No cap on the clusters below M K.
 *   4. cluster score = ((Ss / (float)n) * (float)min(n, M)) / W,  W = weight[0] + weight[1] + ... (m ascending, fp32).  Members of
 *      one source may share a cluster, hence the min.
 *   5. output order: ascending keys ~orderable(score) << 32 | cluster index (stable descending score); the first top_k, row stride
 *      top_k:  out_boxes [N,top_k,4] (fused), out_scores, out_labels (int64), n_members (n), lead_source = lead / K, lead_slot =
 *      lead % K, lead_anchor = anchors[lead_source][n, lead_slot] (optional: NULL, and it must be NULL when any anchors[m] is NULL);
 *      out_counts[n] = min(#clusters, top_k), n_clusters[n] = #clusters before the cut.  Padded slots as mtbt_nms_batched pads:
 *      boxes and scores 0, labels -1; lead_source / lead_slot / lead_anchor -1; n_members 0.
 * workspace: >= mtbt_fuse_workspace_bytes(M, N, K) bytes, 16-byte aligned (0 is returned for arguments the launch would refuse).
 * Order of the checks: MTBT_EINVAL before any launch for NULL a, M outside 1..8, N < 0, K < 1, M K > 4096, top_k < 1, img_size not > 0,
 * an orient outside 0..7, a weight not > 0 (NaN included); then N == 0 is MTBT_OK with nothing launched; then MTBT_EINVAL for a NULL
 * required pointer (every source array but anchors, every output but lead_anchor, workspace), lead_anchor without every anchors[m], a
 * workspace that is too small; then MTBT_EALIGN for boxes[m] / out_boxes / workspace not 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define MTBT_FUSE_MAX_SOURCES 8
#define MTBT_FUSE_MAX_CANDIDATES 4096
typedef struct mtbt_box_fuse_args {
  const float* boxes[MTBT_FUSE_MAX_SOURCES];
  const float* scores[MTBT_FUSE_MAX_SOURCES];
  const int64_t* labels[MTBT_FUSE_MAX_SOURCES];
  const int32_t* counts[MTBT_FUSE_MAX_SOURCES];
  const int32_t* anchors[MTBT_FUSE_MAX_SOURCES]; /* each [N,K] or NULL */
  int32_t orient[MTBT_FUSE_MAX_SOURCES];
  float weight[MTBT_FUSE_MAX_SOURCES];
  int32_t n_sources, N, K, top_k;
  float img_size, iou_thr, skip_thr;
  int32_t reserved;
  float* out_boxes;
  float* out_scores;
  int64_t* out_labels;
  int32_t* out_counts;
  int32_t* n_clusters;
  int32_t* n_members;
  int32_t* lead_source;
  int32_t* lead_slot;
  int32_t* lead_anchor; /* [N,top_k] or NULL */
  void* workspace;
  int64_t workspace_bytes;
} mtbt_box_fuse_args;

int64_t mtbt_fuse_workspace_bytes(int n_sources, int N, int K);
int mtbt_fuse_detections(const mtbt_box_fuse_args* a, void* stream);
/* sizeof(mtbt_box_fuse_args) as the library was compiled (mtbt_fuse_args is the BiFPN fusion node's struct, above) */
int mtbt_sizeof_box_fuse_args(void);
/* mtbt_fuse_detections plus the MEMBERSHIP of the clusters: the same kernel, the same checks in the same order, every output above
 * bit-identical (mtbt_fuse_detections is the member_slot == NULL path of this code; the struct, its sizeof and the workspace do not
 * change).  member_slot int32 [N, M*K]: for candidate c = m K + k the output row r < out_counts[n] of the cluster it opened or joined;
 * -1 for a slot that is no candidate (k >= counts[m][n], s <= skip_thr) and for a member of a cluster that top_k cut.  Every element is
 * written.  A NULL member_slot is MTBT_EINVAL (checked with the required pointers, after the N == 0 return). */
int mtbt_fuse_detections_members(const mtbt_box_fuse_args* a, int32_t* member_slot, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Instance masks of FUSED detections, voted over the members of each cluster (test-time augmentation, ensembles): the sign of the
 * score-weighted mean logit of the members at prototype resolution, upright, then sampled as mtbt_masks_to_frames samples.  The
 * reference has NO counterpart; this is the project's own definition (tests/vote_reference.py restates it).  Sources m < n_sources = M
 * <= 8 are the ones mtbt_fuse_detections_members fused: scores[m] [N,K], anchors[m] int32 [N,K] (the NMS keep_anchor), weight[m],
 * orient[m]; mc[m] the source's mask coefficients, element (n, channel c, anchor a) at mc[m][n * mc_batch_stride[m] + a *
 * mc_k_stride[m] + c * mc_c_stride[m]]; protos[m] [N,G,G,32] fp32 NHWC in the frame of the source's VIEW (hp == wp == G, nm == 32);
 * member_slot int32 [N, M*K] as mtbt_fuse_detections_members writes it; counts [N], boxes [N,top_k,4] the FUSED list (upright).
 * For image n and fused row r < min(counts[n], top_k), members c = m K + k with member_slot[n,c] == r, s_c = scores[m][n,k] * weight[m]:
 *   Ss[n,r]      = sum of s_c over the members, m ascending then k ascending (starting from the first member's s_c)
 *   W[n,r,m,:]   = (sum over the members c of source m, k ascending, of s_c * coeff_c[:]) / Ss[n,r],  coeff_c = mc[m][n, :, anchors[m][n,k]]
 *                  fp32; multiply, then add (the sum starts at 0); ONE true division at the end; no FMA contraction
 *   low[n,r,y,x] = sum over m ascending, c ascending of W[n,r,m,c] * U_m[n,y,x,c]                  (fp32 MFMA, 4 terms per step)
 *   U_m          = protos[m] turned upright (postprocess.unorient_batch at the G x G grid):
 *                  U_m[y,x] = P_m[fy(a), fx(b)],  (a,b) = (x,y) if orient bit 2 else (y,x),  fy(a) = G-1-a if bit 1,  fx(b) = G-1-b if bit 0
 *   bit(n,r,Y,X) = bilinear tap of low at the frame pixel > 0 (and inside boxes_frame[n,r] with `crop`)
 * Rows r >= counts[n] of W and Ss and (row, source) pairs without a member are zeros.  W float [N,top_k,M,32] and Ss float [N,top_k] are
 * caller-provided and fully written (one small deterministic launch), then one mask launch reads W.  Everything from the bilinear tap
 * on -- frame descriptors, step range, boxes_frame = clamp(boxes / scale), the crop rule, the packed layout with K = top_k planes per
 * image, zero planes for r >= counts[n], zero padding bits, every byte written -- is mtbt_masks_to_frames' contract, above.
 * Linear up to W: one vote costs one coefficient row per (row, source), not one mask per member.
 * MTBT_EINVAL before any launch: NULL a / frames / out / member_slot / counts / W / Ss, M outside 1..8, n_frames outside 1..32 or != N,
 * nm != 32, K < 1, M K > 4096, top_k outside 1..65535, hp < 1, hp != wp, out_bytes < 0, an orient outside 0..7, a NULL protos[m] / mc[m]
 * / anchors[m] / scores[m] for m < M, crop or boxes_frame without boxes, then the frame descriptor checks of mtbt_masks_to_frames.
 * MTBT_EALIGN for a protos[m] / out not 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
typedef struct mtbt_vote_mask_args {
  const float* protos[MTBT_FUSE_MAX_SOURCES];
  const float* mc[MTBT_FUSE_MAX_SOURCES];
  int64_t mc_batch_stride[MTBT_FUSE_MAX_SOURCES], mc_k_stride[MTBT_FUSE_MAX_SOURCES], mc_c_stride[MTBT_FUSE_MAX_SOURCES];
  const int32_t* anchors[MTBT_FUSE_MAX_SOURCES];
  const float* scores[MTBT_FUSE_MAX_SOURCES];
  float weight[MTBT_FUSE_MAX_SOURCES];
  int32_t orient[MTBT_FUSE_MAX_SOURCES];
  const int32_t* member_slot; /* [N, M*K] */
  const int32_t* counts;      /* [N] fused */
  const float* boxes;         /* [N,top_k,4] fused, letterboxed upright xyxy, or NULL */
  float* boxes_frame;         /* [N,top_k,4] or NULL */
  float* W;                   /* [N,top_k,M,32] */
  float* Ss;                  /* [N,top_k] */
  uint8_t* out;               /* packed planes of all images, top_k per image */
  int64_t out_bytes;
  int32_t n_sources, N, K, top_k, nm, hp, wp, crop;
} mtbt_vote_mask_args;

int mtbt_vote_masks(const mtbt_vote_mask_args* a, const mtbt_frame* frames, int n_frames, void* stream);
int mtbt_sizeof_vote_mask_args(void);

/* ---------------------------------------------------------------------------------------------
 * Sliced inference: the model runs on overlapping S x S windows (tiles) of a large image at or near native resolution, plus the whole
 * image once, and the per-tile results are merged in the image's own pixel frame.  The reference has NO counterpart; this arithmetic is
 * the project's own definition (tests/slice_reference.py restates it).  Every fp32 operation below is one correctly rounded operation in
 * the order written (no FMA contraction).
 *
 * TILES.  A pass over image (H0, W0) at zoom z resizes it to R with new = max(1, (int)(dim * z)) per axis (the letterbox's rule; R is
 * never materialised).  A tile is the S x S canvas showing R[oy:oy+S, ox:ox+S], 114/255 pad beyond R: mtbt_augment_batch with the
 * geometry row (new_w, new_h, -ox, -oy, 0, 0, 0, 0) and no table.  ox, oy are multiples of up = S / G (4 for the models), so the tile's
 * prototype grid sits at the integer offset (pox, poy) = (ox / up, oy / up) of R's virtual prototype grid.  Its descriptor:
 *   image            index of the image (within the call) the tile belongs to; the tiles of an image are consecutive
 *   pox, poy         >= 0
 *   wx0,wy0,wx1,wy1  the frame WINDOW, half-open, clamped to the image: the frame pixels X whose centre (X + 0.5) * z lies in
 *                    [ox, min(ox + S, new_w)), the same in y (computed by the host in double); the tile that reaches the end of the
 *                    resized axis (ox + S >= new_w) takes the pixels up to the image's edge, since (int)(dim * z) may cut the last centre off
 *   height, width    H0, W0 of the image
 *   step, scale      step = (float)(z / up), 0 < step <= 1 prototype pixels per frame pixel;  scale = (float)z
 *   fox, foy         (float)ox, (float)oy
 * The whole-image pass is the tile z = S / max(H0, W0), ox = oy = 0, window = the image: for it everything below reduces to
 * mtbt_masks_to_frames / its boxes_frame bit for bit.
 *
 * MERGING (mtbt_merge_tiles): one launch, one workgroup per image, no host synchronisation, deterministic.  Sources are exactly what
 * mtbt_nms_batched writes for a batch of NT tiles: boxes [NT,K,4] xyxy in each tile's canvas, scores [NT,K], labels int64 [NT,K],
 * counts int32 [NT], anchors int32 [NT,K] or NULL.  Image n owns tiles [first[n], first[n+1]), T_n = first[n+1] - first[n] <= 64 and
 * T_n K <= 4096; first[0] = 0, first[N] = NT.
 *   1. candidates: (tile t, slot k < min(counts[t], K)) with score s > skip_thr; index within the image c = (t - first[n]) K + k.
 *      Component v of its FRAME box is clamp((v + off) / scale_t, 0, hi): one add, then one true division; off = fox_t | foy_t,
 *      hi = W0 | H0.
 *   2. order: ascending keys ~orderable(s) << 32 | c (the NMS / fusion key: stable descending s, ties to ascending c).
 *   3. greedy non-maximum MERGING in that order.  A candidate i not yet absorbed opens the next row; every later, not yet absorbed
 *      candidate j with the same label (any label with class_agnostic) and metric(box_i, box_j) > thr is absorbed into it.  box_i is i's
 *      OWN frame box, never the growing union.  With area_x = (x2 - x1) * (y2 - y1), inter = max(0, min(x2) - max(x1)) * max(0, min(y2) -
 *      max(y1)) as the NMS computes them:
 *        metric 0 (IoU)  inter / ((area_i + area_j) - inter)
 *        metric 1 (IoS)  inter / fminf(area_i, area_j)          (intersection over the smaller: a part is absorbed by the whole)
 *      A NaN never matches.  The row's box is the union of its members' frame boxes (min / max), its score and label the leader's.
 *      The loop stops after top_k rows.
 *   4. outputs, row stride top_k, padded as mtbt_nms_batched pads (boxes and scores 0, labels -1, lead_* -1, n_members 0):
 *      out_boxes [N,top_k,4] in FRAME pixels, out_scores, out_labels int64, out_counts [N], n_members, lead_tile (index into the tile
 *      table), lead_slot, lead_anchor (optional; needs anchors), member_slot int32 [NT,K] (the row the slot opened or joined, -1
 *      otherwise; every element is written), n_left [N] (candidates neither leading nor absorbed when the loop stopped: > 0 iff top_k cut).
 * `tiles` is a HOST copy of the tile table (validated, never dereferenced on the device), `tiles_dev` the caller's DEVICE copy of the
 * same NT descriptors (read by the kernels); `first` is a host array.  No allocation and no synchronisation inside the library.
 * Order of the checks: MTBT_EINVAL before any launch for NULL a, N < 0, K < 1, top_k < 1, a metric outside 0..1, a NaN thr or skip_thr;
 * then N == 0 is MTBT_OK with nothing launched; then MTBT_EINVAL for a NULL required pointer (boxes, scores, labels, counts, tiles,
 * tiles_dev, first, every output but lead_anchor), lead_anchor without anchors, a bad `first` (first[0] != 0, decreasing, T_n > 64,
 * T_n K > 4096, first[N] != n_tiles), a bad descriptor (image != n, negative pox / poy, an empty or out-of-image window, step outside
 * (0, 1], scale not > 0, a NaN or negative fox / foy, height or width < 1 or not the same for every tile of the image, reserved != 0);
 * then MTBT_EALIGN for boxes / out_boxes not 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define MTBT_TILE_MAX_PER_IMAGE 64
#define MTBT_MERGE_IOU 0
#define MTBT_MERGE_IOS 1
typedef struct mtbt_tile {
  int32_t image;
  int32_t pox, poy;
  int32_t wx0, wy0, wx1, wy1;
  int32_t height, width;
  int32_t reserved;
  float step, scale;
  float fox, foy;
} mtbt_tile;

typedef struct mtbt_tile_merge_args {
  const float* boxes;       /* [NT,K,4] */
  const float* scores;      /* [NT,K] */
  const int64_t* labels;    /* [NT,K] */
  const int32_t* counts;    /* [NT] */
  const int32_t* anchors;   /* [NT,K] or NULL */
  const mtbt_tile* tiles;     /* HOST [NT] */
  const mtbt_tile* tiles_dev; /* DEVICE [NT] */
  const int32_t* first;     /* HOST [N+1] */
  int32_t N, n_tiles, K, top_k;
  int32_t metric, class_agnostic;
  float thr, skip_thr;
  float* out_boxes;
  float* out_scores;
  int64_t* out_labels;
  int32_t* out_counts;
  int32_t* n_members;
  int32_t* lead_tile;
  int32_t* lead_slot;
  int32_t* lead_anchor;     /* [N,top_k] or NULL */
  int32_t* member_slot;     /* [NT,K] */
  int32_t* n_left;          /* [N] */
} mtbt_tile_merge_args;

int mtbt_merge_tiles(const mtbt_tile_merge_args* a, void* stream);

/* Instance masks of MERGED rows, voted across the tiles of their members straight into the bit-packed frame planes
 * (mtbt_vote_tile_masks).  For merged row r < min(counts[n], top_k) of image n, members c = (tile t, slot k) with member_slot[t,k] == r,
 * s_c = scores[t,k], tl = t - first[n]:
 *   Ss[n,r]      = sum of s_c over the members, c ascending (fp32 adds from 0)
 *   W[n,r,tl,:]  = (sum over row r's members in tile t, k ascending, of s_c * coeff_c[:]) / Ss[n,r]      coeff_c = mc[t, :, anchors[t,k]];
 *                  multiply, then add from 0, ONE true division; (row, tile) pairs without a member, rows r >= counts[n] and tl >= T_n: 0
 *   low_t        = W[n,r,tl,:] . P_t            (fp32 MFMA, 4 terms per step; P_t = protos[t] [G,G,32], tile-major NHWC)
 *   tap_t(Y,X)   : sx = max(((float)X + 0.5f) * step_t - 0.5f - (float)pox_t, 0), then exactly mtbt_masks_to_frames' rule against G:
 *                  x0 = min((int)sx, G-1); x1 = min(x0+1, G-1); lx = clamp(sx - x0, 0, 1); the same in y with poy_t; its bilinear form
 *   v(Y,X)       = sum, tiles t ascending, over the tiles with a member in r whose window holds (X, Y), of tap_t   (fp32 adds from 0)
 *   bit          = v > 0, and with `crop` also x1 <= X < x2 && y1 <= Y < y2 of boxes[n,r] (the merged union box, frame pixels)
 * Pixels that no member tile sees are 0.  The packed layout, the mtbt_frame descriptors (<= 32 images per call; their height, width,
 * pitch and offset are read, step and scale are ignored), K = top_k planes per image, zero planes for r >= counts[n], zero padding bits
 * and "every byte written exactly once" are mtbt_masks_to_frames' contract.  No atomics, no memset.  W float [N,top_k,Tmax,32] and Ss
 * float [N,top_k] are caller-provided and fully written by one small launch (serial sums in the stated order); Tmax >= every T_n.
 * `tiles` (HOST) / `tiles_dev` (DEVICE) / `first` (HOST [N+1], absolute indices into the tile table; first[0] may be > 0 here) as above.
 * MTBT_EINVAL before any launch: NULL a / frames / out / member_slot / counts / W / Ss / protos / mc / anchors / scores / tiles /
 * tiles_dev / first, n_frames outside 1..32 or != N, nm != 32, K < 1, top_k outside 1..65535, hp < 1, hp != wp, Tmax outside 1..64,
 * out_bytes < 0, crop without boxes, a bad `first` (first[0] < 0, decreasing, T_n > Tmax, T_n K > 4096, first[N] > n_tiles), a bad
 * descriptor (as above, except `image`; height / width must equal the frame's), then the frame descriptor checks of
 * mtbt_masks_to_frames.  MTBT_EALIGN for protos / out not 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
typedef struct mtbt_tile_mask_args {
  const float* protos;        /* [NT,G,G,32] */
  const float* mc;            /* element (t, channel c, anchor a) at mc[t * mc_batch_stride + a * mc_k_stride + c * mc_c_stride] */
  int64_t mc_batch_stride, mc_k_stride, mc_c_stride;
  const int32_t* anchors;     /* [NT,K] */
  const float* scores;        /* [NT,K] */
  const int32_t* member_slot; /* [NT,K] */
  const int32_t* counts;      /* [N] merged */
  const float* boxes;         /* [N,top_k,4] merged, frame pixels, or NULL */
  const mtbt_tile* tiles;     /* HOST [n_tiles] */
  const mtbt_tile* tiles_dev; /* DEVICE [n_tiles] */
  const int32_t* first;       /* HOST [N+1] */
  float* W;                   /* [N,top_k,Tmax,32] */
  float* Ss;                  /* [N,top_k] */
  uint8_t* out;               /* packed planes of all images, top_k per image */
  int64_t out_bytes;
  int32_t N, n_tiles, K, top_k, Tmax, nm, hp, wp, crop, reserved;
} mtbt_tile_mask_args;

int mtbt_vote_tile_masks(const mtbt_tile_mask_args* a, const mtbt_frame* frames, int n_frames, void* stream);
/* sizeof() of the three structs above as the library was compiled: which = 0 mtbt_tile, 1 mtbt_tile_merge_args, 2 mtbt_tile_mask_args;
 * -1 otherwise */
int mtbt_sizeof_tile_args(int which);

/* ---------------------------------------------------------------------------------------------
 * The SEMANTIC mask in the original image frame (mtbt_seg_to_frames): the trainer's seg_proto_projector (a 1x1 conv over the 32
 * prototypes, running_main_v3.py:186, :251-257) averaged over several forward passes -- the views of test-time augmentation, the
 * models of an ensemble, the tiles of sliced inference -- and sampled at the image's own pixels, one bit per pixel and optionally the
 * averaged logit itself.  The reference has NO counterpart of the averaging; this arithmetic is the project's own definition
 * (tests/seg_frame_reference.py restates it).  Every fp32 operation below is one correctly rounded operation in the order written (no
 * FMA contraction).
 *
 * SOURCES.  Image n owns sources s in [first[n], first[n+1]), at most 64 (MTBT_TILE_MAX_PER_IMAGE).  A source is one forward pass over
 * one window of the image:
 *   tiles[s]      its mtbt_tile descriptor exactly as sliced inference writes it (window wx0..wy1, step, pox, poy, height, width).  A
 *                 whole-image pass (a TTA view, an ensemble member) is the descriptor of the full view: window = the frame, pox = poy = 0,
 *                 step = the frame's
 *   sources[s]    pass, slot: its prototypes P_s = protos[pass] + slot * G * G * 32, fp32 NHWC [G, G, 32] in the frame of its own VIEW
 *                 (hp == wp == G, nm == 32); pass < n_passes <= 64, slot < pass_items[pass]
 *                 orient 0..7: the dihedral view the pass saw, codes as in mtbt_augment_batch;  weight > 0;
 *                 proj: row of the projector table q float [n_proj, 33], 32 weights then the bias;  blend 0 or 1
 * LAUNCH 1, the projector at prototype resolution, into the caller's fp32 workspace [n_sources, G, G] (source s at s * G * G):
 *   L_s[y,x] = (((0 + q[j,0] * P_s[y,x,0]) + q[j,1] * P_s[y,x,1]) + ... + q[j,31] * P_s[y,x,31]) + q[j,32]          j = proj_s
 *   a serial fp32 sum, c ascending, multiply then add, the bias last (NOT the MFMA order of the instance kernels).
 * LAUNCH 2, the blend into the frame.  For frame pixel (X, Y) of image n, over the sources s ascending whose window holds (X, Y), with
 * num = den = 0 at the start:
 *   (x0, x1, lx) = mtbt_vote_tile_masks' tap of X with step_s, pox_s against G;  (y0, y1, ly) likewise with poy_s
 *   U_s[y,x]     = L_s[fy(a), fx(b)],  (a,b) = (x,y) if orient bit 2 else (y,x),  fy(a) = G-1-a if bit 1,  fx(b) = G-1-b if bit 0
 *                  (mtbt_vote_masks' upright rule)
 *   tap          = (1-ly)*((1-lx)*U[y0,x0] + lx*U[y0,x1]) + ly*((1-lx)*U[y1,x0] + lx*U[y1,x1])
 *   bx           = blend_s ? (1-lx)*tab[x0] + lx*tab[x1] : 1.f;   by likewise with y;   w = weight_s * (bx * by)
 *   num = num + w * tap;   den = den + w
 *   v   = den > 0 ? num / den (one true division) : 0;      bit = den > 0 && v > threshold
 * `tab` float [G]: the blend window along one axis of a tile's upright prototype grid, every entry finite and > 0; NULL is allowed
 * when no source has blend = 1.  A pixel that no source sees has v = 0 and bit = 0.
 * OUTPUTS.  One packed plane per image under the mtbt_frame descriptors (K = 1; height, width, pitch, offset are read, step and scale
 * ignored, as in mtbt_vote_tile_masks); mtbt_masks_to_frames' layout contract holds: little-endian bits, zero padding bits, every byte
 * written exactly once, no memset, no atomics.  With `logits` != NULL also v as dense fp32 [H0, W0], image n at logits +
 * logits_offset[n] floats (a multiple of 4, the image inside logits_floats); every element is written.
 * `sources` / `tiles` / `tab` are HOST copies (validated, never dereferenced on the device), `sources_dev` / `tiles_dev` / `tab_dev` the
 * caller's DEVICE copies of the same (read by the kernels); `first` is a host array of absolute indices into the tables (first[0] may be
 * > 0).  A call projects and blends the sources first[0] .. first[N] - 1 only.  No allocation and no synchronisation inside the library.
 * mtbt_seg_frame_workspace_bytes(n_sources, G) = 4 n_sources G^2 (0 for arguments the launch would refuse).
 * Order of the checks, all MTBT_EINVAL before any launch: NULL a / frames / proj / sources / sources_dev / tiles / tiles_dev / first /
 * workspace / out; n_passes outside 1..64, a NULL protos[p] or pass_items[p] < 1 for p < n_passes; n_frames outside 1..32 or != N; nm != 32,
 * hp < 1, hp != wp, n_proj < 1, reserved != 0; a bad `first` (first[0] < 0, decreasing, more than 64 sources for an image, past
 * n_sources); per source: a pass or slot outside the passes, an orient outside 0..7, a weight not > 0 (NaN included) or infinite, proj
 * outside the table, a blend not 0 or 1 or blend = 1 without tab and tab_dev, reserved != 0; a tab entry (tab given) that is not finite and
 * > 0; a NaN threshold; a workspace that is too
 * small; a bad tile descriptor (as mtbt_vote_tile_masks; height / width must equal the frame's); the frame descriptor checks of
 * mtbt_masks_to_frames with K = 1; a logits_offset that is negative, no multiple of 4 or whose image leaves logits_floats.  Then
 * MTBT_EALIGN for a protos[p] / out / workspace / logits not 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define MTBT_SEG_MAX_PASSES 64
typedef struct mtbt_seg_source {
  int32_t pass, slot;
  int32_t orient, proj, blend;
  float weight;
  int32_t reserved[2];
} mtbt_seg_source;

typedef struct mtbt_seg_frame_args {
  const float* protos[MTBT_SEG_MAX_PASSES];   /* DEVICE, pass p: [pass_items[p], G, G, 32] */
  int32_t pass_items[MTBT_SEG_MAX_PASSES];
  const float* proj;                  /* DEVICE [n_proj, 33] */
  const mtbt_seg_source* sources;     /* HOST [n_sources] */
  const mtbt_seg_source* sources_dev; /* DEVICE [n_sources] */
  const mtbt_tile* tiles;             /* HOST [n_sources] */
  const mtbt_tile* tiles_dev;         /* DEVICE [n_sources] */
  const int32_t* first;               /* HOST [N+1] */
  const float* tab;                   /* HOST [G] or NULL */
  const float* tab_dev;               /* DEVICE [G] or NULL */
  float* workspace;                   /* DEVICE [n_sources, G, G] */
  int64_t workspace_bytes;
  uint8_t* out;                       /* packed planes of all images, one per image */
  int64_t out_bytes;
  float* logits;                      /* DEVICE or NULL */
  int64_t logits_floats;
  int64_t logits_offset[32];          /* floats, image n of this call */
  float threshold;
  int32_t N, n_sources, n_passes, n_proj, nm, hp, wp, reserved;
} mtbt_seg_frame_args;

int mtbt_seg_to_frames(const mtbt_seg_frame_args* a, const mtbt_frame* frames, int n_frames, void* stream);
int64_t mtbt_seg_frame_workspace_bytes(int n_sources, int G);
/* sizeof() of the two structs above as the library was compiled: which = 0 mtbt_seg_source, 1 mtbt_seg_frame_args; -1 otherwise */
int mtbt_sizeof_seg_frame_args(int which);

/* ---------------------------------------------------------------------------------------------
 * Multitask loss VALUE (forward only), MultiTaskLitModel._multitask_loss, running_main_v3.py:232-387:
 *   per (image, anchor): trainer decode (:268-290), IoU against the image's GT boxes (:316), positives = max IoU >
 *   iou_thresh (:319-321), sum(1 - IoU) (:331), BCE-with-logits(sum) of the class logits against one-hot /
 *   label-smoothed targets (:334-346), two-bin DFL cross-entropy (:351-367); segmentation BCE-with-logits (mean over
 *   seg_n logits, :257); image-classification cross-entropy (:237); normalisation by the batch's positive count (batch
 *   size if none, :371) and the weighted total (:377-383).
 * map[l]: raw Detect maps [N,h_l,w_l,4*reg_max+nc] f32 NHWC (pixel stride map_pixel_stride[l]).  GT boxes grouped by image:
 * gt_xyxy [G][4] pixels, gt_cls [G], gt_off [N+1] (image n owns [gt_off[n], gt_off[n+1])).  seg_logits / seg_targets:
 * seg_n floats each (may be NULL with seg_n = 0); *seg_bias (device scalar, optional) is added to every seg logit.  img_logits [N][n_img_classes] f32, img_gt [N] int64.
 * out[8] = total, seg, box, dfl, cls_det, img_cls, #positives, mean matched IoU.  Deterministic; no host synchronisation.
 * ------------------------------------------------------------------------------------------- */
typedef struct mtbt_loss_args {
  const float* map[3];
  int32_t h[3], w[3];
  int32_t map_pixel_stride[3];
  int32_t n_levels, N, nc, reg_max;
  float img_size;
  const float* gt_xyxy;
  const int32_t* gt_cls;
  const int32_t* gt_off;
  float iou_thresh, label_smoothing;
  int32_t training; /* label smoothing applies in training mode only (:337) */
  const float* seg_logits;
  const float* seg_targets;
  const float* seg_bias; /* optional device scalar added to every seg logit (the projector's bias), may be NULL */
  int64_t seg_n;
  const float* img_logits;
  const int64_t* img_gt;
  int32_t n_img_classes;
  float w_seg, w_box, w_dfl, w_cls, w_img;
  float* workspace;
  int64_t workspace_bytes; /* >= mtbt_loss_workspace_bytes(N, A, seg_n) */
  float* out;
} mtbt_loss_args;

int64_t mtbt_loss_workspace_bytes(int N, int A, int64_t seg_n);
int mtbt_multitask_loss(const mtbt_loss_args* a, void* stream);

/* Gradient of out[0] (the weighted total) with respect to the head outputs the loss reads -- what `total_loss.backward()` hands
 * to the heads in `training_step` (running_main_v3.py:421-447), the first operator of the backward pass.  Call after
 * mtbt_multitask_loss with the SAME args on the same stream (the batch's positive count is read from a->out[6]).
 * d_map[l]: [N,h_l,w_l,4*reg_max+nc] f32 NHWC, pixel stride d_map_pixel_stride[l]; every element is written (zeros for anchors
 * that are not positives).  d_seg_logits: seg_n floats (required when seg_n > 0) = w_seg / seg_n * (sigmoid - target);
 * d_img_logits [N][n_img_classes] (may be NULL) = w_img / N * (softmax - onehot).  The positives mask, the matched GT index and
 * the DFL targets carry no gradient, exactly as in autograd. */
int mtbt_multitask_loss_grad(const mtbt_loss_args* a, float* const* d_map, const int32_t* d_map_pixel_stride, float* d_seg_logits,
                             float* d_img_logits, void* stream);

/* Confusion matrices of the validation epoch (running_main_v3.py:193-195 image classes, :218 + :349-350 + :710-722 matched anchors).
 * counts [nc][nc] int64, row = target, column = prediction (torchmetrics' layout); the kernels ADD to it (the caller zeroes it once).
 * pred = argmax of the nc logits with torch semantics: the first maximum wins and a NaN counts as the maximum.  A target outside
 * [0, nc) is not counted and sets bit 0 of *status (the caller zeroes it).  Integer sums per workgroup in LDS, then one global atomic
 * add per non-zero bin: deterministic.  nc <= MTBT_CONFUSION_MAX_NC.  MTBT_EINVAL before any launch for NULL pointers, N < 1,
 * nc < 1 or nc above the cap.  Asynchronous, no workspace.
 *
 * mtbt_det_confusion reads the detection fields of the loss's own argument block -- map / h / w / map_pixel_stride / n_levels, N,
 * nc, reg_max, img_size, gt_xyxy / gt_cls / gt_off, iou_thresh -- and validates only those (MTBT_EALIGN for a misaligned gt_xyxy).
 * Every anchor is decoded and matched exactly as mtbt_multitask_loss does (one shared prologue): its positives are the loss's
 * positives; each adds 1 at [gt_cls of its matched GT][argmax of its nc raw class logits].
 * mtbt_cls_confusion: logits [N][nc] f32 contiguous, target [N] int64; adds 1 at [target][argmax] per row. */
#define MTBT_CONFUSION_MAX_NC 64
int mtbt_det_confusion(const mtbt_loss_args* a, int64_t* counts, int32_t* status, void* stream);
int mtbt_cls_confusion(const float* logits, const int64_t* target, int N, int nc, int64_t* counts, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Instance-mask loss (YOLOv8-seg `v8SegmentationLoss.single_mask_loss` / `crop_mask`; an extension beyond `_multitask_loss`, which
 * reads the prototypes only through the 1x1 projector) and its gradient with respect to the mask coefficients and the prototypes.
 *   positives   mtbt_multitask_loss's own rule (the shared decode + match prologue) against gt_xyxy, where every GT row is its own
 *               box in pixels of the img_size frame, grouped by image with gt_off [N+1]; rows at or beyond gt_off[N] belong to no image
 *   target      t[b][y][x] = gt_masks[b][y * (S / hp)][x * (S / wp)] (nearest), S = img_size, S % hp == S % wp == 0
 *   per positive a matched to row g:  q = gt_xyxy[g] * (wp / S, hp / S, wp / S, hp / S); pixel (x, y) is inside iff
 *               x >= q.x1 && x < q.x2 && y >= q.y1 && y < q.y2;  logit = sum_c mc[b][a][c] * protos[b][y][x][c];
 *               loss_a = sum_inside bce_with_logits(logit, t) / ((q.x2 - q.x1) * (q.y2 - q.y1))
 *   out[0] = sum_a loss_a / norm, out[1] = #positives;  norm = #positives of the batch, N if there are none
 *   gradients of weight * out[0]:  r = weight * (sigmoid(logit) - t) / (norm * area) on inside pixels,
 *               d_mc[b][a][c] = sum_px r * protos[b][px][c],  d_protos[b][px][c] = sum_a r * mc[b][a][c]
 * map / h / w / map_pixel_stride / n_levels / N / reg_max / img_size / iou_thresh: as in mtbt_loss_args (the class channels are not read).
 * mc: fp32, element (b, a, c) at mc[b * mc_batch_stride + a * mc_anchor_stride + c * mc_channel_stride].  protos: fp32 dense NHWC
 * [N][hp][wp][nm], 16-byte aligned.  gt_masks: fp32 [N][S][S] dense.  nm must be 32.  n_gt rows in gt_xyxy, n_gt <= N * A.
 * d_mc (optional): fp32 dense [N][A][nm]; d_protos (optional): dense NHWC in dprotos_dtype (MTBT_F32 / BF16 / F16, rounded once from
 * fp32).  Both are written whole (zeros for anchors that are not positives and for pixels outside every matched box), or added to
 * when their accumulate flag is set.  Deterministic (fixed-order sums, no floating-point atomics); no host synchronisation.
 * MTBT_EINVAL before any launch: NULL args / maps / gt_xyxy / gt_off / mc / protos / gt_masks / out / workspace, a non-integral
 * img_size or one that hp or wp does not divide, nm != 32, n_gt < 0 or > N * A, workspace_bytes below
 * mtbt_mask_loss_workspace_bytes(N, A, hp, wp, nm), an unknown dprotos_dtype.  MTBT_EALIGN for misaligned gt_xyxy / protos / d_mc / d_protos.
 *
 * mtbt_instance_mask_loss_assigned: the same loss with the positives GIVEN (ultralytics `v8SegmentationLoss`: the mask term runs on
 * the task-aligned assigner's foreground anchors and their assigned GT rows).  assigned: int32 [N][A] dense, in the anchor order of
 * the maps -- what mtbt_tal_det_loss writes; element (b, a) is a row of gt_xyxy or -1.  A value v is foreground only if
 * gt_off[b] <= v < min(gt_off[b + 1], n_gt); any other value (another image's row, at or beyond n_gt, below -1) is background and is
 * never used as an index.  map / h / w / n_levels are read for the anchor count A only: the map pointers may be NULL, and
 * map_pixel_stride, reg_max and iou_thresh are ignored.  Target, crop, area, norm, out, both gradients with their accumulate flags and
 * dtypes, the workspace size, determinism and the error codes are those above; MTBT_EINVAL also for a NULL `assigned`, before any launch.
 * ------------------------------------------------------------------------------------------- */
typedef struct mtbt_mask_loss_args {
  const float* map[3];
  int32_t h[3], w[3];
  int32_t map_pixel_stride[3];
  int32_t n_levels, N, reg_max;
  float img_size, iou_thresh;
  int32_t n_gt;
  const float* gt_xyxy; /* [n_gt][4] pixels */
  const int32_t* gt_off; /* [N+1] */
  const float* mc;
  int64_t mc_batch_stride, mc_anchor_stride, mc_channel_stride;
  const float* protos;
  const float* gt_masks;
  int32_t hp, wp, nm;
  float weight;
  float* d_mc;
  void* d_protos;
  int32_t accumulate_dmc, dprotos_dtype, accumulate_dprotos;
  int32_t reserved;
  void* workspace;
  int64_t workspace_bytes;
  float* out; /* [2]: mask loss, #positives */
} mtbt_mask_loss_args;
int64_t mtbt_mask_loss_workspace_bytes(int N, int A, int hp, int wp, int nm);
int mtbt_instance_mask_loss(const mtbt_mask_loss_args* a, void* stream);
int mtbt_instance_mask_loss_assigned(const mtbt_mask_loss_args* a, const int32_t* assigned, void* stream);
int mtbt_sizeof_mask_loss_args(void);

/* ---------------------------------------------------------------------------------------------
 * Task-aligned detection loss (the loss ultralytics' `Detect` head is trained with: TaskAlignedAssigner + CIoU + DFL + BCE over all
 * anchors, `v8DetectionLoss`; an opt-in sibling of mtbt_multitask_loss's detection terms, whose positives need a predicted box that
 * already overlaps a GT box) and its gradient with respect to the raw Detect maps.  The definition, restated (nothing is copied):
 *   decode      as mtbt_multitask_loss: softmax expectation per side, anchor point (x + .5, y + .5) * stride, stride = img_size / w,
 *               boxes xyxy in pixels.  GT rows: every row its own box in pixels, grouped by image with gt_off [N+1]; rows at or beyond
 *               gt_off[N] belong to no image.  A row whose class lies outside [0, nc) takes part with score 0 and no class target.
 *   ciou(p, g)  eps = 1e-7; w = x2 - x1, h = y2 - y1 + eps; inter = clamp(min(x2) - max(x1), 0) * clamp(min(y2) - max(y1), 0);
 *               iou = inter / (w_p h_p + w_g h_g - inter + eps); cw, ch = extent of the enclosing box;
 *               rho2 = ((g.x1 + g.x2 - p.x1 - p.x2)^2 + (g.y1 + g.y2 - p.y1 - p.y2)^2) / 4;
 *               v = 4 / pi^2 * (atan(w_g / h_g) - atan(w_p / h_p))^2; alpha = v / (v - iou + (1 + eps)), a constant in the gradient;
 *               ciou = iou - (rho2 / (cw^2 + ch^2 + eps) + v * alpha)
 *   assignment  (no gradient) per image, GT row g, anchor a:
 *               inside(g, a) = min(ax - x1, ay - y1, x2 - ax, y2 - ay) > 1e-9;  ov(g, a) = max(ciou(pred_a, gt_g), 0) where inside, else 0;
 *               metric(g, a) = sigmoid(class logit[a][cls_g])^alpha * ov(g, a)^beta  (fp32 powf);
 *               g selects its `topk` anchors of largest metric among ALL anchors of the image, ties (zeros included) to the lower
 *               anchor index; selected anchors that are not inside are dropped; an anchor selected by several rows goes to the one
 *               with the largest ov (the first maximum in row order); such an anchor is foreground (fg) with row g(a).
 *               M_g = max metric, O_g = max ov over g's fg anchors; target score t_a = metric(g(a), a) * O_g / (M_g + 1e-9);
 *               class target = t_a at class cls_g(a), 0 elsewhere; background anchors have all-zero targets.
 *   loss        T = max(sum_a t_a over the batch, 1)
 *               out[2] cls = sum over EVERY anchor and class of bce_with_logits(logit, target) / T
 *               out[0] box = sum_fg (1 - ciou(pred_a, gt_g(a))) * t_a / T
 *               out[1] dfl = sum_fg t_a * mean over the 4 sides of [ce(side, tl) * wl + ce(side, tr) * wr] / T, side target =
 *                            clamp(distance from the anchor point to the GT side / stride, 0, reg_max - 1 - 0.01), tl = floor, tr = tl + 1,
 *                            wl = tr - target, wr = 1 - wl
 *               out[3] = #fg (an exact integer), out[4] = mean ov(g(a), a) over fg (0 without fg), out[5] = T,
 *               out[6] = w_box * box + w_dfl * dfl + w_cls * cls, out[7] = 0
 *   gradient    of out[6] with respect to every channel of every anchor's map row (T, t_a and the assignment are constants):
 *               class channels w_cls * (sigmoid(x) - target) / T for ALL anchors; the 4 * reg_max distribution channels of fg anchors
 *               through the corners (d dist / d raw_j = p_j (j - dist)) plus the DFL term; exact zeros for background anchors.
 * map / h / w / map_pixel_stride / n_levels / N / nc / reg_max / img_size: as in mtbt_loss_args.  n_gt rows in gt_xyxy (16-byte
 * aligned) / gt_cls.  topk in [1, 64].  d_map (all NULL, or one per level, pixel stride >= 4 * reg_max + nc): fp32 NHWC rows,
 * every row written whole, or added to when `accumulate` is set.  assigned (optional) int32 [N][A]: g(a) as a row of gt_xyxy, -1 for
 * background; target_score (optional) fp32 [N][A].  Deterministic (fixed-order sums, no floating-point atomics); no host
 * synchronisation.  MTBT_EINVAL before any launch: NULL args / maps / gt_xyxy / gt_cls / gt_off / out / workspace, bad sizes, topk
 * outside [1, 64], n_gt < 0, some but not all d_map given; MTBT_EALIGN for a misaligned gt_xyxy / workspace; MTBT_EWORKSPACE for
 * workspace_bytes below mtbt_tal_loss_workspace_bytes(N, A, n_gt).
 * ------------------------------------------------------------------------------------------- */
typedef struct mtbt_tal_loss_args {
  const float* map[3];
  int32_t h[3], w[3];
  int32_t map_pixel_stride[3];
  int32_t n_levels, N, nc, reg_max;
  float img_size;
  int32_t n_gt;
  const float* gt_xyxy;   /* [n_gt][4] pixels */
  const int32_t* gt_cls;  /* [n_gt] */
  const int32_t* gt_off;  /* [N+1] */
  int32_t topk;
  float alpha, beta;
  float w_box, w_dfl, w_cls;
  int32_t accumulate;
  int32_t reserved;
  float* d_map[3];
  int32_t d_map_pixel_stride[3];
  int32_t reserved2;
  int32_t* assigned;
  float* target_score;
  void* workspace;
  int64_t workspace_bytes;
  float* out; /* [8] */
} mtbt_tal_loss_args;
int64_t mtbt_tal_loss_workspace_bytes(int N, int A, int G);
int mtbt_tal_det_loss(const mtbt_tal_loss_args* a, void* stream);
int mtbt_sizeof_tal_loss_args(void);

/* ---------------------------------------------------------------------------------------------
 * ConvTranspose2d(C, Cm, 2, stride 2, bias) -> Conv 3x3 (Cm -> K, pad 1) + per-channel shift + activation as ONE direct convolution
 * over the LOW-resolution map (inference).  Replaces ultralytics `Proto.upsample` followed by `Proto.cv2` (conv + folded BatchNorm +
 * SiLU): main_model.py:326-328 [ultralytics Proto], SURVEY 8a row 10.  Both operators are linear with nothing in between: per output
 * parity q = 2 * (Y & 1) + (X & 1) the pair is a 2 x 2-tap convolution of the source map with composed weights (4/10 of the MACs; the
 * upsampled tensor is never written).
 *   x [N,H,W,C] dtype NHWC (H % 16 == 0, W % 16 == 0);  y [N,2H,2W,K] dtype (K % 128 == 0)
 *   w [4][K][2][2][C] dtype:  w[q][k][rho][sigma][ci] multiplies source pixel (i + a - 1 + rho, j + b - 1 + sigma), a = q >> 1, b = q & 1,
 *       for output pixel (2i + a, 2j + b) (zero outside the source map)
 *   shift [9][K] f32: shift[rc * 3 + cc][k], rc / cc = border class of the OUTPUT row / column: 0 = first, 2 = last, 1 = interior
 *       (the transposed conv's bias enters through the taps that lie inside the upsampled map only: the 3x3 conv pads with zeros)
 *   y = act(conv2x2_q(x) + shift[class])           act: MTBT_ACT_NONE | MTBT_ACT_SILU
 * ------------------------------------------------------------------------------------------- */
typedef struct mtbt_upconv_args {
  const void* x;
  const void* w;
  void* y;
  const float* shift;
  int64_t x_batch_stride, y_batch_stride; /* elements */
  int32_t x_pixel_stride, y_pixel_stride; /* elements */
  int32_t N, H, W, C, K;
  int32_t dtype; /* MTBT_F32 | MTBT_BF16 | MTBT_F16: x, w, y */
  int32_t act;
} mtbt_upconv_args;
int mtbt_convt2x2_conv3x3_nhwc(const mtbt_upconv_args* a, void* stream);

/* Fused ConvNeXt MLP (timm Mlp fc1 -> GELU -> fc2 with the layer-scale folded, + residual) for d in {96, 192}, bf16 only:
 *   y[p][:] = res[p][:] + W2' . GELU(W1 . t[p][:] + b1) + b2'      (the 4d-wide hidden tensor never leaves the chip)
 * t, res, y: dense [M][d] bf16; w1 [4d][d] bf16; b1 [4d] f32; b2 [d] f32; w2p [d][4d] bf16 whose columns are reordered
 * inside every group of 32 hidden units: slot 8g+j holds hidden 4g+j (j < 4) or 16+4g+(j-4) (j >= 4), g = 0..3. */
int mtbt_convnext_mlp_fused(const void* t, const void* res, const void* w1, const float* b1, const void* w2p,
                            const float* b2, void* y, int64_t M, int D, void* stream);
/* the same with the 16-bit storage type given: MTBT_BF16 or MTBT_F16 */
int mtbt_convnext_mlp_fused_dt(const void* t, const void* res, const void* w1, const float* b1, const void* w2p,
                               const float* b2, void* y, int64_t M, int D, int dtype, void* stream);
/* Training forward of the same block (bf16, d in {96, 192}): y as above PLUS hpre [M][4d] bf16 = W1 . t + b1, the fc1 PRE-activation in
 * natural hidden order -- all the backward needs (GELU' in the fc2 input gradient, GELU re-applied by mtbt_conv_wgrad_xact); the activated
 * hidden tensor is never written.  Weight order of THIS entry: w1_perm / b1_perm have their rows permuted inside every group of 32 hidden
 * units -- row 16 b + 4 g + e holds hidden unit 8 g + 4 b + e (b = 0..1, g = 0..3, e = 0..3) -- and w2 [d][4d] keeps the natural column
 * order (layer scale folded into its rows, b2 = gamma * fc2.bias).  Replaces timm Mlp.forward under model.train(), main_model.py:21-26. */
int mtbt_convnext_mlp_fused_train(const void* t, const void* res, const void* w1_perm, const float* b1_perm, const void* w2, const float* b2,
                                  void* y, void* hpre, int64_t M, int D, void* stream);

/* Pairwise IoU of xyxy boxes (running_main_v3.py:71-97, `batch_bbox_iou`): out[i][j] = inter / (area1_i + area2_j - inter + eps),
 * inter = clamp(min(x2)-max(x1), 0) * clamp(min(y2)-max(y1), 0); fp32, the reference's operation order without FMA
 * contraction (bit-exact with the torch CPU result).  boxes1 [n,4], boxes2 [m,4], out [n,m] row-major; n or m == 0 is a
 * no-op (the reference returns an empty/zero matrix). */
int mtbt_bbox_iou_pairwise(const float* boxes1, int n, const float* boxes2, int m, float eps, float* out, void* stream);

/* Input pipeline of one batch (dataset_btxrdv2.py:109-166: `_letterbox`, BGR->RGB, /255, HWC->CHW, mask binarise), SURVEY §8f N2.
 * images: HOST array of `count` descriptors of DEVICE buffers (decoded 8-bit BGR image as cv2.imread returns it, optional
 * 8-bit grayscale mask of the same size).  Per image: scale = S / max(H0, W0), new = max(1, int(dim * scale)),
 * image resized like cv2.resize(INTER_LINEAR) (OpenCV's 8-bit fixed-point path), mask like INTER_NEAREST, both placed
 * top-left; image padded with 114, mask with 0.  out_images [count][3][S][S] f32 RGB in [0,1]; out_masks
 * [count][1][S][S] f32 in {0,1} (NULL = skip; a NULL descriptor mask gives zeros); out_scales HOST [count] (NULL = skip):
 * the letterbox scale the caller applies to its YOLO-txt boxes (:200-203).  S % 4 == 0.
 * Order of the checks, the same in the three entry points of this pipeline: (1) MTBT_EINVAL with every item checked, so before any
 * launch and before out_scales is written: NULL images / out_images, count < 0, img_size <= 0 or % 4, a descriptor with a NULL bgr, a
 * height or width <= 0, row_stride < 3 * width, a mask with mask_row_stride < width, height * row_stride >= 2^31 - 1, or a resized side
 * beyond 32768 (only an img_size beyond 32768 gives one); (2) then MTBT_EALIGN for outputs not 16-byte aligned; (3) then the first
 * launch, one per <= 32 images.  count == 0 is MTBT_OK with nothing launched. */
typedef struct {
  const uint8_t* bgr;
  const uint8_t* mask;
  int32_t height, width;
  int64_t row_stride;       /* bytes between image rows (>= 3 * width) */
  int64_t mask_row_stride;  /* bytes between mask rows (>= width) */
} mtbt_raw_image;
int mtbt_letterbox_batch(const mtbt_raw_image* images, int count, int img_size, float* out_images, float* out_masks,
                         double* out_scales, void* stream);

/* Training augmentation fused into the same work: scale / aspect jitter, shift / crop, the eight dihedral orientations and a
 * per-image intensity table, one launch per <= 32 images.  The reference has NO augmentation; this arithmetic is the project's own
 * definition (which is why oracle/ holds no counterpart; tests/augment_reference.py restates it in numpy).
 * geom: HOST int32 [count][geom_stride], geom_stride must be 8:
 *   [0] new_w, [1] new_h   size of the resized image R, each in [1, 32768], independent of each other and of S
 *   [2] off_x, [3] off_y   canvas offset of the oriented image, any int32 (negative offsets crop)
 *   [4] orient             bit 0 flips x, bit 1 flips y, bit 2 transposes;  [5..7] reserved, must be 0
 * R is the source resized to new_w x new_h by mtbt_letterbox_batch's arithmetic (8-bit INTER_LINEAR image, INTER_NEAREST mask, source
 * step 1.0 / ((double)new / (double)old) per axis); it is never materialised.  The oriented image Q is (qh, qw) = (new_h, new_w), or
 * (new_w, new_h) when transposed:  Q[y][x] = R[y'][x'] with x1 = bit 0 ? qw-1-x : x, y1 = bit 1 ? qh-1-y : y, (x', y') = bit 2 ? (y1, x1) : (x1, y1).
 * Canvas O[dy][dx] = Q[dy-off_y][dx-off_x] where that lies inside Q; elsewhere the image is 114/255 and the mask 0 (an image wholly
 * outside gives a pure pad image).  lut: DEVICE uint8 [count][3][256] in the source's BGR channel order or NULL (identity), applied to
 * each resized 8-bit channel value before the one correctly rounded /255; pad pixels are not remapped.  Outputs as
 * mtbt_letterbox_batch.  With the letterbox's new_w / new_h, zero offsets, orient 0 and no table the output equals
 * mtbt_letterbox_batch bit for bit.  Every source index is clamped to the source: no geometry addresses outside it.
 * Order of the checks as in mtbt_letterbox_batch: (1) MTBT_EINVAL with every image checked, so before any launch: NULL images / geom /
 * out_images, geom_stride != 8, img_size <= 0 or % 4, count < 0, new_w or new_h outside [1, 32768], orient outside 0..7, a non-zero
 * reserved field, a descriptor mtbt_letterbox_batch refuses; (2) then MTBT_EALIGN for outputs not 16-byte aligned (a call that is both
 * invalid and misaligned is MTBT_EINVAL); (3) then the first launch.  count == 0 is MTBT_OK with nothing launched. */
int mtbt_augment_batch(const mtbt_raw_image* images, int count, int img_size, const int32_t* geom, int geom_stride,
                       const uint8_t* lut, float* out_images, float* out_masks, void* stream);

/* Four-image mosaic on the same arithmetic (the project's own definition as well; tests/mosaic_reference.py restates it from
 * tests/augment_reference.py).  A canvas is S x S with a centre (cx, cy), 0 <= cx <= S, cx % 4 == 0, 0 <= cy <= S, which cuts it into four
 * half-open rectangles, x then y:
 *   tile 0 [0,cx) x [0,cy)    tile 1 [cx,S) x [0,cy)    tile 2 [0,cx) x [cy,S)    tile 3 [cx,S) x [cy,S)
 * Tile t of canvas i has its own source descriptor tiles[4*i + t] and its own geometry row geom[4*i + t] = (new_w, new_h, off_x, off_y,
 * orient, 0, 0, 0), which means exactly what it means in mtbt_augment_batch, its offsets in CANVAS coordinates: inside its rectangle the
 * canvas equals what mtbt_augment_batch would draw for that source and row on a whole S x S canvas (image, 114/255 pad and mask); outside
 * its rectangle a tile draws nothing.  lut: one optional table per CANVAS (DEVICE uint8 [count][3][256], BGR order) that remaps the resized
 * bytes of all four tiles, never the pad.  A tile whose descriptor has no mask contributes zeros to its rectangle.  An empty rectangle (cx
 * or cy at 0 or S) is legal; with the centre at (S, S) tile 0 is the whole canvas and the result is mtbt_augment_batch of tile 0, bit for
 * bit, so a batch that mixes mosaic and plain canvases is one call.  Descriptors may repeat.  One launch per <= 8 canvases (32 descriptors);
 * every output byte is written exactly once; every source index is clamped to its source.  Outputs as mtbt_letterbox_batch.
 * Order of the checks as in mtbt_letterbox_batch: (1) MTBT_EINVAL with every canvas checked, so before any launch: NULL tiles / geom /
 * centres / out_images, geom_stride != 8, count < 0, img_size <= 0 or % 4, cx outside [0, S] or % 4, cy outside [0, S], any of a canvas's
 * four rows or descriptors that mtbt_augment_batch would refuse (also those of an empty tile); (2) then MTBT_EALIGN for outputs not
 * 16-byte aligned; (3) then the first launch.  count == 0 is MTBT_OK with nothing launched. */
int mtbt_mosaic_batch(const mtbt_raw_image* tiles /* HOST [4*count], canvas-major, repeats allowed */, int count, int img_size,
                      const int32_t* geom /* HOST [4*count][geom_stride], geom_stride == 8 */, int geom_stride,
                      const int32_t* centres /* HOST [count][2] = cx, cy */, const uint8_t* lut /* DEVICE [count][3][256] or NULL */,
                      float* out_images, float* out_masks /* NULL = skip */, void* stream);

/* Affine augmentation on the device (csrc/warp_affine.hip; `preprocess.warp_batch`, `affine_samples`): rotation by any angle, shear, and
 * with them every 2 x 3 map, one canvas per source.  The reference augments nothing and cv2 is absent here, so THE RULE below is this
 * project's own definition, modelled on cv2's warpAffine(INTER_LINEAR) -- an inverse map in fixed point, a position reduced to 1/32 pixel,
 * 2 x 2 taps -- and exact in integers (tests/warp_reference.py restates it in numpy).  It has a kernel of its own: the two entry points above
 * rest on separable taps (a canvas row is a row or a column of the source), and a rotated row is neither.
 * Per canvas i: a source descriptor images[i] (H0 x W0) and a row coef[i] = (a, b, c, d, e, f, 0, 0) of HOST int64, coef_stride must be 8.
 *   Position       of canvas pixel (dx, dy), in source pixel-index coordinates (an integer is a pixel centre), units of 1/65536 px, int64:
 *                  X = a dx + b dy + c, Y = d dx + e dy + f;  Xs = (X + 1024) >> 11, Ys = (Y + 1024) >> 11 (arithmetic shift = floor):
 *                  the position rounded to 1/32 px.
 *   Inside         -16 <= Xs <= 32 W0 - 17 and -16 <= Ys <= 32 H0 - 17: the rounded position lies in the source's pixel footprint
 *                  [-0.5, W0 - 0.5) x [-0.5, H0 - 0.5).  Compared in int64, before anything is narrowed.
 *   Image, inside  sx = Xs >> 5 (may be -1), fx = Xs & 31, the same for y;  x0 = clamp(sx, 0, W0 - 1), x1 = clamp(sx + 1, 0, W0 - 1),
 *                  y0, y1 likewise;  per channel
 *                  v = ((32-fx)(32-fy) S[y0][x0] + fx (32-fy) S[y0][x1] + (32-fx) fy S[y1][x0] + fx fy S[y1][x1] + 512) >> 10.
 *                  The weights sum to 1024, so v is in 0..255 without a clamp.  Then the optional table lut[i][c][v] (DEVICE uint8
 *                  [count][3][256], the source's BGR order, as in mtbt_augment_batch), the one correctly rounded /255, BGR -> RGB planes.
 *   Mask, inside   mx = clamp((Xs + 16) >> 5, 0, W0 - 1), my likewise: the nearest source pixel; 1.f when that byte is >= 128, else 0.f.
 *                  A descriptor without a mask gives zeros.
 *   Outside        image 114/255, not remapped by the table; mask 0.  A map that shows nothing of the source gives a pure pad canvas.
 * Every source index is clamped, so no coefficients address outside the source.  Outputs as mtbt_letterbox_batch: out_images
 * [count][3][S][S] f32 RGB in [0,1], out_masks [count][1][S][S] f32 in {0,1} or NULL.  There is NO area averaging: a map that shrinks the
 * source by more than 2 aliases, as warpAffine does and as the INTER_LINEAR path of the entry points above does.  This rule is NOT
 * bit-equal to mtbt_augment_batch at angle 0: that path is cv2's two-pass resize with 11-bit coefficients per axis, this one blends four
 * taps with 5-bit fractions in one step; no equality between the two is claimed or tested.
 * Limits: |a|, |b|, |d|, |e| <= 2^26 (1024 source px per canvas px), |c|, |f| <= 2^47, img_size <= 32768; with them |X|, |Y| < 2^48.
 * The host side (`preprocess.affine_coefficients`) makes the row from a forward matrix in float64 and moves the labels by the exact
 * inverse of the INTEGER map, so labels follow the pixels.
 * One launch per <= 32 canvases, asynchronous on `stream`; every output byte is written exactly once; no LDS, no atomics.
 * Order of the checks as in mtbt_letterbox_batch: (1) MTBT_EINVAL with every canvas checked, so before any launch: NULL images / coef /
 * out_images, coef_stride != 8, count < 0, img_size <= 0, % 4 or > 32768, a coefficient outside the limits, a non-zero reserved field, a
 * descriptor mtbt_letterbox_batch refuses; (2) then MTBT_EALIGN for outputs not 16-byte aligned (a call that is both invalid and
 * misaligned is MTBT_EINVAL); (3) then the first launch.  count == 0 is MTBT_OK with nothing launched. */
int mtbt_warp_batch(const mtbt_raw_image* images, int count, int img_size, const int64_t* coef /* HOST [count][coef_stride] */,
                    int coef_stride, const uint8_t* lut /* DEVICE [count][3][256] or NULL */, float* out_images,
                    float* out_masks /* NULL = skip */, void* stream);

/* Contrast-limited adaptive histogram equalisation of raw uint8 images on the device (csrc/clahe.hip; `preprocess.clahe_batch`, the
 * `clahe=` option of the `*_samples` functions), ahead of the resampling entry points above and independent of them.  The reference
 * equalises nothing; cv2 is absent here, so THE RULE below is this project's own definition, modelled step for step on cv2's CLAHE
 * (modules/imgproc/src/clahe.cpp) and exact in integers (tests/clahe_reference.py restates it in numpy).  It differs from cv2 in two
 * places, where cv2 rounds through float32 (the curve's scale 255 / area and the bilinear blend) and this rule rounds the exact rational:
 * a difference from cv2 of at most one grey level at a few pixels is expected and has not been measured.
 * Per image: H x W, channels 1 or 3 (interleaved, as cv2.imread returns them), a grid gx x gy, an integer clip >= 0.
 *   Key            one channel: k = v.  Three channels: k = (c0 + 2 c1 + c2 + 2) >> 2.  ONE curve is built from k and applied to each
 *                  channel value, so a grey image stored as three equal channels stays grey and equals the one-channel result.
 *   Tiles          tw = ceil(W / gx), th = ceil(H / gy), area = tw th.  The image is extended on the right and bottom to gx tw x gy th by
 *                  reflection without repeating the edge (index i >= n reads 2 (n - 1) - i); the extension is never materialised.  Tile
 *                  (i, j) covers [i tw, (i + 1) tw) x [j th, (j + 1) th) of the extended image; hist[b] counts its keys and sums to area.
 *   Clip           skipped when clip == 0.  excess = sum max(hist[b] - clip, 0); hist[b] = min(hist[b], clip); hist[b] += excess / 256
 *                  for all b; r = excess % 256; if r > 0: step = max(256 / r, 1) and hist[j step] += 1 for j = 0 .. r - 1 (the closed
 *                  form of cv2's loop).  The counts still sum to area.
 *   Curve          cdf[b] = sum of hist[b'] over b' <= b; lut[b] = (510 cdf[b] + area) / (2 area), integer division: 255 cdf / area
 *                  rounded half up, so lut[255] = 255.
 *   Interpolation  column x: u = 2 x + 1 - tw, t1 = floor(u / 2 tw) (may be -1), a = u - t1 2 tw in [0, 2 tw); weights (2 tw - a, a)
 *                  on tiles (clamp(t1), clamp(t1 + 1)), clamped to [0, gx - 1]; rows the same with th and gy.
 *                  out = (sum over the four tiles of wy wx lut_tile[v] + 2 tw th) / (4 tw th): the exact rational of cv2's bilinear
 *                  blend between tile centres, rounded half up.  With area <= 2^22 the sum fits uint32.
 *   Host           clip = 0 if clip_limit <= 0 else max(1, int(clip_limit * area / 256)) in double arithmetic is cv2's formula
 *                  (`preprocess.clahe_clip`); the library sees only the integer.
 * images: HOST array of DEVICE buffers; sizes and channel counts may be mixed within a batch.  dst == src with equal strides is allowed
 * (each output byte depends on the input only at its own place plus the finished curves).  Every byte of the width * channels bytes of
 * each destination row is written; stride padding is never touched.  Workspace: mtbt_clahe_workspace_bytes(...) bytes of DEVICE memory,
 * 16-byte aligned (int32 histograms, cleared on the stream by the entry point, then the curves); two calls on one stream may share it.
 * Asynchronous on `stream`, no host synchronisation, graph-capturable; integer arithmetic and integer atomics only, so the result is a
 * pure function of the input.  Three launches (histograms, curves, apply) per <= 32 images.
 * Order of the checks as in mtbt_letterbox_batch: (1) MTBT_EINVAL with every item checked, so before any launch: NULL images / src /
 * dst, count < 0, grid_x or grid_y outside [1, 16], channels not 1 or 3, height < grid_y or width < grid_x, clip < 0, a stride below
 * width * channels, height * stride >= 2^31 - 1, area > 2^22, a workspace that is NULL or smaller than mtbt_clahe_workspace_bytes when
 * that is positive, a destination that overlaps a source of the call other than exactly its own (dst == src, equal strides); (2) then
 * MTBT_EALIGN for a workspace not 16-byte aligned; (3) then the first launch.  count == 0 is MTBT_OK with nothing launched.
 * mtbt_clahe_workspace_bytes returns MTBT_EINVAL for count < 0, a grid outside [1, 16] or NULL images with count > 0. */
typedef struct mtbt_clahe_image { /* HOST array, DEVICE buffers */
  const uint8_t* src;
  uint8_t* dst;
  int32_t height, width, channels, clip;
  int64_t src_row_stride, dst_row_stride; /* bytes, >= width * channels */
} mtbt_clahe_image;
int64_t mtbt_clahe_workspace_bytes(const mtbt_clahe_image* images, int count, int grid_x, int grid_y);
int mtbt_clahe_batch(const mtbt_clahe_image* images, int count, int grid_x, int grid_y, void* workspace, int64_t workspace_bytes,
                     void* stream);
/* sizeof() of the struct above as the library was compiled: which = 0 mtbt_clahe_image; -1 otherwise */
int mtbt_sizeof_clahe_args(int which);

/* Copy-paste augmentation between the canvases of a batch on the device (csrc/copy_paste.hip; `preprocess.copy_paste_batch`, the
 * `copy_paste=` option of the `*_samples_seg` functions): instances, given as bit-packed planes, are cut out of donor canvases and laid
 * on destination canvases, pixels, planes and label rows together.  The reference augments nothing, so THE RULE below is this project's
 * own, and exact: no float arithmetic touches a pixel (tests/copy_paste_reference.py restates it in numpy).
 *   Inputs     B canvases images f32 [B][3][S][S]; M planes uint8 [M][S][pitch], pitch = 8 * ceil(S / 64), packed as everywhere in this
 *              header, grouped by canvas through row_off[B + 1] (canvas i owns the rows row_off[i] .. row_off[i + 1] - 1); a label row per
 *              plane, rows_in f32 [M][6] = (image, cls, xc, yc, w, h); P paste entries grouped by DESTINATION canvas through
 *              paste_off[B + 1], each (src_row, dx, dy, flip, 0, 0, 0, 0) of int32, entry_stride must be 8.
 *   Pasted     entry e of canvas i with donor row r = src_row, which lies on canvas j (row_off[j] <= r < row_off[j + 1]; j == i is
 *              allowed):  T_e[y'][x'] = planes[r][y][x] with y = y' - dy, x = flip ? S - 1 - (x' - dx) : x' - dx, and 0 wherever (x, y) is
 *              outside [0, S)^2: the donor canvas is mirrored first, then translated.
 *   Layering   the entries of a canvas apply in table order, later above earlier: C_e = OR of T over the later entries of the canvas, the
 *              visible plane V_e = T_e & ~C_e; U_i = OR of all T of canvas i; an old row m of canvas i becomes O_m = planes[m] & ~U_i.
 *              Old planes that overlap each other are left as they are.
 *   Pixels     out[i][c][y'][x'] = images[j][c][y][x] of the topmost entry with T_e[y'][x'] set (its j, x, y), else images[i][c][y'][x'].
 *              Floats are copied, never recomputed.  The input is never modified, so mutual pastes (i from j and j from i) and
 *              self-pastes read pristine pixels; outputs may not overlap inputs.
 *   Planes     out_planes [M + P][S][pitch]: rows 0 .. M-1 are O_m, rows M .. M+P-1 are V_e in table order; every byte is written,
 *              padding bits are zero (input bits at x >= S, which the layout forbids, are ignored).
 *   Mask       out_masks (optional) [B][1][S][S] f32 in {0, 1}: the union of the canvas's output planes = old union | U_i.
 *   Records    area_before uint32 [M + P]: popcount of planes[m], respectively of T_e; area uint32 [M + P]: popcount of the output plane;
 *              box int32 [M + P][4]: tight x1, y1, x2, y2 of the output plane with exclusive maxima, all zero for an empty plane (the
 *              convention of mtbt_fill_polygons).  All three are fully defined after the call.
 *   Rows       rows_out (optional) f32 [M + P][6]; the first rule that applies:
 *                (1) an old row with area == area_before is rows_in[m], bit for bit (so P == 0 returns rows_in);
 *                (2) a row with area == 0 is (image, cls, 0, 0, 0, 0);
 *                (3) every other row is (image, cls, xc, yc, w, h) from the box: xc = float(x1 + x2) / float(2 S),
 *                    yc = float(y1 + y2) / float(2 S), w = float(x2 - x1) / float(S), h = float(y2 - y1) / float(S), each division
 *                    correctly rounded in f32; the operands are exact integers, so the result is one defined float.
 *              image and cls of an old row are rows_in[m][0], rows_in[m][1]; of a pasted row float(i) and rows_in[src_row][1].
 *              A zero row is what an instance becomes that later pastes cover completely.  Downstream `loss.group_gt_rows_cls` moves a
 *              row of zero width or height behind off[N], so the task-aligned loss and the mask loss skip it; in the reference's loss it
 *              is a zero-area box whose IoU with everything is 0.  Rows are never dropped here: area and area_before are returned for
 *              callers that filter.
 * row_off, paste_off and entries are HOST arrays, validated in full before any launch and handed to the kernel by value, 8 canvases per
 * launch; everything else is DEVICE memory.  Asynchronous on `stream`, no allocation, no workspace, no host synchronisation,
 * graph-capturable.  Integer atomics gather the records only (cleared on the stream first), and one small finishing launch turns them into
 * boxes and rows: the result is a pure function of the input.  Every output byte is written exactly once.
 * Limits: S % 4 == 0, 4 <= S <= 32768, at most 16 entries per canvas, |dx|, |dy| <= S.
 * Required pointers: a, row_off, paste_off; images and out_images when B > 0; planes when M > 0; entries when P > 0; out_planes,
 * area_before, area and box when M + P > 0; rows_in when rows_out is given and M + P > 0.
 * Order of the checks: (1) MTBT_EINVAL with every item checked, so before any launch: a NULL required pointer, B, M or P negative, S
 * outside the limits, pitch != 8 * ceil(S / 64), entry_stride != 8, an offset table that does not start at 0, decreases or ends
 * elsewhere than M respectively P, more than 16 entries on a canvas, src_row outside [0, M), flip outside {0, 1}, |dx| or |dy| > S, a
 * non-zero reserved field, rows_out without rows_in, an output range that overlaps an input range; (2) then MTBT_EALIGN: images, out_images
 * or out_masks not 16-byte aligned, planes or out_planes not 8-byte aligned, rows or records not 4-byte aligned; (3) then the launches.
 * B == 0 launches nothing.  M == 0 or P == 0 is legal: the images are copied, the planes copied (P == 0) or absent (M == 0). */
typedef struct mtbt_copy_paste_args {
  const float* images;           /* [B][3][S][S] */
  const uint8_t* planes;         /* [M][S][pitch] */
  const float* rows_in;          /* [M][6], or NULL when rows_out is NULL */
  const int32_t* row_off;        /* HOST [B + 1] into the planes */
  const int32_t* paste_off;      /* HOST [B + 1] into the entries */
  const int32_t* entries;        /* HOST [P][entry_stride] = src_row, dx, dy, flip, 0, 0, 0, 0 */
  float* out_images;             /* [B][3][S][S] */
  uint8_t* out_planes;           /* [M + P][S][pitch] */
  float* out_masks;              /* [B][1][S][S] or NULL */
  float* rows_out;               /* [M + P][6] or NULL */
  uint32_t* area_before;         /* [M + P] */
  uint32_t* area;                /* [M + P] */
  int32_t* box;                  /* [M + P][4] */
  int32_t B, M, P, S, pitch, entry_stride;
} mtbt_copy_paste_args;
int mtbt_copy_paste(const mtbt_copy_paste_args* a, void* stream);
/* sizeof() of the struct above as the library was compiled: which = 0 mtbt_copy_paste_args; -1 otherwise */
int mtbt_sizeof_copy_paste_args(int which);

/* Segmentation metric accumulators (running_main_v3.py:466-498 feeding the torchmetrics objects of :198-203), SURVEY §8f N3.
 * logits, gt: [B][n_per_image] f32 (n % 4 == 0); prediction = sigmoid(logit) > 0.5, target = int(gt) >= 1.
 * counts [B][4] int64 = TP, FP, FN, TN per image; prob_sum [B] = sum of sigmoid(logit) over predicted-foreground pixels
 * (numerator of the per-image mask score, :483).  Asynchronous, deterministic. */
int64_t mtbt_seg_confusion_workspace_bytes(int B);
int mtbt_seg_confusion(const float* logits, const float* gt, int B, int64_t n_per_image, int64_t* counts, float* prob_sum,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* COCO box matching for the box mAP (torchmetrics MeanAveragePrecision of running_main_v3.py:209-217, evaluate_model.py:81-93):
 * pycocotools COCOeval.evaluateImg (bbox, no crowd) for B images x the 4 COCO area ranges x T IoU thresholds in one launch.
 *   boxes [B][K][4] xyxy f32 (16-byte aligned), scores [B][K] f32, labels [B][K] int64 (class ids within int32), counts [B] int32
 *   (valid slots per image; NULL => all K) -- exactly what mtbt_nms_batched writes;
 *   gt [M][6] f32 rows (batch_idx, cls, a, b, c, d): gt_format 0 = (cx, cy, w, h) normalised, converted to clamped xyxy pixels with
 *   img_size by validation_step's per-box formula (:566); 1 = (x1, y1, x2, y2) pixels.  Rows need not be grouped by image.
 *   iou_thresholds[0..T-1] (fp64, 1 <= T <= 32); max_det = the largest max-detection threshold.
 * Outputs: rank [B][K] int32 (position in the (image, class) score order, stable on the slot; -1 = invalid or beyond max_det);
 *   match / ignore [B][K][4] uint32 (word = area range all / small / medium / large, bit t = IoU threshold t); gt_area [M] uint32
 *   (bit a: the row is not ignored in area range a; 0 for rows of no image); status: set to 1 when an image has more than 1024 GT
 *   rows (the caller zeroes it; that image's detections come back invalid).  Caps: K <= 1024, 1024 GT boxes per image.
 * IoU in fp64 in metrics.box_iou_xyxy's operation order, no contraction: decisions bit-identical to the host metric.  Semantics
 * spelled out in csrc/box_eval.hip.  MTBT_EINVAL for NULL pointers, T outside [1, 32], K outside [1, 1024], max_det < 1, a bad
 * gt_format; MTBT_EALIGN for misaligned pointers.  Asynchronous, deterministic, no workspace. */
typedef struct mtbt_box_eval_args {
  const float* boxes;
  const float* scores;
  const int64_t* labels;
  const int32_t* counts;
  const float* gt;
  int32_t* rank;
  uint32_t* match;
  uint32_t* ignore;
  uint32_t* gt_area;
  int32_t* status;
  double iou_thresholds[32];
  int32_t B, K, M, T;
  int32_t max_det;
  int32_t gt_format;
  float img_size;
} mtbt_box_eval_args;
int mtbt_box_eval(const mtbt_box_eval_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Instance-mask COCO evaluation from bit-packed planes (csrc/mask_eval.hip): three entry points that turn packed detection and
 * ground-truth masks into the per-detection records mtbt_box_eval writes for boxes.  Every count is an exact integer and every
 * IoU a quotient of exact integers in fp64: results are bit-reproducible against numpy.
 * Packed layout (the one mtbt_masks_to_frames writes): a plane is H rows of pitch = 8 * ceil(W / 64) bytes, pixel X is bit X & 7
 * of byte X >> 3, padding bits X >= W are zero (inputs may rely on that).  Planes are 8-byte aligned, NOT more: with H odd and
 * pitch = 8 mod 16 every second plane sits on an odd 8-byte boundary, so the kernels use 8-byte accesses only.
 * All three are asynchronous on `stream`, deterministic, free of global atomics (the matching walk
 * sets its match bit sets with LDS atomicOr, as mtbt_box_eval does) and need no workspace.
 * ------------------------------------------------------------------------------------------- */

/* mtbt_pack_masks: dense planes -> packed planes.
 *   src       [n_src] planes of H rows; element (s, Y, X) at src + s * plane_stride + Y * row_stride + X (strides in ELEMENTS);
 *             dtype 0 = uint8 (bool storage), 1 = float32
 *   plane_of  int32 [n_out] or NULL: output j is made from source plane plane_of[j] (NULL: j, then n_out <= n_src is required);
 *             a value outside [0, n_src) gives a zero plane
 *   boxes     float32 [n_out][4] xyxy pixels or NULL: output j keeps only x1 <= X < x2 && y1 <= Y < y2, compared in fp32 (the crop
 *             rule of mtbt_masks_to_frames); pixels outside the box are not read; a NaN corner gives a zero plane
 *   out       [n_out][H][pitch]; bit = value > 0 (NaN -> 0).  EVERY byte is written, padding included.
 * MTBT_EINVAL before any launch: NULL a / out, NULL src with n_src > 0, n_src < 0, n_out < 0, H < 1, W < 1, H * W >= 2^31,
 * pitch != 8 * ceil(W / 64), row_stride < W, plane_stride < 0, a dtype other than 0 / 1, plane_of == NULL with n_out > n_src.
 * MTBT_EALIGN: out not 8-byte aligned, a float32 src / boxes / plane_of not 4-byte aligned.  n_out == 0 launches nothing. */
typedef struct mtbt_pack_masks_args {
  const void* src;
  const int32_t* plane_of; /* [n_out] or NULL */
  const float* boxes;      /* [n_out][4] or NULL */
  uint8_t* out;            /* [n_out][H][pitch] */
  int64_t plane_stride, row_stride; /* elements */
  int32_t n_src, n_out, H, W, pitch;
  int32_t dtype;           /* 0 uint8, 1 float32 */
} mtbt_pack_masks_args;
int mtbt_pack_masks(const mtbt_pack_masks_args* a, void* stream);

/* mtbt_mask_pair_counts: pixel-count tables of one launch of up to 32 images, each with its own size.
 * Image b: K packed detection planes at det (plane k at det + k * H * pitch) and its ground-truth planes addressed from gt_base:
 * flat GT plane m (0 <= m < M) belongs to image gt_image[m] of THIS launch (device int32; a value outside [0, n_images) = no image)
 * and lives at gt_base_b + (m - g0_b) * H_b * pitch_b; a row with m - g0_b outside [0, gt_planes_b) is treated as of no image.
 * One rule, two layouts: a list of images with their own GT tensors (g0_b = index of the image's first flat row, gt_planes_b = its
 * G_b), or a uniform batch whose GT planes are one flat [M][H][pitch] buffer (every image: gt_base = the buffer, g0 = 0, gt_planes = M;
 * membership is known only on the device).  The descriptors are read on the host and travel as kernel arguments.
 *   inter    uint32 [M][K]  popcount(gt_m & det_{b(m),k});  det_area uint32 [n_images][K];  gt_area uint32 [M]
 *   counts   int32 [n_images] or NULL (all K): planes k >= counts[b] count as empty and are NOT read
 * Rows of no image give zeros.  Every output word is defined after the call (the entry point clears inter and gt_area on the stream
 * before the launch; the kernel writes det_area whole): the caller does not pre-zero.  One workgroup owns one (image, plane k).
 * MTBT_EINVAL before any launch: NULL a / images / det_area, M > 0 with NULL inter / gt_image / gt_area (all three
 * may be NULL when M == 0: nothing of them is read or written), K outside [1, 1024],
 * n_images outside [1, 32] or != a->B, M < 0, and per image NULL det / gt_base, H < 1, W < 1, H * W >= 2^31,
 * pitch != 8 * ceil(W / 64), gt_planes < 0.  MTBT_EALIGN: det / gt_base not 8-byte aligned, the tables not 4-byte aligned. */
typedef struct mtbt_mask_image {
  const uint8_t* det;     /* K packed planes (only the first counts[b] are read) */
  const uint8_t* gt_base; /* see the addressing rule above; any non-NULL 8-byte aligned pointer when the image has no GT */
  int32_t H, W, pitch;
  int32_t g0;             /* flat row of the plane at gt_base */
  int32_t gt_planes;      /* planes addressable from gt_base */
  int32_t reserved;
} mtbt_mask_image;

typedef struct mtbt_mask_pair_args {
  const int32_t* counts;   /* [B] or NULL */
  const int32_t* gt_image; /* [M] */
  uint32_t* inter;         /* [M][K]; NULL allowed when M == 0 */
  uint32_t* det_area;      /* [B][K] */
  uint32_t* gt_area;       /* [M]; NULL allowed when M == 0 */
  int32_t B, K, M;
  int32_t reserved;
} mtbt_mask_pair_args;
int mtbt_mask_pair_counts(const mtbt_mask_pair_args* a, const mtbt_mask_image* images, int n_images, void* stream);

/* mtbt_mask_eval: the matching walk of mtbt_box_eval (semantics at the top of csrc/box_eval.hip: per (image, class), score order
 * stable on the slot, max_det, the four inclusive area ranges, lim = min(t, 1 - 1e-10), highest IoU / later GT on ties, the
 * non-ignored / ignored two-candidate rule, detection ignore flags) over the tables of mtbt_mask_pair_counts:
 *   IoU  = inter / (det_area + gt_px - inter) in fp64 from the integers, 0 when the union is 0; areas are the pixel counts;
 *   GT membership, order and class come from gt_image [M] (a value outside [0, B) = no image) and gt_label [M], both int32.
 * B is not limited here (the tables of several pair-count launches may be evaluated together).  Outputs as mtbt_box_eval: rank
 * [B][K] int32, match / ignore [B][K][4] uint32, gt_area [M] uint32 area-range sets (0 for rows of no image), status set to 1 when
 * an image holds more than 1024 GT planes (the caller zeroes it; that image's detections come back invalid).
 * MTBT_EINVAL: NULL pointers (inter / gt_px / gt_image / gt_label / gt_area may be NULL only when M == 0), T outside [1, 32],
 * K outside [1, 1024], B < 0, M < 0, max_det < 1.  MTBT_EALIGN for misaligned pointers. */
typedef struct mtbt_mask_eval_args {
  const uint32_t* inter;    /* [M][K] */
  const uint32_t* det_area; /* [B][K] */
  const uint32_t* gt_px;    /* [M] pixel counts */
  const float* scores;      /* [B][K] */
  const int64_t* labels;    /* [B][K] */
  const int32_t* counts;    /* [B] or NULL */
  const int32_t* gt_image;  /* [M] */
  const int32_t* gt_label;  /* [M] */
  int32_t* rank;
  uint32_t* match;
  uint32_t* ignore;
  uint32_t* gt_area;
  int32_t* status;
  double iou_thresholds[32];
  int32_t B, K, M, T;
  int32_t max_det;
  int32_t reserved;
} mtbt_mask_eval_args;
int mtbt_mask_eval(const mtbt_mask_eval_args* args, void* stream);
/* sizeof() of the four structs above as the library was compiled: which = 0 mtbt_pack_masks_args, 1 mtbt_mask_image,
 * 2 mtbt_mask_pair_args, 3 mtbt_mask_eval_args; -1 otherwise */
int mtbt_sizeof_mask_eval_args(int which);

/* ---------------------------------------------------------------------------------------------
 * Surface distances between pairs of bit-packed planes (csrc/surface_dist.hip): the records from which the host forms the
 * Hausdorff distance, its percentile, the average symmetric surface distance and the normalised surface Dice (MedPy's
 * definitions; `metrics.SurfaceDistanceMetrics`).  Packed layout and alignment as in the section above (planes 8-byte aligned,
 * 8-byte accesses only); bits X >= W never count, whatever they hold.
 * For a plane M its EDGE SET dM holds the set pixels with at least one of their four neighbours unset or outside the image
 * (M ^ binary_erosion(M, 4-connected cross, border_value = 0)).  For a pair (A, B) the directed list A->B holds, for every pixel
 * of dA in row-major order, d2 = min over dB of (dy^2 + dx^2), an exact integer below 2^29; B->A likewise; the pooled list is A->B
 * followed by B->A.  A pair with dA or dB empty is UNDEFINED: all its records are zero, n_edge apart.
 *   a, b      [n][H][pitch] packed planes
 *   tol2      squared tolerance in pixels: n_within counts d2 <= tol2
 *   Q, q[]    0..4 quantiles, each in [0, 1]
 *   n_edge    uint32 [n][2]        |dA|, |dB|
 *   max_d2    uint32 [n][2]        largest d2 of A->B, of B->A
 *   n_within  uint32 [n][2]        items with d2 <= tol2 of A->B, of B->A
 *   sum_d     double [n][2]        sum of sqrt(d2) in a fixed order: the same inputs give the same bits on every run
 *   rank_d2   uint32 [n][Q][3][2]  for the segments A->B, B->A, pooled of length m: the order statistics (0-based, ascending) at
 *                                  lo = floor(q * (m - 1)) and min(lo + 1, m - 1), q * (m - 1) being ONE IEEE double product (the
 *                                  host recomputes it for the interpolation weight); zeros for m == 0.  May be NULL when Q == 0.
 * Every output word is defined after the call: the caller does not pre-zero.  Asynchronous on `stream`, no host synchronisation,
 * no global atomics, deterministic, graph-capturable.  The pairs are taken in groups that share `workspace`
 * (>= mtbt_surface_distances_workspace_bytes(n, H, W), 16-byte aligned; the query returns MTBT_EINVAL for a shape refused below).
 * MTBT_EINVAL before any launch: NULL a or a NULL pointer member (rank_d2 only with Q > 0, workspace only when the query is > 0),
 * n < 0, H or W outside [1, 16384], pitch != 8 * ceil(W / 64), Q outside [0, 4], a q outside [0, 1] or NaN, workspace_bytes below
 * the query.  MTBT_EALIGN: a / b / sum_d not 8-byte, workspace not 16-byte, the other outputs not 4-byte aligned.  n == 0 launches
 * nothing. */
typedef struct mtbt_surface_args {
  const uint8_t* a;        /* [n][H][pitch] */
  const uint8_t* b;        /* [n][H][pitch] */
  void* workspace;
  int64_t workspace_bytes;
  uint32_t* n_edge;        /* [n][2] */
  uint32_t* max_d2;        /* [n][2] */
  uint32_t* n_within;      /* [n][2] */
  double* sum_d;           /* [n][2] */
  uint32_t* rank_d2;       /* [n][Q][3][2] */
  double q[4];
  int32_t n, H, W, pitch;
  uint32_t tol2;
  int32_t Q;
} mtbt_surface_args;
int64_t mtbt_surface_distances_workspace_bytes(int n, int H, int W);
int mtbt_surface_distances(const mtbt_surface_args* a, void* stream);
/* sizeof() of the struct above as the library was compiled: which = 0 mtbt_surface_args; -1 otherwise */
int mtbt_sizeof_surface_args(int which);

/* ---------------------------------------------------------------------------------------------
 * Connected components of bit-packed planes (csrc/components.hip; `postprocess.label_components`, `filter_components`,
 * `metrics.LesionMetrics`).  Packed layout and alignment as in the two sections above (planes 8-byte aligned, 8-byte accesses only);
 * bits X >= W never count, whatever they hold.
 * mtbt_label_components: two set pixels belong together when a path of set pixels joins them, a step going to one of the 4
 * (connectivity 4) or 8 (connectivity 8) neighbours.  The components of a plane are numbered 1 .. n_components in row-major order of
 * their FIRST pixel, the one with the smallest flat index y * W + x (the numbering of scipy.ndimage.label); 0 is background.
 *   packed        [n][H][pitch]
 *   other         [n][H][pitch] a second stack, or NULL (then inter is NULL too)
 *   labels        int32  [n][H][W] the label map; NULL: not written (the workspace still holds it for mtbt_select_components)
 *   n_components  int32  [n]       the true count, never capped
 *   area          uint32 [n][C]    pixels of id i at [i - 1], for i <= min(n_components, C), C = max_components in [1, 65536]
 *   box           int32  [n][C][4] x1, y1, x2, y2 with exclusive maxima: x1 <= X < x2 (the crop rule of mtbt_pack_masks)
 *   first         int32  [n][C]    flat index of the first pixel
 *   inter         uint32 [n][C]    popcount(component & other's plane)
 * The rows of the four tables beyond n_components are zero.  Every output word is defined after the call: the caller does not pre-zero.
 * The result is a pure function of the input (union by minimum index: the root of a component is its first pixel; integer atomics only).
 * mtbt_select_components: `packed` and `workspace` as given to (and left by) the LAST mtbt_label_components call with the same n, H, W.
 * A component is kept when area >= min_area and, with keep_largest = k > 0, it is among the k largest of its plane by area, ties going
 * to the lower id; exact for every component, also ids above max_components (the workspace holds the area of every id).
 *   out     [n][H][pitch] the kept components; every byte is written, padding bits zero
 *   n_kept  int32 [n]
 * Both: asynchronous on `stream`, no host synchronisation, no workgroup waits on another, graph-capturable.  `workspace`:
 * >= mtbt_components_workspace_bytes(n, H, W) bytes, 16-byte aligned (about 6 bytes per pixel; the query returns MTBT_EINVAL for a shape
 * refused below).  MTBT_EINVAL before any launch: NULL args or a NULL pointer member (labels may be NULL; other and inter only together;
 * workspace only when the query is 0), n < 0, H or W outside [1, 16384], H * W >= 2^31, pitch != 8 * ceil(W / 64), a connectivity other
 * than 4 or 8, max_components outside [1, 65536], keep_largest < 0, workspace_bytes below the query.  MTBT_EALIGN: packed / other / out
 * not 8-byte, workspace not 16-byte, the other pointers not 4-byte aligned.  n == 0 launches nothing. */
typedef struct mtbt_components_args {
  const uint8_t* packed;   /* [n][H][pitch] */
  const uint8_t* other;    /* [n][H][pitch] or NULL */
  void* workspace;
  int64_t workspace_bytes;
  int32_t* labels;         /* [n][H][W] or NULL */
  int32_t* n_components;   /* [n] */
  uint32_t* area;          /* [n][C] */
  int32_t* box;            /* [n][C][4] */
  int32_t* first;          /* [n][C] */
  uint32_t* inter;         /* [n][C] or NULL */
  int32_t n, H, W, pitch;
  int32_t connectivity;    /* 4 or 8 */
  int32_t max_components;  /* C */
} mtbt_components_args;
typedef struct mtbt_select_components_args {
  const uint8_t* packed;   /* [n][H][pitch] */
  void* workspace;
  int64_t workspace_bytes;
  uint8_t* out;            /* [n][H][pitch] */
  int32_t* n_kept;         /* [n] */
  int32_t n, H, W, pitch;
  uint32_t min_area;
  int32_t keep_largest;    /* 0: no limit */
} mtbt_select_components_args;
int64_t mtbt_components_workspace_bytes(int n, int H, int W);
int mtbt_label_components(const mtbt_components_args* a, void* stream);
int mtbt_select_components(const mtbt_select_components_args* a, void* stream);
/* sizeof() of the structs above as the library was compiled: which = 0 mtbt_components_args, 1 mtbt_select_components_args; -1 otherwise */
int mtbt_sizeof_components_args(int which);

/* ---------------------------------------------------------------------------------------------
 * Polygons -> bit-packed planes (csrc/polygon_fill.hip; `postprocess.fill_polygons`, `yolo_seg_planes`,
 * `preprocess.augment_samples_seg`).  Packed layout and alignment as in the sections above (planes 8-byte aligned, 8-byte accesses only).
 * THE FILL RULE is this project's own and exact in integers (tests/polygon_reference.py restates it):
 *   Quantisation  a vertex coordinate v, in pixels of the target plane, is given as fixed point q = rint(float32(v) * 16), round half
 *                 to even, int32 (the caller quantises).  Pixel (X, Y) has its centre at (16 X + 8, 16 Y + 8).
 *   Crossing      an edge a -> b of the closed polygon (the last vertex joins the first) crosses the scanline yc = 16 Y + 8 when
 *                 (ay <= yc) != (by <= yc); a horizontal edge never crosses.
 *   Left          with the crossing edge oriented so that ay < by, the pixel is left of it when
 *                 (bx - ax) * (yc - ay) - (xc - ax) * (by - ay) > 0, in int64.
 *   Even-odd      the pixel is inside the polygon when the number of crossing edges it is left of is odd.
 *   Planes        a plane is the union (OR) of its polygons, each filled on its own; a polygon of fewer than 3 vertices fills nothing.
 *   Clip          an optional rectangle (x0, y0, x1, y1) per plane, int32, half-open in pixel indices, zeroes everything outside it.
 * The result does not depend on the starting vertex or the winding; two polygons that share an edge tile the pixels without overlap or
 * gap; a rectangle sets exactly q(x1) <= 16 X + 8 < q(x2), q(y1) <= 16 Y + 8 < q(y2).
 *   vertices       int32 [n_vertices][2] x, y
 *   poly_offsets   int32 [n_polys + 1]: polygon p owns the vertices poly_offsets[p] .. poly_offsets[p + 1] - 1
 *   plane_offsets  int32 [n + 1]: plane j owns the polygons plane_offsets[j] .. plane_offsets[j + 1] - 1
 *   clip           int32 [n][4] or NULL
 *   out            [n][H][pitch]; EVERY byte is written, padding bits X >= W are zero: the caller never pre-zeroes
 *   area           uint32 [n] or NULL: the popcount of the plane
 *   box            int32 [n][4] or NULL: the tight x1, y1, x2, y2 with exclusive maxima (the convention of mtbt_label_components);
 *                  all zero for an empty plane
 * area and box are fully defined after the call (the entry point clears them on the stream before the launch).  Integer arithmetic
 * and integer atomics only: the result is a pure function of the input.
 * CLAMPING: the tables live on the device, so the library cannot validate them.  The kernel clamps every offset it reads into
 * [0, n_polys] or [0, n_vertices] (a decreasing pair is an empty range) and every coordinate into [-2^24, 2^24], so that the products
 * fit int64; its loop bounds then come from the host-side counts, and no table can make it read outside `vertices` or spin.
 * Asynchronous on `stream`, no host synchronisation, no workspace, graph-capturable.
 * MTBT_EINVAL before any launch: NULL a / out / poly_offsets / plane_offsets, NULL vertices with n_vertices > 0, n < 0, n_polys < 0,
 * n_vertices < 0, H < 1, W < 1, H * W >= 2^31, pitch != 8 * ceil(W / 64).  MTBT_EALIGN: out not 8-byte aligned, an int32 / uint32 pointer
 * not 4-byte aligned.  n == 0 launches nothing. */
typedef struct mtbt_fill_polygons_args {
  const int32_t* vertices;       /* [n_vertices][2] x, y, fixed point 1/16 px */
  const int32_t* poly_offsets;   /* [n_polys + 1] into vertices */
  const int32_t* plane_offsets;  /* [n + 1] into polygons */
  const int32_t* clip;           /* [n][4] x0, y0, x1, y1, or NULL */
  uint8_t* out;                  /* [n][H][pitch] */
  uint32_t* area;                /* [n] or NULL */
  int32_t* box;                  /* [n][4] or NULL */
  int32_t n, n_polys, n_vertices, H, W, pitch;
} mtbt_fill_polygons_args;
int mtbt_fill_polygons(const mtbt_fill_polygons_args* a, void* stream);
/* sizeof() of the struct above as the library was compiled: which = 0 mtbt_fill_polygons_args; -1 otherwise */
int mtbt_sizeof_fill_polygons_args(int which);

/* ---------------------------------------------------------------------------------------------
 * Exact Euclidean distance transform of bit-packed planes (csrc/distance_transform.hip; `postprocess.distance_transform`,
 * `signed_distance`).  Packed layout and alignment as in the surface and component sections above (planes 8-byte aligned, 8-byte
 * accesses only, pitch = 8 * ceil(W / 64)); bits X >= W never count, whatever they hold.
 * THE DISTANCE RULE, exact in integers (tests/edt_reference.py restates it):
 *   d2_set    uint32 [n][H][W]  at pixel (x, y) the minimum of dy^2 + dx^2 over the SET pixels of the plane; 0 on a set pixel
 *                               (scipy.ndimage.distance_transform_edt(~m) squared)
 *   d2_unset  uint32 [n][H][W]  the same over the UNSET pixels inside the image; 0 on an unset pixel (distance_transform_edt(m) squared)
 *   Sentinel  where no such pixel exists (d2_set of an empty plane, d2_unset of a full one) every word of that map is 0xFFFFFFFF.
 *             Outside the image is neither set nor unset.
 * Either output may be NULL (not both): the other map is still defined.  H, W in [1, 16384], so d2 < 2^29.  Every output word is
 * defined after the call: the caller does not pre-zero.  Asynchronous on `stream`, no host synchronisation, no global atomics,
 * deterministic, graph-capturable.  The planes are taken in chunks that share `workspace`
 * (>= mtbt_distance_transform_workspace_bytes(n, H, W), 16-byte aligned; the query returns MTBT_EINVAL for a shape refused below).
 * MTBT_EINVAL before any launch: NULL args or packed, both outputs NULL, workspace NULL when the query is > 0, n < 0, H or W outside
 * [1, 16384], pitch != 8 * ceil(W / 64), workspace_bytes below the query.  MTBT_EALIGN: packed not 8-byte, workspace not 16-byte, an
 * output not 4-byte aligned.  n == 0 launches nothing. */
typedef struct mtbt_distance_transform_args {
  const uint8_t* packed;   /* [n][H][pitch] */
  void* workspace;
  int64_t workspace_bytes;
  uint32_t* d2_set;        /* [n][H][W] or NULL */
  uint32_t* d2_unset;      /* [n][H][W] or NULL */
  int32_t n, H, W, pitch;
} mtbt_distance_transform_args;
int64_t mtbt_distance_transform_workspace_bytes(int n, int H, int W);
int mtbt_distance_transform(const mtbt_distance_transform_args* a, void* stream);

/* The region terms of the segmentation loss over those maps (`loss.seg_region_loss`, `SegRegionLoss`, `TrainStep(seg_dice_weight=,
 * seg_boundary_weight=)`); not terms of the reference's loss.  With z = logits + bias (bias: one float on the device, or NULL),
 * p = sigmoid(z), t the target bit of the packed plane and N = H * W:
 *   THE DICE RULE      per image I = sum p t, P = sum p, T = sum t; dice = mean over images of 1 - (2 I + smooth) / (P + T + smooth)
 *                      (MONAI's DiceLoss(sigmoid=True) per sample: one `smooth` in numerator and denominator).
 *   THE BOUNDARY RULE  phi = +sqrt(d2_set) on an unset pixel, -(sqrt(d2_unset) - 1) on a set pixel (Kervadec et al. 2019, one_hot2dist:
 *                      edt(neg) * neg - (edt(pos) - 1) * pos); phi = 0 wherever the map it needs holds the sentinel, so an empty and a
 *                      full plane contribute nothing; boundary = (1 / (B N)) sum phi p.
 *   out[0..2]          dice, boundary, w_dice * dice + w_boundary * boundary (fp32)
 *   d_logits           fp32 [B][H][W] or NULL: the gradient of out[2] with respect to the logits, written, or with accumulate = 1 ADDED
 *                      to what the buffer holds
 * Arithmetic: sigmoid in fp32; the per-image sums in fp64 in a fixed order (the same inputs give the same bits on every run); the Dice
 * gradient's per-image factor -[2 t (P + T + smooth) - (2 I + smooth)] / (P + T + smooth)^2 * w_dice / B in fp64, cast once; sqrt of
 * (double)d2, cast to fp32.  d2_set and d2_unset (the outputs of mtbt_distance_transform for `targets`) are given both or neither; they
 * may be NULL only with w_boundary == 0 (phi is then 0).  Asynchronous on `stream`, no host synchronisation, no atomics, graph-capturable.
 * `workspace`: >= mtbt_seg_region_loss_workspace_bytes(B, H, W) bytes, 16-byte aligned (the query returns MTBT_EINVAL for a shape refused
 * below).  MTBT_EINVAL before any launch: NULL args / logits / targets / out / workspace, B outside [1, 65535], H or W outside [1, 16384],
 * pitch != 8 * ceil(W / 64), smooth, w_dice or w_boundary negative, NaN or infinite, one map without the other, w_boundary != 0 without
 * maps, accumulate other than 0 or 1, workspace_bytes below the query.  MTBT_EALIGN: targets not 8-byte, workspace not 16-byte, the
 * other pointers not 4-byte aligned. */
typedef struct mtbt_seg_region_args {
  const float* logits;       /* [B][H][W] */
  const float* bias;         /* 1 value on the device, or NULL */
  const uint8_t* targets;    /* [B][H][pitch] */
  const uint32_t* d2_set;    /* [B][H][W] or NULL */
  const uint32_t* d2_unset;  /* [B][H][W] or NULL */
  float* d_logits;           /* [B][H][W] or NULL */
  void* workspace;
  int64_t workspace_bytes;
  float* out;                /* [3] */
  int32_t B, H, W, pitch;
  float smooth, w_dice, w_boundary;
  int32_t accumulate;
} mtbt_seg_region_args;
int64_t mtbt_seg_region_loss_workspace_bytes(int B, int H, int W);
int mtbt_seg_region_loss(const mtbt_seg_region_args* a, void* stream);
/* sizeof() of the structs above as the library was compiled: which = 0 mtbt_distance_transform_args, 1 mtbt_seg_region_args; -1 otherwise */
int mtbt_sizeof_distance_args(int which);

/* ---------------------------------------------------------------------------------------------
 * Bit-packed planes -> polygons (csrc/contours.hip; `postprocess.trace_contours`, `contour_polygons`, `yolo_seg_rows`,
 * `labelme_shapes`): the way back from mtbt_fill_polygons.  Packed layout, alignment and shape limits as mtbt_label_components (planes
 * 8-byte aligned, 8-byte accesses only, pitch = 8 * ceil(W / 64), bits X >= W never count, H and W in [1, 16384]); everything outside
 * the plane is unset.
 * THE CONTOUR RULE, exact in integers (tests/contour_reference.py restates it):
 *   Lattice     pixel (X, Y) is the square [X, X + 1] x [Y, Y + 1].  A vertex is an integer point (x, y), 0 <= x <= W, 0 <= y <= H;
 *               its key is y * (W + 1) + x.
 *   Edges       a set pixel contributes up to four directed boundary edges: its top side (X, Y) -> (X + 1, Y) heading E when the pixel
 *               above is unset, its right side (X + 1, Y) -> (X + 1, Y + 1) heading S when the pixel to the right is unset, its bottom
 *               side (X + 1, Y + 1) -> (X, Y + 1) heading W when the pixel below is unset, its left side (X, Y + 1) -> (X, Y) heading N
 *               when the pixel to the left is unset.  The set pixel always lies to the right of the direction of travel.
 *   Successor   the edge that follows e starts where e ends.  Where two edges start there the vertex is a saddle (exactly two diagonal
 *               pixels set): connectivity 4 takes the edge that turns right, in the cycle E -> S -> W -> N -> E, and the contour stays on
 *               the same pixel; connectivity 8 takes the edge that turns left and the contour crosses to the diagonal pixel.  The
 *               successor is a permutation of the edges; its cycles are the contours.
 *   Vertices    the vertices of a contour are the start points of those of its edges whose predecessor has a different direction: no
 *               three consecutive vertices are collinear, consecutive edges alternate between horizontal and vertical.  A contour may
 *               pass through a lattice vertex twice; it never repeats a directed edge.
 *   Start       the start point of the contour's E-heading edge with the smallest key (always a vertex of the contour); the vertices are
 *               listed from there in successor order.
 *   Order       the contours of a plane are sorted by the key of their start, ascending.
 *   Area        area2 = sum over i of x_i * y_{i+1} - x_{i+1} * y_i, int64: > 0 for an outer contour, < 0 for a hole.
 * What follows from the rule: every contour filled on its own by mtbt_fill_polygons (vertices as pixel coordinates: multiples of 16 in its
 * fixed point against centres at 16 X + 8, so no tie) and the fills XOR-ed give back the plane; the sum of area2 is twice the popcount;
 * the outer contours, in order, are the components of mtbt_label_components at the same connectivity in id order, the k-th starting at
 * the k-th component's first pixel; the holes are the components of the complement, at the complementary connectivity, that do not reach
 * the outside.
 *   n_vertices  int32 [n]        the true number of contour vertices of the plane, never capped (<= 2 H W + 2)
 *   n_contours  int32 [n]        the true count, or -1 when n_vertices > V = max_vertices
 *   vertices    int32 [n][V][2]  x, y: the contours of the plane back to back, in contour order
 *   offset      int32 [n][C]     first vertex row of contour i, C = max_contours in [1, 65536]
 *   count       int32 [n][C]     its number of vertices
 *   area2       int64 [n][C]
 *   box         int32 [n][C][4]  x1, y1, x2, y2 over its vertices, lattice coordinates: for an outer contour the pixel box with exclusive
 *                                maxima, the convention of mtbt_label_components
 *   start       int32 [n][C]     the key of its start
 * The tables hold the first min(n_contours, C) contours; the rows beyond are zero.  OVERFLOW: a plane with n_vertices > V has zero
 * tables and n_contours = -1; its vertex rows are unspecified (nothing is written outside them).  Every other output word is defined
 * after the call: the caller does not pre-zero.  Vertex rows from n_vertices on are not written.
 * COUNT ONLY: vertices == NULL with every table pointer NULL (n_contours is then ignored, and so are workspace, max_contours and
 * max_vertices): only n_vertices is written, by one pass that counts 2 x 2 pixel patterns (one vertex where one or three of the four
 * pixels round a lattice point are set, two where exactly two diagonal ones are) -- no ranking, no workspace.
 * Asynchronous on `stream`, no host synchronisation, graph-capturable, a pure function of the input (integer atomics only).  No
 * workgroup waits on another; every loop bound is a host-side number (H, W, V, a round count from min(V, 2 H W + 2)), never device
 * data.  `workspace`: >= mtbt_contours_workspace_bytes(n, H, W, max_vertices) bytes, 16-byte aligned (about 32 bytes per vertex of
 * capacity; the query returns MTBT_EINVAL for a shape refused below).
 * MTBT_EINVAL before any launch: NULL args, packed or n_vertices; n < 0, H or W outside [1, 16384], pitch != 8 * ceil(W / 64); a
 * connectivity other than 4 or 8; and, unless the call is count only: a NULL vertices, n_contours or table pointer (so also tables
 * given without vertices), max_contours outside [1, 65536], max_vertices < 0, workspace NULL or workspace_bytes below the query.
 * MTBT_EALIGN: packed or area2 not 8-byte, workspace not 16-byte, the other pointers not 4-byte aligned.  n == 0 launches nothing. */
typedef struct mtbt_contours_args {
  const uint8_t* packed;   /* [n][H][pitch] */
  void* workspace;
  int64_t workspace_bytes;
  int32_t* n_vertices;     /* [n] */
  int32_t* n_contours;     /* [n] */
  int32_t* vertices;       /* [n][V][2] or NULL: count only */
  int32_t* offset;         /* [n][C] */
  int32_t* count;          /* [n][C] */
  int64_t* area2;          /* [n][C] */
  int32_t* box;            /* [n][C][4] */
  int32_t* start;          /* [n][C] */
  int32_t n, H, W, pitch;
  int32_t connectivity;    /* 4 or 8 */
  int32_t max_contours;    /* C */
  int32_t max_vertices;    /* V, per plane */
  int32_t reserved;        /* 0 */
} mtbt_contours_args;
int64_t mtbt_contours_workspace_bytes(int n, int H, int W, int max_vertices);
int mtbt_trace_contours(const mtbt_contours_args* a, void* stream);

/* Bit-packed planes -> COCO run lengths (`postprocess.rle_encode`, `coco_segm_results`).  Same planes as above.
 * THE RUN RULE (tests/contour_reference.py restates it): the pixels of a plane read COLUMN-MAJOR, index x * H + y, fall into runs of
 * equal pixels; the runs are listed from a run of UNSET pixels, which is 0 when pixel (0, 0) is set, and alternate from there.  Their
 * sum is H * W.  This is the uncompressed `counts` of a COCO RLE of size [H, W].
 *   n_runs  int32  [n]     the true number of runs, never capped (<= H W + 1)
 *   counts  uint32 [n][R]  the first min(n_runs, R) runs, R = max_runs >= 0; the words from n_runs on are not written; NULL: only
 *                          n_runs is written (then max_runs is ignored)
 * Asynchronous on `stream`, no host synchronisation, no atomics, graph-capturable; loop bounds are host-side numbers.  `workspace`:
 * >= mtbt_rle_workspace_bytes(n, H, W) bytes, 16-byte aligned (8 bytes per column and 128-row band).
 * MTBT_EINVAL before any launch: NULL args, packed or n_runs; workspace NULL when the query is > 0; n < 0, H or W outside [1, 16384],
 * pitch != 8 * ceil(W / 64), max_runs < 0 with counts given, workspace_bytes below the query.  MTBT_EALIGN: packed not 8-byte, workspace not 16-byte, counts or
 * n_runs not 4-byte aligned.  n == 0 launches nothing. */
typedef struct mtbt_rle_args {
  const uint8_t* packed;   /* [n][H][pitch] */
  void* workspace;
  int64_t workspace_bytes;
  uint32_t* counts;        /* [n][R] or NULL */
  int32_t* n_runs;         /* [n] */
  int32_t n, H, W, pitch;
  int32_t max_runs;        /* R */
  int32_t reserved;        /* 0 */
} mtbt_rle_args;
int64_t mtbt_rle_workspace_bytes(int n, int H, int W);
int mtbt_rle_encode(const mtbt_rle_args* a, void* stream);
/* sizeof() of the structs above as the library was compiled: which = 0 mtbt_contours_args, 1 mtbt_rle_args; -1 otherwise */
int mtbt_sizeof_contours_args(int which);

/* ---------------------------------------------------------------------------------------------
 * Measurements of regions of bit-packed planes or label maps (csrc/measure.hip, csrc/measure_exact.h; `postprocess.measure_regions`,
 * `measure_components`, `region_properties`, `measure_detections`): sums, the lattice convex hull, Feret diameters, the minimum-area
 * rectangle.  Packed layout, alignment and shape limits as mtbt_label_components (planes 8-byte aligned, 8-byte accesses only,
 * pitch = 8 * ceil(W / 64), bits X >= W never count, H and W in [1, 16384]).
 * THE MEASURE RULE, exact in integers (tests/measure_reference.py restates it):
 *   Regions     PLANE MODE (labels == NULL): region 1 of plane p is the set bits of packed[p] with X < W; n planes, one region each,
 *               max_regions = C = 1.  LABEL MODE (labels int32 [n][H][W], as mtbt_label_components writes them; packed may be NULL):
 *               region i is {label == i} for 1 <= i <= C = max_regions in [1, 65536].  Labels <= 0 are background; labels > C belong
 *               to no reported region but are "not this region" for the perimeter.  Any label map will do; a region need not be
 *               connected in either mode.  Pixel (X, Y) is the square [X, X + 1] x [Y, Y + 1], the lattice of THE CONTOUR RULE.
 *   Sums        sums uint64 [n][C][8] = area, perimeter (the unit pixel sides of the region whose 4-neighbour across the side is outside
 *               the plane or not in the region), sum X, sum Y, sum X^2, sum X Y, sum Y^2, 0 over the region's pixel indices X, Y.
 *   Hull        the convex hull of the region's closed pixel squares, i.e. of their lattice corners, strictly convex (a point collinear
 *               with its neighbours is no vertex), listed from the vertex with the smallest key y * (W + 1) + x in the sense of an outer
 *               contour of THE CONTOUR RULE (E -> S -> W -> N, the region on the right).  n_hull int32 [n][C] is the true count h, never
 *               capped; hull int32 [n][C][Vh][2] (or NULL) holds the first min(h, Vh) vertices x, y, the rows after them zero,
 *               Vh = max_hull >= 4; hull_area2 int64 [n][C] by the contour rule's area2 formula (> 0).  No measurement depends on max_hull.
 *   Calipers    over the FULL hull p_0 .. p_{h-1}, p_h = p_0, e_i = p_{i+1} - p_i, len2_i = |e_i|^2, cross(a, b) = ax by - ay bx:
 *     diameter    d2 = max |p_i - p_j|^2; the pair (a, b) = (p_i, p_j) with the smallest i, then the smallest j > i, among the maxima.
 *     extent      with u = p_j - p_i of that pair, perp = max_q cross(u, q - p_i) - min_q cross(u, q - p_i) over the hull vertices q
 *                 (the extent perpendicular to the diameter is perp / sqrt(d2)).
 *     width       h_i = max_q |cross(e_i, q - p_i)|; the minimum over i of h_i^2 / len2_i, compared as exact fractions, a tie going to
 *                 the smallest i: w_edge = i, w_num = h_i, w_len2 = len2_i, w_vertex = the smallest hull index q attaining h_i.
 *     rectangle   tmin_i, tmax_i = min, max over q of dot(e_i, q - p_i), t_i = tmax_i - tmin_i; the minimum over i of
 *                 h_i t_i / len2_i (the area), exact, a tie to the smallest i: r_edge, r_h, r_t, r_tmin, r_len2.
 *               The cross-multiplied fractions reach 2^87: they are compared in 128 bits (csrc/measure_exact.h), never in floating
 *               point or wrapped 64-bit words.
 *   Tables      caliper int64 [n][C][8] = d2, perp, w_num, w_len2, r_h, r_t, r_tmin, r_len2;
 *               caliper_at int32 [n][C][8] = xa, ya, xb, yb, w_edge, w_vertex, r_edge, 0.
 * An empty region (or id) has every word zero; a non-empty one has n_hull >= 4.  Every output word is defined after the call: the caller
 * does not pre-zero.  Asynchronous on `stream`, no host synchronisation, graph-capturable, a pure function of the input (integer atomics
 * only, no floating point).  No workgroup waits on another; every loop bound is a host-side number (H, W, 2 (H + 1)) or a count the
 * kernel has clamped by one.  `workspace`: >= mtbt_measure_workspace_bytes(n, H, W, max_regions) bytes, 16-byte aligned: 8 bytes per
 * (region, lattice row) of the planes of one launch group (the query returns MTBT_EINVAL for a shape refused below).
 * MTBT_EINVAL before any launch: NULL args, sums, n_hull, hull_area2, caliper or caliper_at; packed and labels both NULL; n < 0, H or W
 * outside [1, 16384], pitch != 8 * ceil(W / 64); max_regions outside [1, 65536], or != 1 in plane mode; max_hull < 4; a non-zero
 * reserved field; workspace NULL or workspace_bytes below the query.  MTBT_EALIGN: packed, sums, hull_area2 or caliper not 8-byte,
 * workspace not 16-byte, the other pointers not 4-byte aligned.  n == 0 launches nothing. */
typedef struct mtbt_measure_args {
  const uint8_t* packed;   /* [n][H][pitch]; may be NULL in label mode */
  const int32_t* labels;   /* [n][H][W] or NULL: plane mode */
  void* workspace;
  int64_t workspace_bytes;
  uint64_t* sums;          /* [n][C][8] */
  int32_t* n_hull;         /* [n][C] */
  int32_t* hull;           /* [n][C][Vh][2] or NULL */
  int64_t* hull_area2;     /* [n][C] */
  int64_t* caliper;        /* [n][C][8] */
  int32_t* caliper_at;     /* [n][C][8] */
  int32_t n, H, W, pitch;
  int32_t max_regions;     /* C */
  int32_t max_hull;        /* Vh */
  int32_t reserved[2];     /* 0 */
} mtbt_measure_args;
int64_t mtbt_measure_workspace_bytes(int n, int H, int W, int max_regions);
int mtbt_measure_regions(const mtbt_measure_args* a, void* stream);
/* sizeof() of the struct above as the library was compiled: which = 0 mtbt_measure_args; -1 otherwise */
int mtbt_sizeof_measure_args(int which);

/* Weight gradient of a k x k convolution (any stride / padding; 1x1 and the 2x2 stride-2 downsample included), bf16 (MFMA) or fp32 operands:
 *   dw[k][r][s][c] (fp32, packed [K][R*S*C] like the forward weight) (+)= sum_p dy[p][k] * x[n][y*stride + r - pad][x*stride + s - pad][c]
 * x [N,H,W,C], dy [N,Ho,Wo,K] (Ho = (H + 2 pad - R) / stride + 1) NHWC with pixel / batch strides in elements (multiples of 8; C % 8 == K % 8 == 0;
 * fp32 operands -- the parity mode, a VALU kernel -- multiples of 4).  accumulate != 0
 * adds to dw (gradient accumulation into a flat bucket).  Deterministic: per-slice fp32 partials in `workspace`
 * (>= mtbt_conv_wgrad_workspace_bytes) summed in a fixed order.  This is what autograd computes for `Conv2d.weight.grad`. */
int64_t mtbt_conv_wgrad_workspace_bytes(int N, int H, int W, int C, int K, int R, int S);
int mtbt_conv_wgrad(const void* x, const void* dy, float* dw, int N, int H, int W, int C, int K, int R, int S, int pad, int stride,
                    int64_t x_batch_stride, int32_t x_pixel_stride, int64_t dy_batch_stride, int32_t dy_pixel_stride, int dtype,
                    int accumulate, void* workspace, int64_t workspace_bytes, void* stream);
/* The same with an activation applied to x while it is staged (x_act = MTBT_ACT_GELU_POLY; bf16, 1 x 1): x is a kept PRE-activation,
 * dw[k][c] (+)= sum_p dy[p][k] * gelu(x[p][c]) -- the fc2 weight gradient behind mtbt_convnext_mlp_fused_train. */
int mtbt_conv_wgrad_xact(const void* x, const void* dy, float* dw, int N, int H, int W, int C, int K, int R, int S, int pad, int stride,
                         int64_t x_batch_stride, int32_t x_pixel_stride, int64_t dy_batch_stride, int32_t dy_pixel_stride, int dtype,
                         int x_act, int accumulate, void* workspace, int64_t workspace_bytes, void* stream);
/* The same plus the bias gradient dbias[k] (+)= sum_p dy[p][k] (`Conv2d.bias.grad`, `Linear.bias.grad`, and the sum_p dy the layer-scale
 * gradient needs) from the dY fragments the kernel holds anyway: the workgroups of the first input-channel tile and tap multiply them
 * with a fragment of ones -- no separate pass over dy. */
int mtbt_conv_wgrad_bias(const void* x, const void* dy, float* dw, float* dbias, int N, int H, int W, int C, int K, int R, int S, int pad,
                         int stride, int64_t x_batch_stride, int32_t x_pixel_stride, int64_t dy_batch_stride, int32_t dy_pixel_stride,
                         int dtype, int accumulate, void* workspace, int64_t workspace_bytes, void* stream);

/* Pointwise pieces of the backward pass.  mtbt_act_backward: dz[i] = dy[i] * act'(z[i]) for MTBT_ACT_* (z = the PRE-activation the
 * training forward keeps; n % 8 == 0; dtype f32 or bf16 for all three arrays).  mtbt_channel_sum: out[c] (+)= sum_p x[p][c] (* x2[p][c]
 * when x2 != NULL) over `pixels` rows of pixel_stride elements (C % 8 == 0): the gradient of a conv bias / BatchNorm shift, and
 * with x2 of a BatchNorm scale / layer-scale; deterministic. */
int mtbt_act_backward(const void* dy, const void* z, void* dz, int64_t n, int act, int dtype, void* stream);
int64_t mtbt_channel_sum_workspace_bytes(int64_t pixels, int C);
int mtbt_channel_sum(const void* x, const void* x2, int64_t pixels, int C, int32_t pixel_stride, int32_t pixel_stride2, int dtype,
                     float* out, int accumulate, void* workspace, int64_t workspace_bytes, void* stream);

/* out[p][c] = a[c] * x1[p][c] + b[c] * x2[p][c] + d[c] over dense [pixels][C] tensors (C % 8 == 0; f32 or bf16): the elementwise pass
 * of a batch-statistic BatchNorm backward, dx = (gamma/sigma) (dy - mean(dy) - xhat mean(dy xhat)), written on (dy, pre-activation). */
int mtbt_channel_affine2(const void* x1, const void* x2, const float* a, const float* b, const float* d, void* out, int64_t pixels, int C,
                         int dtype, void* stream);

/* LayerNorm backward over the channels of every pixel (timm ConvNeXt block `norm`, downsample LayerNorm2d): x, dy, dx (and the
 * optional xhat output) dense [pixels][C], f32 or bf16; w = gamma [C] f32.  dx = rstd (g - mean_c g - xhat mean_c(g xhat)), g = dy gamma.
 * d gamma = mtbt_channel_sum(dy, xhat), d beta = mtbt_channel_sum(dy). */
int mtbt_layernorm_backward_nhwc(const void* x, const void* dy, const float* w, float eps, void* dx, void* xhat, int64_t pixels, int C,
                                 int dtype, int accumulate /* != 0: dx += (dx already holds another consumer's gradient) */, void* stream);

/* The same in ONE pass together with the parameter gradients (the training plan's form): dx (+)= ...; dgamma (+)= sum_p dy * xhat;
 * dbeta (+)= sum_p dy.  Per-wave partial rows in `workspace` (>= mtbt_layernorm_backward_params_workspace_bytes), summed in a fixed
 * order.  No xhat tensor, no separate channel-sum passes over dy. */
int64_t mtbt_layernorm_backward_params_workspace_bytes(int64_t pixels, int C);
int mtbt_layernorm_backward_params_nhwc(const void* x, const void* dy, const float* w, float eps, void* dx, int64_t pixels, int C, int dtype,
                                        int accumulate_dx, float* dgamma, float* dbeta, int accumulate_params, void* workspace,
                                        int64_t workspace_bytes, void* stream);

/* Weight gradient of a depthwise k x k convolution (stride 1, pad k/2; k = 3 or 7): dw[tap][c] (fp32, the forward tap layout [k*k][C])
 * (+)= sum_p dy[p][c] * x[p shifted by the tap][c]; x, dy dense [N,H,W,C], f32 or bf16.  Deterministic.  (Persistent workgroups over
 * 8 x 8-pixel tiles: input halo and dy tile staged in LDS, the k*k tap accumulators in registers across tiles.) */
int64_t mtbt_dwconv_wgrad_workspace_bytes(int N, int H, int W, int C, int ksize);
int mtbt_dwconv_wgrad(const void* x, const void* dy, float* dw, int N, int H, int W, int C, int ksize, int dtype, int accumulate, void* workspace,
                      int64_t workspace_bytes, void* stream);
/* the same plus dbias[c] (+)= sum_p dy[p][c] from the same launch */
int mtbt_dwconv_wgrad_bias(const void* x, const void* dy, float* dw, float* dbias, int N, int H, int W, int C, int ksize, int dtype, int accumulate,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* Fused AdamW step over a flat fp32 bucket: torch.optim.AdamW as the reference trainer configures it
 * (running_main_v3.py:732-734: lr, weight_decay 0.0005, default betas / eps), torch's single-tensor operation order, in place.
 * step >= 1 is the number of the step being taken (bias corrections use beta^step).  n need not be a multiple of 4.
 * grad_scale: optional DEVICE scalar multiplied into every gradient first (the clip coefficient, see mtbt_clip_coef). */
int mtbt_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int64_t step, const float* grad_scale, void* stream);

/* torch.optim.SGD over a flat fp32 bucket (BASELINE configs[2] names SGD; momentum / dampening / weight decay / Nesterov as torch's
 * single-tensor form; momentum_buf may be NULL when momentum == 0; step 1 initialises the buffer with the gradient). */
int mtbt_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum, float dampening,
                  float weight_decay, int nesterov, int64_t step, const float* grad_scale, void* stream);

/* Weight EMA (exponential moving average of the weights; the reference trainer has none -- this is the project's own definition).
 * Per element, after the optimiser has produced the new p:
 *     d   = (float)ema_decay        omd = (float)(1.0 - ema_decay)      host, in double, then rounded once
 *     e   = e * d                                                         one rounding
 *     e   = e + omd * p                                                   product rounded, then the sum rounded: no contraction
 * which is torch's CPU `e.mul_(d); e.add_((1 - d) * p)` bit for bit.  mtbt_adamw_step_ema / mtbt_sgd_step_ema are the steps above with
 * that update applied, in the same pass, to the p about to be stored: param and the moments come out exactly as from the plain entry
 * points, and the EMA costs one 4-byte read and one 4-byte write per parameter and no launch.  mtbt_ema_update is the same update for
 * values no optimiser steps (BatchNorm running statistics); ema and src 16-byte aligned, as mtbt_adamw_step(_ema) asks of its buffers.
 * MTBT_EINVAL for a null ema / src, n < 0 or ema_decay outside [0, 1] (NaN included); n == 0 is MTBT_OK without a launch. */
int mtbt_adamw_step_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float lr, float beta1,
                        float beta2, float eps, float weight_decay, int64_t step, const float* grad_scale, double ema_decay, void* stream);
int mtbt_sgd_step_ema(float* param, const float* grad, float* momentum_buf, float* ema, int64_t n, float lr, float momentum, float dampening,
                      float weight_decay, int nesterov, int64_t step, const float* grad_scale, double ema_decay, void* stream);
int mtbt_ema_update(float* ema, const float* src, int64_t n, double ema_decay, void* stream);

/* Gradient clipping by global norm (Trainer(gradient_clip_val=10), running_main_v3.py:826 -> torch.nn.utils.clip_grad_norm_):
 * mtbt_sumsq adds the sum of squares of one flat bucket to *out (deterministic two-level reduction; workspace >=
 * mtbt_sumsq_workspace_bytes()); after an all-reduce-free sum over the buckets, mtbt_clip_coef writes
 * coef = min(1, max_norm / (sqrt(sumsq) + 1e-6)) -- the device scalar the optimiser kernels take as `grad_scale` (NULL = 1),
 * so clipping costs no pass over the gradients and no host synchronisation. */
int64_t mtbt_sumsq_workspace_bytes(void);
int mtbt_sumsq(const float* g, int64_t n, float* out, int accumulate, void* workspace, int64_t workspace_bytes, void* stream);
int mtbt_clip_coef(const float* sumsq, float max_norm, float* coef, float* norm_out, void* stream);

/* =============================================================================================================================
 * Training step (BASELINE configs[2]-[3]; running_main_v3.py:393-445 training_step -> total_loss.backward() -> clip -> optimizer).
 * The entry points below, with mtbt_conv2d_nhwc (dgrad = the forward kernel on dY with re-laid-out weights; y2 / MTBT_ACT_D*),
 * mtbt_conv_wgrad, mtbt_dwconv_wgrad, mtbt_layernorm_backward_nhwc and mtbt_multitask_loss(_grad), are what the backward plan
 * of `ConvNeXtBiFPNYOLO.forward(x, "train")` launches (multitask_bonetumor_yolo_amd/train.py).
 * ============================================================================================================================= */

/* Training variants of the stem and the depthwise kernel: they also write what the backward pass needs.
 * stem: `raw` [N,H/4,W/4,Cout] (out_dtype) = the LayerNorm2d INPUT (conv + bias).
 * dwconv, LayerNorm form: `raw` = conv + bias (the LayerNorm input); scale / shift form: `res` is added after the activation and
 * may alias y -- the depthwise input gradient accumulating into a buffer that already holds the residual branch's gradient. */
int mtbt_stem_conv4x4_ln_train(const float* x, const float* w, const float* bias, const float* ln_w, const float* ln_b, float ln_eps,
                               void* y, void* raw, int N, int H, int W, int Cout, int out_dtype, void* stream);
int mtbt_dwconv_nhwc_train(const void* x, const void* w, const float* bias, const float* ln_w, const float* ln_b, float ln_eps,
                           const float* scale, const float* shift, int act, void* y, void* raw, const void* res, int N, int H, int W,
                           int C, int ksize, int dtype, void* stream);

/* BatchNorm2d forward, general form (every ConvBlock / DepthwiseConvBlock / ultralytics Conv BatchNorm under model.train(),
 * main_model.py:95,126-136): x dense [pixels][C]; y rows of y_pixel_stride elements (a channel slice of a C2f concat buffer,
 * main_model.py:144-173, or dense).  use_running != 0: module in eval mode (running statistics, nothing updated).  stats [2*C]
 * receives the (mean, biased variance) used -- the input of mtbt_bn_backward_nhwc.  workspace >= mtbt_bn_train_workspace_bytes. */
int mtbt_bn_forward_nhwc(const void* x, void* y, int32_t y_pixel_stride, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float momentum, float eps, int act, int64_t pixels, int C, int dtype, int use_running,
                         float* stats, void* workspace, int64_t workspace_bytes, void* stream);

/* The same with the batch statistics taken from the column sums the producing conv accumulated in its epilogue (mtbt_conv_args.colsum
 * with colsum_sq): sums [2C] = sum (x - shift), sum (x - shift)^2.  shift [C] or NULL; it may alias running_mean.  One pass over x
 * instead of two. */
int mtbt_bn_forward_sums_nhwc(const void* x, void* y, int32_t y_pixel_stride, const float* gamma, const float* beta, float* running_mean,
                              float* running_var, float momentum, float eps, int act, int64_t pixels, int C, int dtype, const float* sums,
                              const float* shift, float* stats, void* stream);

/* ... and straight from the conv's partial rows (second level and statistics in one launch).  The partial rows are CONSUMED: a tall
 * matrix (> 768 rows) is folded in place before the per-channel second level. */
int mtbt_bn_forward_partials_nhwc(const void* x, void* y, int32_t y_pixel_stride, const float* gamma, const float* beta, float* running_mean,
                                  float* running_var, float momentum, float eps, int act, int64_t pixels, int C, int dtype, float* partial,
                                  int64_t rows, int32_t pitch, const float* shift, float* stats, void* stream);

/* Backward of activation + BatchNorm2d in one operator: dy = gradient of the ACTIVATED output (rows of dy_pixel_stride elements),
 * x = the conv output the forward normalised (dense), stats as written by mtbt_bn_forward_nhwc.
 *   du = dy * act'(xhat * gamma + beta);  d beta (+)= sum du;  d gamma (+)= sum du * xhat;
 *   dx = gamma * rstd * (du - mean(du) - xhat * mean(du * xhat))     (use_running: dx = gamma * rstd * du)
 * Two passes over (dy, x), deterministic.  dgamma / dbeta may be NULL. */
int64_t mtbt_bn_backward_workspace_bytes(int64_t pixels, int C);
int mtbt_bn_backward_nhwc(const void* dy, int32_t dy_pixel_stride, const void* x, const float* stats, const float* gamma, const float* beta,
                          float eps, int act, int use_running, void* dx, float* dgamma, float* dbeta, int accumulate, int64_t pixels, int C,
                          int dtype, void* workspace, int64_t workspace_bytes, void* stream);

/* Per-step weight preparation, ONE launch for the whole network: descriptor j turns a master parameter (fp32, any strides) into the
 * dense row-major [dim0][dim1][dim2][dim3] tensor a kernel reads, in the compute dtype:
 *   dst[a][b][c][d] = src[ia*sstride0 + ib*sstride1 + ic*sstride2 + id*sstride3] * scale0[index of dim scale0_dim] * scale1[...]
 * with ix = flip[x] ? dim[x]-1-x : x.  Forward weights: KRSC; dgrad weights: C,R,S,K with R,S flipped; ConvNeXt fc2 with the layer
 * scale, DepthwiseConvBlock with its k=1 depthwise scale: per-row / per-column scale vectors.  table_dev / block_start_dev live in
 * DEVICE memory; block_start[j] = first workgroup of descriptor j (mtbt_weight_prep_blocks(elements) workgroups each). */
typedef struct mtbt_prep_desc {
  const float* src;
  void* dst;
  const float* scale0;
  const float* scale1;
  int64_t sstride[4];
  int32_t dim[4];
  int32_t flip[4];
  int32_t scale0_dim, scale1_dim;
  int32_t dst_dtype;
  int32_t src_dim3; /* > 0: the source has only src_dim3 entries along dim 3; dst[..][d >= src_dim3] = 0 (channel padding) */
} mtbt_prep_desc;
int mtbt_weight_prep_blocks(int64_t elements);
int mtbt_weight_prep(const mtbt_prep_desc* table_dev, const int32_t* block_start_dev, int n_desc, int total_blocks, void* stream);

/* BiFPN fusion weights on the device (main_model.py:194-196): out[j][i] = ELU(w[i][j]) / (sum_i ELU(w[i][j]) + eps), w [n][2]
 * (n = 2: w1, n = 3: w2); out / dout are TRANSPOSED [2][n] so that the n weights of fusion node j are contiguous (wgt_dev of
 * mtbt_bifpn_fuse).  The backward of that normalisation: dw [n][2] (+)= J^T dout. */
int mtbt_bifpn_norm_weights(const float* w, int n, float eps, float* out, void* stream);
int mtbt_bifpn_norm_weights_backward(const float* w, int n, float eps, const float* dout, float* dw, int accumulate, void* stream);

/* One input of a BiFPN fusion node y = sum_i w_i * resample_i(x_i) (main_model.py:211-240), backward:
 *   dx (+)= wgt * resample^T(dy);   *dwgt (+)= <dy, resample(x_in)>
 * dy [N,H,W,C]; x_in / dx [N,H,W,C] (mode 0), [N,H/2,W/2,C] (mode 1, bilinear x2) or [N,2H,2W,C] (mode 2, 2x2 mean); wgt, dwgt DEVICE
 * scalars; dx or dwgt may be NULL.  Dense NHWC in `dtype`; workspace >= mtbt_bifpn_fuse_backward_workspace_bytes(). */
int64_t mtbt_bifpn_fuse_backward_workspace_bytes(void);
int mtbt_bifpn_fuse_backward(const void* dy, const void* x_in, int mode, const float* wgt, void* dx, int accumulate_dx, float* dwgt,
                             int accumulate_dwgt, int N, int H, int W, int C, int dtype, void* workspace, int64_t workspace_bytes,
                             void* stream);

/* The oldest variant's WeightedAdd node (reference src/model.py:27-37: `w = relu(w); w = w / (w.sum() + eps); sum(w_i + f_i)`; its inputs
 * src/model.py:60-74: identity, F.interpolate(scale_factor=2, mode="nearest"), F.max_pool2d(., 2)), training side:
 *   mtbt_wadd_norm_weights            out[i] = relu(w[i]) / (sum_j relu(w[j]) + eps), n <= 8 (the forward fusion reads them through wgt_dev)
 *   mtbt_wadd_norm_weights_backward   dw[j] (+)= [w[j] > 0] * eps / (s + eps)^2 * sum(dy); dy_colsum [C] = per-channel sums of dy
 *   mtbt_resample_backward            dx (+)= resample^T(dy) for ONE input: mode 0 identity, 3 nearest x2 up (x_in / dx [N,H/2,W/2,C]),
 *                                     4 max pooling 2x2 (x_in / dx [N,2H,2W,C]; x_in = the forward input, required: dy goes to each window's
 *                                     first maximum in row-major order, as torch's max_pool2d backward does).  Dense NHWC, f32 / bf16. */
int mtbt_wadd_norm_weights(const float* w, int n, float eps, float* out, void* stream);
int mtbt_wadd_norm_weights_backward(const float* w, int n, float eps, const float* dy_colsum, int C, float* dw, int accumulate, void* stream);
int mtbt_resample_backward(const void* dy, const void* x_in, int mode, void* dx, int accumulate, int N, int H, int W, int C, int dtype,
                           void* stream);

/* Backward of the trainer's proto projector + bilinear resize (running_main_v3.py:251-255): dseg [N,Hout,Wout] f32 = d loss / d (resized
 * logits); protos [N,hp,wp,nm] f32 (forward output); w [nm] the Conv2d(nm,1,1) weight.  d_protos [N,hp,wp,nm] (dprotos_dtype) (+)=;
 * dw [nm], db [1] fp32 (+)= (dw NULL to skip both). */
int64_t mtbt_projector_backward_workspace_bytes(int N, int hp, int wp, int nm);
int mtbt_projector_backward(const float* dseg, const float* protos, const float* w, void* d_protos, int dprotos_dtype, int accumulate_dprotos,
                            float* dw, float* db, int accumulate_dw, int N, int hp, int wp, int nm, int Hout, int Wout, void* workspace,
                            int64_t workspace_bytes, void* stream);

/* AdaptiveAvgPool2d(1) + Linear backward (main_model.py:333-334, :364): x [N,HW,C]; dlogits [N,nout]; w [nout][C];
 * dx (+)= (W^T dlogits) / HW broadcast over the pixels; dw [nout][C] (+)= dlogits^T pool; db [nout] (+)= sum_n dlogits (may be NULL).
 * pool_ws: [N][C] floats of scratch. */
int mtbt_gap_fc_backward(const void* x, const float* dlogits, const float* w, void* dx, int accumulate_dx, float* dw, float* db,
                         int accumulate_dw, float* pool_ws, int N, int HW, int C, int nout, int dtype, void* stream);

/* dst[n][p][c] = c < C ? src[n][p][c] : 0, c < C_pad, with dtype conversion; element strides, no alignment requirement (the fp32
 * Detect gradient maps are 66 floats wide: their 64- and nc-channel slices become dense, zero-padded operands of dgrad / wgrad). */
int mtbt_copy_strided(const void* src, int src_dtype, int64_t src_batch_stride, int32_t src_pixel_stride, void* dst, int dst_dtype,
                      int64_t dst_batch_stride, int32_t dst_pixel_stride, int N, int64_t pixels, int C, int C_pad, void* stream);

/* Parameter gradients of a weight the forward folded with a vector, from the raw GEMM weight gradient G [K][C] (fp32, dense):
 *   mode 0, rows (ConvNeXt y = x + gamma * (W h + b), timm layer scale): dW (+)= gamma[k] G;  dvec = d gamma[k] (+)= sum_c W G + bias[k] s[k];
 *           dbias[k] (+)= gamma[k] s[k], with s[k] = sum_p dy[p][k]  (bias / s / dbias may be NULL)
 *   mode 1, columns (DepthwiseConvBlock y = W (v * x), main_model.py:84-93): dW (+)= G v[c];  dvec = d v[c] (+)= sum_k G W. */
int mtbt_scale_grad(int mode, const float* G, const float* W, const float* vec, const float* bias, const float* s, float* dW, float* dvec,
                    float* dbias, int K, int C, int accumulate, void* stream);

/* dst += src over [N][pixels][C] views (element strides, multiples of 8): gradient accumulation where the producer cannot. */
int mtbt_add_nhwc(void* dst, int64_t dst_batch_stride, int32_t dst_pixel_stride, const void* src, int64_t src_batch_stride,
                  int32_t src_pixel_stride, int N, int64_t pixels, int C, int dtype, void* stream);

/* Weight gradient of the ConvNeXt stem conv (4x4, stride 4, 3 -> K) on the caller's NCHW fp32 image: dw [K][48] (torch's [K,3,4,4])
 * (+)= sum_p d[p][k] * patch(p); d dense [N*(H/4)*(W/4)][K] in `dtype`. */
int64_t mtbt_stem_wgrad_workspace_bytes(int K);
int mtbt_stem_wgrad(const float* x, const void* d, float* dw, int N, int H, int W, int K, int dtype, int accumulate, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* dtype / layout helpers on the boundary */
int mtbt_cast(const void* src, void* dst, int64_t n, int src_dtype, int dst_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MTBT_HIP_H */
