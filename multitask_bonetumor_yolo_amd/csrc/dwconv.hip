// C entry points of the depthwise convolution: validation and dispatch to the per-storage-type translation units
// (dwconv_bf16.hip, dwconv_f16.hip, dwconv_f32.hip; kernel in dwconv.inc).
#include "common.h"
#include "dwconv_args.h"

static int dw_dispatch(const DwArgs& a, int dtype, hipStream_t s) {
  if (dtype == MTBT_BF16) return mtbt_dw_run_bf16(a, s);
  if (dtype == MTBT_F16) return mtbt_dw_run_f16(a, s);
  if (dtype == MTBT_F32) return mtbt_dw_run_f32(a, s);
  return MTBT_EINVAL;
}

// the shape rules of the plain entry points, shared with mtbt_dwconv_kernel_choice
static int dw_check_shape(int N, int H, int W, int C, int ksize, int act) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || C > 768) return MTBT_EINVAL;
  if (ksize != 3 && ksize != 7) return MTBT_EINVAL;
  if (act < 0 || act > MTBT_ACT_DGELU_POLY) return MTBT_EINVAL;
  if ((long)(W + 64) * C * 4 >= 0x7fff0000L || (long)H * W * C >= 0x7fff0000L) return MTBT_EINVAL;  // 32-bit offsets in a row / an image
  return MTBT_OK;
}

static int dw_dispatch_mult(const DwArgs& a, int Cx, int dtype, hipStream_t s) {
  if (dtype == MTBT_BF16) return mtbt_dw_run_mult_bf16(a, Cx, s);
  if (dtype == MTBT_F16) return mtbt_dw_run_mult_f16(a, Cx, s);
  if (dtype == MTBT_F32) return mtbt_dw_run_mult_f32(a, Cx, s);
  return MTBT_EINVAL;
}

// the same for the depth-multiplier form
static int dw_check_shape_mult(int N, int H, int W, int C, int M, int act) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 128 || (M != 1 && M != 2) || M * C > 768) return MTBT_EINVAL;
  if (act < 0 || act > MTBT_ACT_DGELU_POLY) return MTBT_EINVAL;
  if ((long)(W + 64) * M * C * 4 >= 0x7fff0000L || (long)H * W * M * C >= 0x7fff0000L) return MTBT_EINVAL;  // 32-bit offsets in a row / an image
  return MTBT_OK;
}

// w: [k*k][C] in the activation dtype (bf16 taps in bf16 mode, like every other conv's weights).
static int dwconv_entry(const void* x, const void* w, const float* bias, const float* ln_w, const float* ln_b, float ln_eps, const float* scale,
                        const float* shift, int act, void* y, void* raw, const void* res, int N, int H, int W, int C, int ksize, int dtype,
                        void* stream) {
  if (!x || !w || !y) return MTBT_EINVAL;
  if (int rc = dw_check_shape(N, H, W, C, ksize, act)) return rc;
  const bool ln = ln_w != nullptr;
  if (ln && (!ln_b || !bias || res)) return MTBT_EINVAL;
  if (!ln && (!scale || !shift || raw)) return MTBT_EINVAL;
  if (!aligned16(x) || !aligned16(y) || !aligned16(w) || (raw && !aligned16(raw)) || (res && !aligned16(res))) return MTBT_EALIGN;
  DwArgs a{x, w, bias, ln_w, ln_b, ln_eps, scale, shift, act, y, raw, res, N, H, W, C, ksize, nullptr};
  return dw_dispatch(a, dtype, reinterpret_cast<hipStream_t>(stream));
}

// What mtbt_dwconv_nhwc(_train) would launch: the dispatch itself runs with DwArgs::choice set and returns where it would launch.  Of the
// pointers only "ln_w is set" takes part in the dispatch; the training outputs raw / res do not.
extern "C" int mtbt_dwconv_kernel_choice(int N, int H, int W, int C, int ksize, int ln, int act, int dtype, int32_t* choice) {
  if (!choice) return MTBT_EINVAL;
  if (int rc = dw_check_shape(N, H, W, C, ksize, act)) return rc;
  static const float some = 0.f;
  DwArgs a{nullptr, nullptr, nullptr, ln ? &some : nullptr, nullptr, 0.f, nullptr, nullptr, act, nullptr, nullptr, nullptr, N, H, W, C, ksize, choice};
  return dw_dispatch(a, dtype, nullptr);
}

extern "C" int mtbt_dwconv_nhwc(const void* x, const void* w, const float* bias, const float* ln_w, const float* ln_b,
                                float ln_eps, const float* scale, const float* shift, int act, void* y, int N, int H,
                                int W, int C, int ksize, int dtype, void* stream) {
  return dwconv_entry(x, w, bias, ln_w, ln_b, ln_eps, scale, shift, act, y, nullptr, nullptr, N, H, W, C, ksize, dtype, stream);
}

// Training variants: `raw` (LayerNorm form only) also receives the LayerNorm INPUT conv + bias (what the LayerNorm backward needs);
// `res` (scale / shift form only) is added after the activation and may alias y (gradient accumulation of the depthwise dgrad).
extern "C" int mtbt_dwconv_nhwc_train(const void* x, const void* w, const float* bias, const float* ln_w, const float* ln_b,
                                      float ln_eps, const float* scale, const float* shift, int act, void* y, void* raw, const void* res,
                                      int N, int H, int W, int C, int ksize, int dtype, void* stream) {
  return dwconv_entry(x, w, bias, ln_w, ln_b, ln_eps, scale, shift, act, y, raw, res, N, H, W, C, ksize, dtype, stream);
}

// Depthwise 3x3 with a depth multiplier M (header): output channel j of M * C reads input channel j mod C.  The one-chunk scale / shift
// kernel with the input chunk and pitch separated from the output's: per channel the same arithmetic as mtbt_dwconv_nhwc.
extern "C" int mtbt_dwconv3x3_mult_nhwc(const void* x, const void* w, const float* scale, const float* shift, int act, void* y, int N, int H, int W,
                                        int C, int M, int dtype, void* stream) {
  if (!x || !w || !y || !scale || !shift) return MTBT_EINVAL;
  if (int rc = dw_check_shape_mult(N, H, W, C, M, act)) return rc;
  if (!aligned16(x) || !aligned16(y) || !aligned16(w)) return MTBT_EALIGN;
  DwArgs a{x, w, nullptr, nullptr, nullptr, 0.f, scale, shift, act, y, nullptr, nullptr, N, H, W, M * C, 3, nullptr};
  return dw_dispatch_mult(a, C, dtype, reinterpret_cast<hipStream_t>(stream));
}

// What mtbt_dwconv3x3_mult_nhwc would launch (see mtbt_dwconv_kernel_choice).
extern "C" int mtbt_dwconv3x3_mult_kernel_choice(int N, int H, int W, int C, int M, int act, int dtype, int32_t* choice) {
  if (!choice) return MTBT_EINVAL;
  if (int rc = dw_check_shape_mult(N, H, W, C, M, act)) return rc;
  DwArgs a{nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, nullptr, nullptr, act, nullptr, nullptr, nullptr, N, H, W, M * C, 3, choice};
  return dw_dispatch_mult(a, C, dtype, nullptr);
}
