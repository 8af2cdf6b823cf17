// Arguments of one depthwise-convolution launch, handed from the C entry (dwconv.hip) to the per-storage-type translation units.
#pragma once
#include <hip/hip_runtime.h>

struct DwArgs {
  const void* x; const void* w; const float* bias; const float* ln_w; const float* ln_b; float ln_eps;
  const float* scale; const float* shift; int act; void* y; void* raw; const void* res;
  int N, H, W, C, ksize;
  int32_t* choice;   // non-null (mtbt_dwconv_kernel_choice): the launch function reports what it would launch, here, and launches nothing
};

int mtbt_dw_run_bf16(const DwArgs& a, hipStream_t s);
int mtbt_dw_run_f16(const DwArgs& a, hipStream_t s);
int mtbt_dw_run_f32(const DwArgs& a, hipStream_t s);
// depth-multiplier form (3x3, scale / shift): a.C = the OUTPUT channels M * Cx, Cx = the input's
int mtbt_dw_run_mult_bf16(const DwArgs& a, int Cx, hipStream_t s);
int mtbt_dw_run_mult_f16(const DwArgs& a, int Cx, hipStream_t s);
int mtbt_dw_run_mult_f32(const DwArgs& a, int Cx, hipStream_t s);
