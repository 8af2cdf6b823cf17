// Depthwise convolution kernels, f16 storage (kernel in dwconv.inc).
#include "dwconv.inc"

int mtbt_dw_run_f16(const DwArgs& a, hipStream_t s) { return dw_run<f16_t, 16, true>(a, s); }
int mtbt_dw_run_mult_f16(const DwArgs& a, int Cx, hipStream_t s) { return dw_run_mult<f16_t, 16, true>(a, Cx, s); }
