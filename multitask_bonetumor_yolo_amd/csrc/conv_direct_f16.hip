// fp16 (v_mfma_f32_16x16x32_f16, saturating stores: BASELINE configs[4]) instantiations of the direct 3x3 convolution kernels (conv3x3_direct.inc).
#include "conv3x3_direct.inc"

int mtbt_conv3x3_direct_f16(const ConvP& p, int TC, bool row_reuse, hipStream_t s) { return dispatch_direct3x3<f16_t>(p, TC, row_reuse, s); }
