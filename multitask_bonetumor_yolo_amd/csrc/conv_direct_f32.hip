// fp32 (exact-fp32 MFMA, parity mode) instantiations of the direct 3x3 convolution kernels (conv3x3_direct.inc).
#include "conv3x3_direct.inc"

int mtbt_conv3x3_direct_f32(const ConvP& p, int TC, bool row_reuse, hipStream_t s) { return dispatch_direct3x3<float>(p, TC, row_reuse, s); }
