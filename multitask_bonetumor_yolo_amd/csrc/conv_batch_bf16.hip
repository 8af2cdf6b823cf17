// bf16 instantiations of the batched convolution kernels (mtbt_conv2d_nhwc_batch): only the tiles the batch chooser can return --
// implicit GEMM 64x64, 128x128, 128x64 and 32x64 with 128-byte K-steps, the row-reuse direct 3x3 at 64 channels.
#define MTBT_CONV_BATCH_UNIT
#include "conv_igemm.inc"
#include "conv3x3_direct.inc"

int mtbt_conv_batch_dispatch_bf16(const ConvBatchP& b, int n, int kind, int TC, int TP, hipStream_t s) {
  if (kind == 1) return TC == 64 ? launch_direct3x3_rr_batch<bf16_t, 64>(b, n, s) : MTBT_EINVAL;
  if (TC == 128 && TP == 128) return launch_batch<bf16_t, 128, 128, 2, 2, 128, 2>(b, n, s);
  if (TC == 128 && TP == 64) return launch_batch<bf16_t, 128, 64, 2, 2, 128, 2>(b, n, s);
  if (TC == 64 && TP == 64) return launch_batch<bf16_t, 64, 64, 1, 4, 128, 2>(b, n, s);
  if (TC == 32 && TP == 64) return launch_batch<bf16_t, 32, 64, 1, 4, 128, 2>(b, n, s);
  return MTBT_EINVAL;
}
