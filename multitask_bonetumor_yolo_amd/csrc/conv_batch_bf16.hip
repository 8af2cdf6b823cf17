// bf16 instantiations of the batched convolution kernels (mtbt_conv2d_nhwc_batch): only what the batch chooser can return --
// the implicit GEMM on the batched tiles of conv_tiles.h with 128-byte K-steps, the row-reuse direct 3x3 at 64 channels.
#define MTBT_CONV_BATCH_UNIT
#include "conv_igemm.inc"
#include "conv3x3_direct.inc"

int mtbt_conv_batch_dispatch_bf16(const ConvBatchP& b, int n, const ConvChoice& c, hipStream_t s) {
  if (c.kind == CONV_DIRECT3X3) return c.TC == 64 ? launch_direct3x3_rr<64>(conv3x3_rr_batch_kernel<bf16_t, 64>, b, n, s) : MTBT_EINVAL;
  return dispatch_tile_batch<bf16_t>(b, n, c.TC, c.TP, s);
}
