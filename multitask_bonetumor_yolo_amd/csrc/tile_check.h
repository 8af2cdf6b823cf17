// The host's checks of a sliced-inference tile table (include/mtbt_hip.h mtbt_tile), shared by tile_merge.hip (mtbt_merge_tiles) and
// mask_tiles.hip (mtbt_vote_tile_masks).  Only the HOST copy is looked at; nothing here touches the device.
#pragma once
#include "mtbt_hip.h"

namespace tile_check {

// `first` [N+1] non-decreasing inside [0, n_tiles], T_n <= t_cap and T_n K <= MTBT_FUSE_MAX_CANDIDATES; every descriptor of every image
// sane, with `image` == n when check_image, and (height, width) those of frames[n] when frames are given, else the same for every tile of
// the image.  t_big = the largest T_n.
inline int check_table(const mtbt_tile* tiles, const int32_t* first, int N, int n_tiles, int K, int t_cap, bool check_image,
                       const mtbt_frame* frames, int& t_big) {
  t_big = 0;
  if (n_tiles < 0 || first[0] < 0) return MTBT_EINVAL;
  for (int n = 0; n < N; ++n) {
    const int t0 = first[n], t1 = first[n + 1];
    if (t1 < t0 || t1 > n_tiles) return MTBT_EINVAL;
    const int T = t1 - t0;
    if (T > t_cap || (long)T * K > MTBT_FUSE_MAX_CANDIDATES) return MTBT_EINVAL;
    if (T > t_big) t_big = T;
    for (int t = t0; t < t1; ++t) {
      const mtbt_tile& d = tiles[t];
      if (check_image && d.image != n) return MTBT_EINVAL;
      if (d.reserved != 0 || d.pox < 0 || d.poy < 0 || d.height < 1 || d.width < 1) return MTBT_EINVAL;
      if (frames ? (d.height != frames[n].height || d.width != frames[n].width) : (d.height != tiles[t0].height || d.width != tiles[t0].width))
        return MTBT_EINVAL;
      if (d.wx0 < 0 || d.wy0 < 0 || d.wx1 <= d.wx0 || d.wy1 <= d.wy0 || d.wx1 > d.width || d.wy1 > d.height) return MTBT_EINVAL;
      if (!(d.step > 0.f && d.step <= 1.f) || !(d.scale > 0.f) || !(d.fox >= 0.f) || !(d.foy >= 0.f)) return MTBT_EINVAL;
    }
  }
  return MTBT_OK;
}

}  // namespace tile_check
