// Host side of mtbt_copy_paste (include/mtbt_hip.h): the checks that come before any launch, and the per-launch table the kernel takes by
// value.  Plain C++ without a HIP include, so that tests/copy_paste_check_main.cpp can compile exactly this code alone under the address and
// undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>

#include "bitplane.h"
#include "mtbt_hip.h"

namespace copy_paste {

constexpr int CHUNK = 8;          // canvases per launch: 8 * 272 = 2176 bytes of kernel arguments (_lib.COPY_PASTE_CHUNK)
constexpr int MAX_ENTRIES = 16;   // paste entries per canvas

struct Entry { int32_t row, src, dx, dy; };                           // src = donor canvas << 1 | flip
struct Canvas { int32_t row0, row1, paste0, n; Entry e[MAX_ENTRIES]; };   // the canvas's old rows, its first entry, its entry count
struct Batch { Canvas c[CHUNK]; };

inline bool overlaps(const void* a, int64_t na, const void* b, int64_t nb) {
  if (!a || !b || na <= 0 || nb <= 0) return false;
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + (uint64_t)nb && pb < pa + (uint64_t)na;
}

// MTBT_OK, MTBT_EINVAL or MTBT_EALIGN; nothing is dereferenced but the struct and the three HOST tables.
inline int check(const mtbt_copy_paste_args* a) {
  if (!a || !a->row_off || !a->paste_off) return MTBT_EINVAL;
  const mtbt_copy_paste_args& p = *a;
  if (p.B < 0 || p.M < 0 || p.P < 0 || p.B > (1 << 30) || p.S < 4 || p.S % 4 || p.S > 32768 || p.entry_stride != 8) return MTBT_EINVAL;
  if (!plane_pitch_ok(p.S, p.pitch) || (int64_t)p.M + p.P > 0x7fffffffLL) return MTBT_EINVAL;
  const int64_t N = (int64_t)p.M + p.P;
  if ((p.B > 0 && (!p.images || !p.out_images)) || (p.M > 0 && !p.planes) || (p.P > 0 && !p.entries)) return MTBT_EINVAL;
  if (N > 0 && (!p.out_planes || !p.area_before || !p.area || !p.box)) return MTBT_EINVAL;
  if (p.rows_out && !p.rows_in && N > 0) return MTBT_EINVAL;
  if (p.row_off[0] != 0 || p.paste_off[0] != 0 || p.row_off[p.B] != p.M || p.paste_off[p.B] != p.P) return MTBT_EINVAL;
  for (int i = 0; i < p.B; ++i) {
    if (p.row_off[i + 1] < p.row_off[i] || p.paste_off[i + 1] < p.paste_off[i] || p.row_off[i + 1] > p.M || p.paste_off[i + 1] > p.P) return MTBT_EINVAL;
    if (p.paste_off[i + 1] - p.paste_off[i] > MAX_ENTRIES) return MTBT_EINVAL;
  }
  for (int64_t e = 0; e < p.P; ++e) {
    const int32_t* t = p.entries + 8 * e;
    if (t[0] < 0 || t[0] >= p.M || t[1] < -p.S || t[1] > p.S || t[2] < -p.S || t[2] > p.S || (t[3] != 0 && t[3] != 1) || t[4] || t[5] || t[6] || t[7])
      return MTBT_EINVAL;
  }
  const int64_t canvas = 4LL * p.S * p.S, plane = (int64_t)p.S * p.pitch;
  const void* in[3] = {p.images, p.planes, p.rows_in};
  const int64_t in_bytes[3] = {3 * canvas * p.B, plane * p.M, 24LL * p.M};
  const void* out[7] = {p.out_images, p.out_planes, p.out_masks, p.rows_out, p.area_before, p.area, p.box};
  const int64_t out_bytes[7] = {3 * canvas * p.B, plane * N, canvas * p.B, 24 * N, 4 * N, 4 * N, 16 * N};
  for (int o = 0; o < 7; ++o)
    for (int i = 0; i < 3; ++i)
      if (overlaps(out[o], out_bytes[o], in[i], in_bytes[i])) return MTBT_EINVAL;
  auto misaligned = [](const void* q, uintptr_t n) { return (reinterpret_cast<uintptr_t>(q) & (n - 1)) != 0; };
  if (misaligned(p.images, 16) || misaligned(p.out_images, 16) || misaligned(p.out_masks, 16) || misaligned(p.planes, 8) || misaligned(p.out_planes, 8) ||
      misaligned(p.rows_in, 4) || misaligned(p.rows_out, 4) || misaligned(p.area_before, 4) || misaligned(p.area, 4) || misaligned(p.box, 4))
    return MTBT_EALIGN;
  return MTBT_OK;
}

// The table of the canvases first .. first + nb - 1 of a checked call.  `donor` walks row_off once per call: donor_of[r] is not stored,
// the canvas of a row is found by bisection.
inline void describe(const mtbt_copy_paste_args& p, int first, int nb, Batch& b) {
  for (int k = 0; k < CHUNK; ++k) {
    Canvas& c = b.c[k];
    c = Canvas{};
    if (k >= nb) continue;
    const int i = first + k;
    c.row0 = p.row_off[i]; c.row1 = p.row_off[i + 1]; c.paste0 = p.paste_off[i]; c.n = p.paste_off[i + 1] - p.paste_off[i];
    for (int e = 0; e < c.n; ++e) {
      const int32_t* t = p.entries + 8 * (int64_t)(c.paste0 + e);
      int lo = 0, hi = p.B - 1;                     // the last canvas j with row_off[j] <= row: empty canvases before it share the offset
      while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (p.row_off[mid] <= t[0]) lo = mid; else hi = mid - 1;
      }
      c.e[e] = Entry{t[0], (int32_t)((uint32_t)lo << 1 | (uint32_t)t[3]), t[1], t[2]};
    }
  }
}

}  // namespace copy_paste
