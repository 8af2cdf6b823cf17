// The host half of csrc/bitplane.h (the pitch rule, the shape predicates, the chunking) as a stand-alone program, compiled by a plain host
// compiler and with the address and undefined-behaviour sanitizers and run on the CPU (tests/test_cpu_bitplane.py does both).  For every
// family of entry points it prints which (H, W, pitch) of a fixed walk over the word boundaries and the size limits its condition accepts:
//   dims        surface distances, distance transform, region loss, contours, RLE: both sides within PLANE_MAX_DIM
//   components  the same and H * W < 2^31
//   area        mask_eval.hip and polygon_fill.hip: H * W < 2^31 and no PLANE_MAX_DIM
//   square      copy_paste_check.h's own check() of an S x S canvas (S = W; H is not used), through a call with no canvas
// Each condition is spelled from the shared predicates as its entry point spells it.  One line per accepted triple, "family H W pitch";
// the expected lines are the test's data.  Then the chunking and the helpers at their edges: "bitplane_check: N cases ok", or 1.
#include <stdio.h>

#include "bitplane.h"
#include "copy_paste_check.h"

namespace {

int cases = 0, failures = 0;

void expect(const char* what, int64_t got, int64_t want) {
  ++cases;
  if (got != want) {
    ++failures;
    printf("bitplane_check: %s gave %lld, expected %lld\n", what, (long long)got, (long long)want);
  }
}

bool square_ok(int S, int pitch) {
  int32_t zero = 0;
  mtbt_copy_paste_args a{};
  a.S = S; a.pitch = pitch; a.entry_stride = 8; a.row_off = &zero; a.paste_off = &zero;
  return copy_paste::check(&a) == MTBT_OK;
}

}  // namespace

int main() {
  const int Ws[] = {1, 63, 64, 65, 127, 128, 129, 16384, 16385}, Hs[] = {1, 16384, 16385};
  const int pitches[] = {0, 8, 16, 24, 2048, 2056, 2064, 8192, 8200};
  struct HW { int H, W; };
  HW walk[3 * 9 + 2];
  int n = 0;
  for (int H : Hs)
    for (int W : Ws) walk[n++] = HW{H, W};
  walk[n++] = HW{32768, 65535};   // H * W = 2^31 - 32768
  walk[n++] = HW{32768, 65536};   // H * W = 2^31
  for (int i = 0; i < n; ++i)
    for (int pitch : pitches) {
      const int H = walk[i].H, W = walk[i].W;
      if (plane_dims_ok(H, W) && plane_pitch_ok(W, pitch)) printf("dims %d %d %d\n", H, W, pitch);
      if (plane_dims_ok(H, W) && plane_area_ok(H, W) && plane_pitch_ok(W, pitch)) printf("components %d %d %d\n", H, W, pitch);
      if (plane_area_ok(H, W) && plane_pitch_ok(W, pitch)) printf("area %d %d %d\n", H, W, pitch);
      if (H == 1 && square_ok(W, pitch)) printf("square %d %d %d\n", H, W, pitch);
    }

  expect("plane_words(0)", plane_words(0), 0);
  expect("plane_pitch(2^31 - 1)", plane_pitch(0x7fffffff), 8LL << 25);
  expect("a negative pitch", plane_pitch_ok(64, -8), 0);
  expect("H = 0", plane_dims_ok(0, 64) || plane_area_ok(0, 64), 0);
  expect("W = 0", plane_dims_ok(64, 0) || plane_area_ok(64, 0), 0);
  expect("negative sides", plane_dims_ok(-1, -1) || plane_area_ok(-1, -1), 0);
  expect("the largest area", plane_area_ok(1, 0x7fffffff), 1);
  expect("up16(0)", up16(0), 0);
  expect("up16(1)", up16(1), 16);
  expect("up16(16)", up16(16), 16);
  expect("up16(2^40 + 1)", up16((1LL << 40) + 1), (1LL << 40) + 16);
  expect("chunk_of: n below the group", chunk_of(3, 1), 3);
  expect("chunk_of: the group", chunk_of(1000, 1), CHUNK);
  expect("chunk_of: what fits", chunk_of(1000, CHUNK_BYTES / 5), 5);
  expect("chunk_of: one always fits", chunk_of(1000, CHUNK_BYTES * 4), 1);
  expect("chunk_of: none of none", chunk_of(0, 1), 0);
  alignas(16) static unsigned char buf[32];
  expect("aligned_n(16)", aligned_n(buf, 16) && !aligned_n(buf + 8, 16) && aligned_n(nullptr, 16), 1);
  expect("aligned8", aligned8(buf + 8) && !aligned8(buf + 4), 1);
  expect("aligned_to<int32_t>", aligned_to(reinterpret_cast<const int32_t*>(buf + 4)) && !aligned_to(reinterpret_cast<const int32_t*>(buf + 2)), 1);
  expect("aligned_to<double>", aligned_to(reinterpret_cast<const double*>(buf + 8)) && !aligned_to(reinterpret_cast<const double*>(buf + 4)), 1);
  if (failures) return 1;
  printf("bitplane_check: %d cases ok\n", cases);
  return 0;
}
