// The bit-packed mask plane, once: its layout, the word helpers of the kernels that read it and the checks of the entry points that take it.
//
// A plane is H rows of pitch = 8 * ceil(W / 64) bytes: 64 pixels per 8-byte word, pixel X is bit X & 7 of byte X >> 3 (bit X & 63 of word
// X >> 6), planes are 8-byte aligned and every access to one is an 8-byte load or store.  Bits X >= W of a row's last word are padding:
// they are masked off where a row word is read (valid_bits) and never count.
//
// The host half is plain C++ without a HIP include: copy_paste_check.h and tests/bitplane_check_main.cpp compile it alone, under the
// address and undefined-behaviour sanitizers.  The device half (and common.h) is there for the HIP compiler only.
#pragma once
#include <stdint.h>

#ifdef __HIP__
#include "common.h"
#define PLANE_HD __host__ __device__
#else
#define PLANE_HD
#endif

typedef unsigned long long u64;

// ---- layout ----------------------------------------------------------------------------------------------------------------------------
PLANE_HD inline int64_t plane_words(int64_t W) { return (W + 63) / 64; }   // 8-byte words of a row
PLANE_HD inline int64_t plane_pitch(int64_t W) { return 8 * plane_words(W); }   // bytes of a row

// ---- host: what an entry point checks before it launches ------------------------------------------------------------------------------
constexpr int PLANE_MAX_DIM = 16384;   // of the operators that keep a row or column index in 16 bits or a squared distance in 32

inline bool plane_pitch_ok(int W, int pitch) { return (int64_t)pitch == plane_pitch(W); }
inline bool plane_dims_ok(int H, int W) { return H >= 1 && H <= PLANE_MAX_DIM && W >= 1 && W <= PLANE_MAX_DIM; }
inline bool plane_area_ok(int H, int W) { return H >= 1 && W >= 1 && (int64_t)H * W < (1LL << 31); }   // a flat pixel index fits an int

inline bool aligned_n(const void* ptr, uintptr_t n) { return (reinterpret_cast<uintptr_t>(ptr) & (n - 1)) == 0; }   // n a power of two; null passes
inline bool aligned8(const void* ptr) { return aligned_n(ptr, 8); }
template <typename T> bool aligned_to(const T* ptr) { return (reinterpret_cast<uintptr_t>(ptr) % sizeof(T)) == 0; }
inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// Planes (or pairs of them) per launch group: at most CHUNK, the grid's z ...
constexpr int CHUNK = 64;
// ... and, where the workspace holds one group only (`bytes_per_plane` of it each), as many as fit CHUNK_BYTES: at least one, at most n
constexpr int64_t CHUNK_BYTES = 1LL << 30;
inline int chunk_of(int n, int64_t bytes_per_plane) {
  int64_t c = CHUNK_BYTES / bytes_per_plane;
  c = c < 1 ? 1 : (c > CHUNK ? CHUNK : c);
  return (int)(c < n ? c : n);
}

// ---- device: the bits of a row word that are pixels ------------------------------------------------------------------------------------
#ifdef __HIP__
__device__ __forceinline__ u64 low_bits(int k) { return k <= 0 ? 0ull : (k >= 64 ? ~0ull : (1ull << k) - 1ull); }   // bits 0 .. k - 1
// The same on a `long`, for polygon_fill.hip alone: its clip rectangle is the caller's data, and min(clip x1, W) - X0 with clip x1 down to
// INT_MIN and X0 up to 2^31 - 64 (H = 1) does not fit an int.
__device__ __forceinline__ u64 low_bits(long k) { return k <= 0 ? 0ull : (k >= 64 ? ~0ull : (1ull << k) - 1ull); }
// valid_bits(w, W) == low_bits(W - 64 * w).  Written out, with its comparisons in the order its kernels were compiled with: through
// low_bits the selects come out in the other order and the kernels of four files change.
__device__ __forceinline__ u64 valid_bits(int w, int W) {   // the bits X < W of row word w
  const int nv = W - w * 64;
  return nv >= 64 ? ~0ull : (nv <= 0 ? 0ull : (1ull << nv) - 1ull);
}
#endif
