// The exact fraction comparisons of mtbt_measure_regions (THE MEASURE RULE in include/mtbt_hip.h): which hull edge gives the smaller caliper
// width h^2 / len2, which the smaller rectangle h t / len2.  h is a cross product of two lattice vectors (< 2^30 at H, W <= 16384), h^2 is
// below 2^60, t < 2^31, len2 < 2^30: the cross-multiplied sides reach 2^90 and do not fit 64 bits, and a double does not hold them either.
// So they are formed in two 64-bit words, from 32-bit halves: no __int128, nothing the device compiler has to lower specially.
//
// Plain C++ without a HIP include: measure.hip compiles it for host and device, tests/measure_exact_main.cpp compiles it alone with the
// host compiler, under the undefined-behaviour sanitizer, and compares it with Python integers.
#pragma once
#include <stdint.h>

#ifdef __HIP__
#define MX_HD __host__ __device__
#else
#define MX_HD
#endif

struct mx_u128 { uint64_t hi, lo; };

// a * b, all 128 bits (schoolbook on 32-bit halves; every partial sum below fits 64 bits)
MX_HD inline mx_u128 mx_mul(uint64_t a, uint64_t b) {
  const uint64_t a0 = a & 0xFFFFFFFFull, a1 = a >> 32, b0 = b & 0xFFFFFFFFull, b1 = b >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (p01 & 0xFFFFFFFFull) + (p10 & 0xFFFFFFFFull);   // < 3 * 2^32
  mx_u128 r;
  r.lo = (p00 & 0xFFFFFFFFull) | (mid << 32);
  r.hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
  return r;
}

// -1, 0, 1 as x is below, equal to, above y
MX_HD inline int mx_cmp(mx_u128 x, mx_u128 y) {
  if (x.hi != y.hi) return x.hi < y.hi ? -1 : 1;
  if (x.lo != y.lo) return x.lo < y.lo ? -1 : 1;
  return 0;
}

// the sign of n1 / d1 - n2 / d2 for d1, d2 > 0: n1 d2 against n2 d1
MX_HD inline int mx_cmp_frac(uint64_t n1, uint64_t d1, uint64_t n2, uint64_t d2) { return mx_cmp(mx_mul(n1, d2), mx_mul(n2, d1)); }

// the sign of h1^2 / len1 - h2^2 / len2: the caliper widths of two edges (h < 2^32, so h * h fits)
MX_HD inline int mx_cmp_width(uint64_t h1, uint64_t len1, uint64_t h2, uint64_t len2) { return mx_cmp_frac(h1 * h1, len1, h2 * h2, len2); }

// the sign of h1 t1 / len1 - h2 t2 / len2: the areas of the rectangles on two edges (h t < 2^64 at h < 2^30, t < 2^31)
MX_HD inline int mx_cmp_rect(uint64_t h1, uint64_t t1, uint64_t len1, uint64_t h2, uint64_t t2, uint64_t len2) {
  return mx_cmp_frac(h1 * t1, len1, h2 * t2, len2);
}
