// The coefficient rows of a voted mask, W[n,r,g,:] = (sum over row r's members c in group g of s_c * coeff_c[:]) / Ss[n,r] with
// Ss[n,r] = sum over all of row r's members of s_c, written by mask_vote.hip (groups = the sources of a fusion) and mask_tiles.hip
// (groups = the tiles of an image), and how the mask kernels read them.  Small, serial sums in the stated order, bit-exact: the tests
// compare W and Ss bit for bit.  Include only from files built with -ffp-contract=off (see frame_tile.h).
//
// `Src` says where an image's candidates live.  Candidate c = g * K + k is slot k of group g:
//   int   groups, width;            groups of this image; the size of W's third dimension (groups past `groups` get zero rows)
//   int   slot(c);                  member_slot: the row the candidate opened or joined, else < 0
//   float score(c);                 s_c
//   float coeff(g, k, ch);          channel ch of the candidate's mask coefficients (through its anchor)
#pragma once
#include "common.h"
#include "frame_tile.h"

namespace frame_tile {

constexpr int VC_NT = 256;     // threads: (group of a pass of 8, channel)
constexpr int VC_ROWS = 8;     // rows per workgroup

// One workgroup per (VC_ROWS rows, image n).  The image's membership and candidate scores are staged in LDS once; per row, wave 0 adds
// the members' scores in candidate order (a ballot finds them, the additions are serial), then thread (g, ch) adds s_c * coeff_c[ch] over
// group g's members in slot order and divides once.
template <class Src>
__device__ __forceinline__ void vote_coeff_rows(const Src& src, int n, int K, int top_k, const int* counts, float* W, float* Ss) {
  __shared__ int s_slot[MTBT_FUSE_MAX_CANDIDATES];
  __shared__ float s_s[MTBT_FUSE_MAX_CANDIDATES];
  __shared__ float s_ss;
  const int tid = threadIdx.x, lane = tid & 63;
  const int C = src.groups * K;
  const int cnt = max(min(counts[n], top_k), 0);
  for (int c = tid; c < C; c += VC_NT) {
    const int slot = src.slot(c);
    s_slot[c] = slot;
    s_s[c] = slot >= 0 ? src.score(c) : 0.f;
  }
  __syncthreads();
  const int ch = tid & 31;
  for (int r = blockIdx.x * VC_ROWS; r < min((int)(blockIdx.x + 1) * VC_ROWS, top_k); ++r) {
    const bool live = r < cnt;
    if (tid < 64) {
      float ss = 0.f;
      if (live)
        for (int c0 = 0; c0 < C; c0 += 64) {
          unsigned long long mem = __ballot(c0 + lane < C && s_slot[min(c0 + lane, C - 1)] == r);
          while (mem) {   // wave-uniform: every lane adds the same members in ascending c
            const int j = __ffsll((long long)mem) - 1;
            mem &= mem - 1;
            ss = __fadd_rn(ss, s_s[c0 + j]);
          }
        }
      if (tid == 0) { s_ss = ss; Ss[(long)n * top_k + r] = ss; }
    }
    __syncthreads();
    for (int g = tid >> 5; g < src.width; g += VC_NT / 32) {
      float acc = 0.f;
      bool any = false;
      if (live && g < src.groups)
        for (int k = 0; k < K; ++k)
          if (s_slot[g * K + k] == r) {
            acc = __fadd_rn(acc, __fmul_rn(s_s[g * K + k], src.coeff(g, k, ch)));
            any = true;
          }
      W[(((long)n * top_k + r) * src.width + g) * NM + ch] = any ? __fdiv_rn(acc, s_ss) : 0.f;
    }
    __syncthreads();   // s_ss is rewritten for the next row
  }
}

// coef[16][32] <- W[n, g0 .. g0 + 15, g, :] (zero rows past cnt).  The barrier publishes coef; false when all of it is zero, i.e. group g
// has no member in any of the 16 rows (workgroup-uniform)
__device__ __forceinline__ bool stage_vote_coef(float* coef, const float* W, int n, int K, int width, int g, int g0, int cnt) {
  bool nz = false;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = threadIdx.x + u * 256, b = i >> 5, c = i & 31;
    const float v = g0 + b < cnt ? W[(((long)n * K + g0 + b) * width + g) * NM + c] : 0.f;
    coef[b * PPITCH + c] = v;
    nz = nz || v != 0.f;
  }
  return __syncthreads_or(nz);
}

}  // namespace frame_tile
