// Instance masks and boxes in the ORIGINAL image frame, masks one bit per pixel (mtbt_masks_to_frames).
//
//   low[k][y][x] = sum_c coeff[k][c] * protos[y][x][c]                   -- MFMA, exact fp32 (v_mfma_f32_16x16x4_f32), as mask_mfma.hip
//   bit(k, Y, X) = bilinear(low[k])(X, Y) > 0  (&& inside the frame box when cropping)
//
// The bilinear taps are taken at the ORIGINAL pixel positions in one step (torch's align_corners=False rule with
// step = scale / up prototype pixels per frame pixel): no letterboxed S x S plane exists in between.  All coordinate
// and box arithmetic is separate fp32 multiplies and adds (this file is compiled with -ffp-contract=off) so that it
// rounds like the CPU restatement in tests/frame_reference.py.
//
// A workgroup owns one tile of one image: 2^wl 64-pixel words wide and th rows tall, both picked per image on the host
// from `step` so that the prototype patch under the tile (first tap of the first pixel .. second tap of the last) fits
// the LDS patch buffer.  Tiles are whole words wide and every word of a plane belongs to exactly one tile, so no two
// workgroups write the same byte and every byte of every plane is written: no pre-zero pass, no atomics.
//   1. the patch is staged in LDS once (lazily: with cropping only when a box group touches the tile);
//   2. boxes are processed 16 at a time: coefficients [16 x 32] x patch [32 x NPX] on the fp32 MFMA -> low in LDS;
//   3. the tile is cut into (row, word) units; a wave takes a run of up to 64 consecutive units.  A lane owns pixel
//      64 * word + lane of the row, evaluates the four taps for each of the 16 boxes and the wave's ballot is the row's
//      8-byte word.  The ballot of the wave's unit j is kept by lane j, and one store per box writes the whole run
//      (consecutive words of a row are consecutive in memory).
// With cropping a (unit, box) pair whose word lies wholly outside the box costs nothing but the zero it stores, and a
// group of 16 boxes that all miss the tile skips the MFMA phase too.  Planes k >= counts[n] are zero-filled here.
#include "common.h"
#include "frame_tile.h"

namespace {

using namespace frame_tile;   // the LDS geometry, FrameD, frame_tap / frame_box and the host's tile choice, shared with mask_vote.hip

struct FrameP {
  const float* protos;
  const float* coeff;
  long cbs, cks, ccs;
  const int* gather;
  const int* counts;
  const float* boxes;
  float* boxes_frame;
  unsigned char* out;
  int n_frames, K, hp, wp;
  FrameD f[MAX_FRAMES];
};

template <bool CROP>
__global__ __launch_bounds__(256) void frame_mask_kernel(const FrameP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* patch = reinterpret_cast<float*>(smem);       // [NPX_CAP][PPITCH]
  float* coef = patch + NPX_CAP * PPITCH;              // [16][PPITCH]
  float* low = coef + 16 * PPITCH;                     // [16][LPITCH]
  float* boxs = low + 16 * LPITCH;                     // [16][4] frame boxes of the group
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  int n = 0;
  for (int i = 1; i < p.n_frames; ++i)
    if ((int)blockIdx.x >= p.f[i].blk0) n = i;
  const FrameD& f = p.f[n];
  const int H0 = f.H0, W0 = f.W0, wl = f.wl, wt = 1 << wl;
  const float step = f.step;
  const int t = (int)blockIdx.x - f.blk0;
  const int ty = t / f.tiles_x, tx = t - ty * f.tiles_x;
  const int X0 = tx * 64 * wt, Y0 = ty * f.th;
  const int Xl = min(X0 + 64 * wt, W0) - 1, Yl = min(Y0 + f.th, H0) - 1;   // last pixel of the tile
  const int words_x = f.pitch >> 3;
  const int nwx = min(wt, words_x - tx * wt), nrows = Yl - Y0 + 1;
  const int cnt = p.counts ? max(min(p.counts[n], p.K), 0) : p.K;

  // boxes in the frame: written once per image, by its first tile
  if (t == 0 && p.boxes_frame) {
    for (int i = tid; i < p.K * 4; i += 256) {
      const long at = (long)n * p.K * 4 + i;
      p.boxes_frame[at] = (i >> 2) < cnt ? frame_box(p.boxes[at], f.scale, i & 3, H0, W0) : 0.f;
    }
  }

  // prototype patch under the tile
  int pxa, pxb, pya, pyb, tmp;
  float ftmp;
  frame_tap(X0, step, p.wp, pxa, tmp, ftmp);
  frame_tap(Xl, step, p.wp, tmp, pxb, ftmp);
  frame_tap(Y0, step, p.hp, pya, tmp, ftmp);
  frame_tap(Yl, step, p.hp, tmp, pyb, ftmp);
  const int PW = pxb - pxa + 1, PH = pyb - pya + 1;
  const int NPX = PW * PH, NPXP = min((NPX + 15) & ~15, NPX_CAP);   // <= NPX_CAP by the host's choice of the tile
  const float* pr = p.protos + (long)n * p.hp * p.wp * NM;

  // units of this wave: u = row * wt + word, a run of upw consecutive ones; lane j keeps (and stores) unit u0 + j
  const int U = nrows << wl, upw = (U + 3) >> 2, u0 = wave * upw;
  const int un = max(min(upw, U - u0), 0);
  const int my_u = u0 + lane, my_row = my_u >> wl, my_word = my_u & (wt - 1);
  const bool my_store = lane < un && my_word < nwx;
  unsigned char* my_out = p.out + f.offset + (long)(Y0 + my_row) * f.pitch + (long)(tx * wt + my_word) * 8;
  const long plane = (long)H0 * f.pitch;

  float cpre[2];
  float bpre = 0.f;
  auto fetch_group = [&](int g) {   // coefficients (gather index -> coefficient: two dependent loads) and boxes, one group ahead
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = tid + u * 256, b = i >> 5, c = i & 31;
      float v = 0.f;
      if (g + b < cnt) {
        const long kk = p.gather ? p.gather[(long)n * p.K + g + b] : (g + b);
        v = p.coeff[(long)n * p.cbs + kk * p.cks + c * p.ccs];
      }
      cpre[u] = v;
    }
    if (CROP && tid < 64) {
      const int b = tid >> 2;
      bpre = g + b < cnt ? frame_box(p.boxes[((long)n * p.K + g + b) * 4 + (tid & 3)], f.scale, tid & 3, H0, W0) : 0.f;
    }
  };

  bool staged = false;
  if (cnt > 0) fetch_group(0);
  for (int g0 = 0; g0 < cnt; g0 += 16) {
    const int nb = min(16, cnt - g0);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = tid + u * 256;
      coef[(i >> 5) * PPITCH + (i & 31)] = cpre[u];
    }
    if (CROP && tid < 64) boxs[tid] = bpre;
    __syncthreads();
    if (g0 + 16 < cnt) fetch_group(g0 + 16);
    bool ghit = true;   // workgroup-uniform: does any box of the group touch the tile
    if (CROP) {
      ghit = false;
      for (int b = 0; b < nb; ++b) {
        const float x1 = boxs[b * 4], y1 = boxs[b * 4 + 1], x2 = boxs[b * 4 + 2], y2 = boxs[b * 4 + 3];
        ghit = ghit || (x1 <= (float)Xl && (float)X0 < x2 && y1 <= (float)Yl && (float)Y0 < y2);
      }
    }
    if (ghit) {
      if (!staged) {
        for (int i = tid; i < NPXP * (NM / 4); i += 256) {
          const int px = i >> 3, c4 = i & 7;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (px < NPX) {
            const int py = px / PW, pxx = px - py * PW;
            v = *reinterpret_cast<const float4*>(pr + ((long)(pya + py) * p.wp + (pxa + pxx)) * NM + c4 * 4);
          }
          float* d = patch + px * PPITCH + c4 * 4;
          d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        staged = true;
        __syncthreads();
      }
      // low[16][NPXP] = coef[16][32] x patch^T on the fp32 MFMA; wave w takes column groups w, w+4, ...
      float a[8];
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) a[ks] = coef[(lane & 15) * PPITCH + ks * 4 + (lane >> 4)];
      for (int pg = wave; pg < NPXP / 16; pg += 4) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* bp = patch + (pg * 16 + (lane & 15)) * PPITCH + (lane >> 4);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ks], bp[ks * 4], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) low[(4 * (lane >> 4) + r) * LPITCH + pg * 16 + (lane & 15)] = acc[r];
      }
      __syncthreads();
    }
    // sampling: one ballot per (unit, box)
    unsigned long long word[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) word[b] = 0ull;
    if (ghit) {
      for (int j = 0; j < un; ++j) {
        const int u = u0 + j, row = u >> wl, wd = u & (wt - 1);
        if (wd >= nwx) continue;
        const int Y = Y0 + row, Xw = X0 + wd * 64, X = Xw + lane;
        const bool valid = X < W0;
        int x0, x1, y0, y1;
        float lx, ly;
        frame_tap(min(X, W0 - 1), step, p.wp, x0, x1, lx);
        frame_tap(Y, step, p.hp, y0, y1, ly);
        const float wx0 = 1.f - lx, wy0 = 1.f - ly;
        const int i00 = (y0 - pya) * PW + (x0 - pxa), i01 = (y0 - pya) * PW + (x1 - pxa);
        const int i10 = (y1 - pya) * PW + (x0 - pxa), i11 = (y1 - pya) * PW + (x1 - pxa);
        const float fX = (float)X, fY = (float)Y, fXw = (float)Xw, fXe = (float)min(Xw + 63, W0 - 1);
#pragma unroll
        for (int b = 0; b < 16; ++b) {
          // hit is wave-uniform.  Without cropping all 16 boxes are sampled (a slot past nb has zero coefficients: v = 0, no bit), so the
          // 64 tap reads of a unit are independent and issue together
          bool in = valid, hit = !CROP || b < nb;
          if (CROP) {
            const float bx1 = boxs[b * 4], by1 = boxs[b * 4 + 1], bx2 = boxs[b * 4 + 2], by2 = boxs[b * 4 + 3];
            hit = hit && bx1 <= fXe && fXw < bx2 && by1 <= fY && fY < by2;   // else the word is wholly outside the box: it stays zero
            in = in && bx1 <= fX && fX < bx2;
          }
          if (hit) {
            const float* l = low + b * LPITCH;
            const float v = wy0 * (wx0 * l[i00] + lx * l[i01]) + ly * (wx0 * l[i10] + lx * l[i11]);
            const unsigned long long m = __ballot(in && v > 0.f);
            if (lane == j) word[b] = m;
          }
        }
      }
    }
    if (my_store) {
#pragma unroll
      for (int b = 0; b < 16; ++b)
        if (b < nb) *reinterpret_cast<unsigned long long*>(my_out + (long)(g0 + b) * plane) = word[b];
    }
    __syncthreads();   // coef / low / boxs are rewritten by the next group
  }
  // planes k >= cnt: zeros
  if (my_store)
    for (int k = cnt; k < p.K; ++k) *reinterpret_cast<unsigned long long*>(my_out + (long)k * plane) = 0ull;
}

}  // namespace

extern "C" int mtbt_sizeof_frame_args(int which) {
  switch (which) {
    case 0: return (int)sizeof(mtbt_frame);
    case 1: return (int)sizeof(mtbt_frame_mask_args);
    default: return -1;
  }
}

extern "C" int mtbt_masks_to_frames(const mtbt_frame_mask_args* a, const mtbt_frame* frames, int n_frames, void* stream) {
  if (!a || !frames || !a->protos || !a->coeff || !a->out) return MTBT_EINVAL;
  if (n_frames < 1 || n_frames > MAX_FRAMES || n_frames != a->N) return MTBT_EINVAL;
  if (a->nm != NM || a->K < 1 || a->K > 65535 || a->hp < 1 || a->wp < 1 || a->out_bytes < 0) return MTBT_EINVAL;
  if ((a->crop || a->boxes_frame) && !a->boxes) return MTBT_EINVAL;
  FrameP p;
  long blocks = 0;
  if (int rc = frame_layout(frames, n_frames, a->K, a->hp, a->wp, a->boxes != nullptr, a->out_bytes, p.f, blocks)) return rc;
  if (!aligned16(a->protos) || !aligned16(a->out)) return MTBT_EALIGN;
  p.protos = a->protos; p.coeff = a->coeff;
  p.cbs = a->coeff_batch_stride; p.cks = a->coeff_k_stride; p.ccs = a->coeff_c_stride;
  p.gather = a->gather_idx; p.counts = a->counts; p.boxes = a->boxes; p.boxes_frame = a->boxes_frame; p.out = a->out;
  p.n_frames = n_frames; p.K = a->K; p.hp = a->hp; p.wp = a->wp;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (a->crop) {
    if (int rc = mtbt_allow_lds(frame_mask_kernel<true>, (int)FRAME_LDS)) return rc;
    hipLaunchKernelGGL(frame_mask_kernel<true>, dim3((unsigned)blocks), dim3(256), FRAME_LDS, s, p);
  } else {
    if (int rc = mtbt_allow_lds(frame_mask_kernel<false>, (int)FRAME_LDS)) return rc;
    hipLaunchKernelGGL(frame_mask_kernel<false>, dim3((unsigned)blocks), dim3(256), FRAME_LDS, s, p);
  }
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}
