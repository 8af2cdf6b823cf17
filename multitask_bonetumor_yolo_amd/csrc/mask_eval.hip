// Instance-mask COCO evaluation from bit-packed planes: mtbt_pack_masks, mtbt_mask_pair_counts, mtbt_mask_eval (contracts in
// include/mtbt_hip.h), feeding `metrics.DeviceMaskMeanAveragePrecision`.
//
// Packed layout everywhere (the one mask_frame.hip writes): a plane is H rows of pitch = 8 * ceil(W / 64) bytes, pixel X is bit
// X & 7 of byte X >> 3, padding bits are zero.  A plane is a run of H * pitch / 8 64-bit words and is 8-byte aligned, not more:
// every access to a plane here is one 8-byte load or store.
//
// pack_masks_kernel   a plane is cut into (row, word) units, consecutive units are consecutive in memory.  A wave takes a run of 64
//                     units: a lane owns pixel 64 * word + lane of the unit's row, the wave's ballot is the unit's word, lane j keeps
//                     the ballot of unit j and one 512-byte store writes the run.  Cropped-away pixels are not read.  Bound: the
//                     source read (1 or 4 bytes per pixel against 1 bit written).
// pair_counts_kernel  one 256-thread workgroup per (image, detection plane k).  The image's GT rows are compacted into LDS (ballot
//                     prefix, as coco_match_kernel compacts GT rows), 256 candidate rows at a time, and taken in groups of 4 with
//                     register accumulators: thread t walks words t, t + 256, ... of the detection plane and of the group's GT
//                     planes, popcount(d & g) per pair; wave reduction, LDS reduction, one plain store per (m, k).  Typical G is 1 - 3:
//                     one pass over the detection plane; a further group re-reads it from L2.  The workgroup of plane 0 also counts
//                     the GT planes' own areas.  No atomics: a workgroup owns its (b, k).  Bound: HBM on the detection planes (the
//                     GT planes of an image are shared by its K workgroups and stay in L2).
// coco_match_kernel<PlanePairs>  coco_eval.h's walk (semantics at the top of box_eval.hip) with the IoU taken from the
//                     pixel-count tables: inter / (det_area + gt_px - inter) in fp64 from exact integers, 0 for an empty union; areas
//                     are pixel counts; GT membership, order and class from gt_image / gt_label.  Latency-bound like the box walk.
#include "bitplane.h"
#include "coco_eval.h"

namespace {

constexpr int MAX_IMAGES = 32;   // images per pair-count launch (descriptors travel as kernel arguments)
constexpr int PT = 256;          // threads of the pack and pair-count workgroups
constexpr int PW = PT / 64;
constexpr int GG = 4;            // GT planes per register group

// ---------------------------------------------------------------------------------------------------------------- pack
template <typename T>
__global__ __launch_bounds__(PT) void pack_masks_kernel(const mtbt_pack_masks_args p, const int bpp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned j = blockIdx.x / (unsigned)bpp, blk = blockIdx.x - j * (unsigned)bpp;   // output plane, block of 256 units within it
  const int words_x = p.pitch >> 3;
  const int U = p.H * words_x;                      // < 2^31 / 64 + H: H * W < 2^31
  const int u0 = ((int)blk * PW + wave) * 64;
  if (u0 >= U) return;
  const int un = min(64, U - u0);
  const int src = p.plane_of ? p.plane_of[j] : (int)j;
  float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
  if (p.boxes) {
    const float* bx = p.boxes + (long)j * 4;
    x1 = bx[0]; y1 = bx[1]; x2 = bx[2]; y2 = bx[3];
  }
  u64 mine = 0ull;
  if (src >= 0 && src < p.n_src) {
    const T* sp = reinterpret_cast<const T*>(p.src) + (long)src * p.plane_stride;
    int row = u0 / words_x, word = u0 - row * words_x;
    for (int i = 0; i < un; ++i) {
      const int X = word * 64 + lane;
      bool in = X < p.W;
      if (p.boxes) in = in && x1 <= (float)X && (float)X < x2 && y1 <= (float)row && (float)row < y2;
      bool bit = false;
      if (in) bit = sp[(long)row * p.row_stride + X] > (T)0;   // NaN > 0 is false
      const u64 m = __ballot(bit);
      if (lane == i) mine = m;
      if (++word == words_x) { word = 0; ++row; }
    }
  }
  if (lane < un) reinterpret_cast<u64*>(p.out)[(long)j * U + u0 + lane] = mine;
}

// ---------------------------------------------------------------------------------------------------------------- pair counts
struct PairImg {
  const u64* det;
  const u64* gt;
  int nwords;      // H * pitch / 8
  int g0, gt_planes, pad_;
};
struct PairP {
  const int* counts;
  const int* gt_image;
  unsigned* inter;
  unsigned* det_area;
  unsigned* gt_area;
  int B, K, M, pad_;
  PairImg im[MAX_IMAGES];
};

__global__ __launch_bounds__(PT) void pair_counts_kernel(const PairP p) {
  __shared__ int gidx[PT];
  __shared__ int wcnt[PW];
  __shared__ unsigned red[PW][2 * GG + 1];
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const PairImg im = p.im[b];
  int cnt = p.K;
  if (p.counts) {
    cnt = p.counts[b];
    cnt = cnt < 0 ? 0 : (cnt > p.K ? p.K : cnt);
  }
  const bool live = k < cnt;     // else the plane counts as empty and is not read
  const bool areas = k == 0;     // this workgroup also counts the image's GT planes
  if (!live && !areas) {         // its inter words stay as the entry point cleared them
    if (tid == 0) p.det_area[(long)b * p.K + k] = 0u;
    return;
  }
  const u64* dp = im.det + (long)k * im.nwords;
  bool det_done = false;

  // one walk over the detection plane against n <= GG GT rows gidx[g .. g + n); uniform over the workgroup
  auto pass = [&](int g, int n) {
    unsigned acc[GG], ga[GG], da = 0u;
    const u64* gp[GG];
#pragma unroll
    for (int j = 0; j < GG; ++j) {
      acc[j] = 0u;
      ga[j] = 0u;
      gp[j] = j < n ? im.gt + (long)(gidx[g + j] - im.g0) * im.nwords : im.gt;
    }
    for (int i = tid; i < im.nwords; i += PT) {
      const u64 d = live ? dp[i] : 0ull;
      da += (unsigned)__popcll(d);
#pragma unroll
      for (int j = 0; j < GG; ++j) {
        if (j < n) {
          const u64 w = gp[j][i];
          acc[j] += (unsigned)__popcll(w & d);
          ga[j] += (unsigned)__popcll(w);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < GG; ++j) {
      acc[j] = wave_sum_u32(acc[j]);
      ga[j] = wave_sum_u32(ga[j]);
    }
    da = wave_sum_u32(da);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < GG; ++j) {
        red[wave][j] = acc[j];
        red[wave][GG + j] = ga[j];
      }
      red[wave][2 * GG] = da;
    }
    __syncthreads();
    if (tid < 2 * GG + 1) {
      unsigned s = 0u;
#pragma unroll
      for (int w = 0; w < PW; ++w) s += red[w][tid];
      if (tid < GG) {
        if (tid < n) p.inter[(long)gidx[g + tid] * p.K + k] = s;
      } else if (tid < 2 * GG) {
        if (areas && tid - GG < n) p.gt_area[gidx[g + tid - GG]] = s;
      } else if (!det_done) {
        p.det_area[(long)b * p.K + k] = s;
      }
    }
    det_done = true;
    __syncthreads();   // red and gidx are rewritten
  };

  for (int base = 0; base < p.M; base += PT) {
    // the image's GT rows among rows base .. base + 255, compacted in row order
    const int m = base + tid;
    bool mine = false;
    if (m < p.M && p.gt_image[m] == b) {
      const int rel = m - im.g0;
      mine = rel >= 0 && rel < im.gt_planes;
    }
    const u64 bal = __ballot(mine);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int off = 0, ng = 0;
#pragma unroll
    for (int w = 0; w < PW; ++w) {
      off += w < wave ? wcnt[w] : 0;
      ng += wcnt[w];
    }
    if (mine) gidx[off + __popcll(bal & ((1ull << lane) - 1ull))] = m;
    __syncthreads();
    for (int g = 0; g < ng; g += GG) pass(g, min(GG, ng - g));
  }
  if (!det_done) pass(0, 0);        // an image without GT: the detection's area alone
}

// ---------------------------------------------------------------------------------------------------------------- matching
__device__ __forceinline__ double count_iou(unsigned inter, unsigned da, unsigned ga) {
  const double it = (double)inter, uni = ((double)da + (double)ga) - it;
  return uni > 0.0 ? it / uni : 0.0;
}

// a pair = (detection plane, GT plane) of the pixel-count tables; LDS holds the areas and the GT rows' indices into `inter`
struct PlanePairs {
  using Args = mtbt_mask_eval_args;
  struct Lds { unsigned darea[CAP], garea[CAP]; int gidx[CAP]; };
  const Args& p;
  Lds& s;
  __device__ bool gt_in_batch(long g, double& area) const {
    const int gi = p.gt_image[g];
    if (!(gi >= 0 && gi < p.B)) return false;
    area = (double)p.gt_px[g];
    return true;
  }
  __device__ void load_det(int i, long at) { s.darea[i] = p.det_area[at]; }
  __device__ bool gt_of(int g, int b) const { return p.gt_image[g] == b; }
  __device__ double load_gt(int g, int pos, int& cls) {
    const unsigned px = p.gt_px[g];
    s.gidx[pos] = g;
    s.garea[pos] = px;
    cls = p.gt_label[g];
    return (double)px;
  }
  __device__ double iou(int i, int j) const { return count_iou(p.inter[(long)s.gidx[j] * p.K + i], s.darea[i], s.garea[j]); }
  __device__ double det_area(int i) const { return (double)s.darea[i]; }
};

bool plane_shape_ok(int H, int W, int pitch) { return plane_area_ok(H, W) && plane_pitch_ok(W, pitch); }

}  // namespace

extern "C" int mtbt_sizeof_mask_eval_args(int which) {
  switch (which) {
    case 0: return (int)sizeof(mtbt_pack_masks_args);
    case 1: return (int)sizeof(mtbt_mask_image);
    case 2: return (int)sizeof(mtbt_mask_pair_args);
    case 3: return (int)sizeof(mtbt_mask_eval_args);
    default: return -1;
  }
}

extern "C" int mtbt_pack_masks(const mtbt_pack_masks_args* a, void* stream) {
  if (!a || !a->out) return MTBT_EINVAL;
  const mtbt_pack_masks_args& p = *a;
  if (p.n_src < 0 || p.n_out < 0 || (p.n_src > 0 && !p.src) || !plane_shape_ok(p.H, p.W, p.pitch)) return MTBT_EINVAL;
  if (p.row_stride < p.W || p.plane_stride < 0 || (p.dtype != 0 && p.dtype != 1)) return MTBT_EINVAL;
  if (!p.plane_of && p.n_out > p.n_src) return MTBT_EINVAL;
  if (!aligned8(p.out) || !aligned_to(p.boxes) || !aligned_to(p.plane_of)) return MTBT_EALIGN;
  if (p.dtype == 1 && !aligned_to(reinterpret_cast<const float*>(p.src))) return MTBT_EALIGN;
  if (p.n_out == 0) return MTBT_OK;
  const int64_t U = (int64_t)p.H * (p.pitch >> 3);
  const int64_t bpp = (U + PT - 1) / PT, blocks = bpp * p.n_out;
  if (blocks > 0x7fffffffLL) return MTBT_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (p.dtype == 0)
    hipLaunchKernelGGL(pack_masks_kernel<unsigned char>, dim3((unsigned)blocks), dim3(PT), 0, s, p, (int)bpp);
  else
    hipLaunchKernelGGL(pack_masks_kernel<float>, dim3((unsigned)blocks), dim3(PT), 0, s, p, (int)bpp);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}

extern "C" int mtbt_mask_pair_counts(const mtbt_mask_pair_args* a, const mtbt_mask_image* images, int n_images, void* stream) {
  if (!a || !images || !a->det_area) return MTBT_EINVAL;
  if (a->K < 1 || a->K > CAP || n_images < 1 || n_images > MAX_IMAGES || n_images != a->B || a->M < 0) return MTBT_EINVAL;
  if (a->M > 0 && (!a->inter || !a->gt_image || !a->gt_area)) return MTBT_EINVAL;
  PairP p;
  for (int i = 0; i < n_images; ++i) {
    const mtbt_mask_image& im = images[i];
    if (!im.det || !im.gt_base || !plane_shape_ok(im.H, im.W, im.pitch) || im.gt_planes < 0) return MTBT_EINVAL;
    if (!aligned8(im.det) || !aligned8(im.gt_base)) return MTBT_EALIGN;
    PairImg& d = p.im[i];
    d.det = reinterpret_cast<const u64*>(im.det);
    d.gt = reinterpret_cast<const u64*>(im.gt_base);
    d.nwords = (int)(((int64_t)im.H * im.pitch) >> 3);
    d.g0 = im.g0; d.gt_planes = im.gt_planes; d.pad_ = 0;
  }
  if (!aligned_to(a->counts) || !aligned_to(a->gt_image) || !aligned_to(a->inter) || !aligned_to(a->det_area) || !aligned_to(a->gt_area))
    return MTBT_EALIGN;
  p.counts = a->counts; p.gt_image = a->gt_image; p.inter = a->inter; p.det_area = a->det_area; p.gt_area = a->gt_area;
  p.B = a->B; p.K = a->K; p.M = a->M; p.pad_ = 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (a->M > 0) {   // rows of no image, and pairs with a plane k >= counts[b], are never written by the kernel
    if (hipMemsetAsync(a->inter, 0, (size_t)a->M * a->K * sizeof(uint32_t), s) != hipSuccess) return MTBT_ELAUNCH;
    if (hipMemsetAsync(a->gt_area, 0, (size_t)a->M * sizeof(uint32_t), s) != hipSuccess) return MTBT_ELAUNCH;
  }
  hipLaunchKernelGGL(pair_counts_kernel, dim3((unsigned)a->K, (unsigned)n_images), dim3(PT), 0, s, p);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}

extern "C" int mtbt_mask_eval(const mtbt_mask_eval_args* args, void* stream) {
  if (!args) return MTBT_EINVAL;
  const mtbt_mask_eval_args& p = *args;
  if (p.T < 1 || p.T > 32 || p.K < 1 || p.K > CAP || p.B < 0 || p.M < 0 || p.max_det < 1) return MTBT_EINVAL;
  if (!p.det_area || !p.scores || !p.labels || !p.rank || !p.match || !p.ignore || !p.status) return MTBT_EINVAL;
  if (p.M > 0 && (!p.inter || !p.gt_px || !p.gt_image || !p.gt_label || !p.gt_area)) return MTBT_EINVAL;
  if (!aligned_to(p.inter) || !aligned_to(p.det_area) || !aligned_to(p.gt_px) || !aligned_to(p.scores) || !aligned_to(p.labels) ||
      !aligned_to(p.counts) || !aligned_to(p.gt_image) || !aligned_to(p.gt_label) || !aligned_to(p.rank) || !aligned_to(p.match) ||
      !aligned_to(p.ignore) || !aligned_to(p.gt_area) || !aligned_to(p.status))
    return MTBT_EALIGN;
  if (p.B == 0) return MTBT_OK;
  hipLaunchKernelGGL(coco_match_kernel<PlanePairs>, dim3((unsigned)p.B, NA), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), p);
  MTBT_LAUNCH_CHECK();
  return MTBT_OK;
}
