// Body of conv3x3_rr_kernel / conv3x3_rr_batch_kernel (conv3x3_direct.inc), included as text inside both: the enclosing kernel provides T, TC,
// `p` (const ConvP) and `bid`, the workgroup's index inside its convolution.  Text, not a __device__ function: the single-call kernel
// compiles exactly as before the batched form existed.
  constexpr int ES = (int)sizeof(T), EPC = 16 / ES, BKB = 64, BKE = BKB / ES;
  constexpr int HWID = 18, NHP = HWID * HWID;
  constexpr int FC = TC / 32, FP = 8, WCH = TC / 2;
  constexpr int XDMA = (NHP * 4 + 255) / 256;                  // halo DMA instructions per wave (6)
  constexpr int XBYTES = XDMA * 256 * 16;
  constexpr int WTAP = TC * BKB, WGRP = 3 * WTAP;              // one tap tile / one filter column
  constexpr int WDMA = WGRP / 16 / 256;
  constexpr unsigned OOB = 0x80000000u;
  static_assert(TC % 64 == 0 && WDMA * 256 * 16 == WGRP, "weight column = whole wave-instructions");
  static_assert(FC % 2 == 0, "fragment pairs (PERM epilogue)");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* aff = reinterpret_cast<float*>(smem + XBYTES + 2 * WGRP);
  static_assert(2 * 4 * 16 * (WCH * 4 + 16) <= XBYTES + 2 * WGRP, "epilogue slabs (two regions per wave) below the affine copy");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = wave & 1, wr = wave >> 1;
  const int lr = lane & 15, lq = lane >> 4;

  const int slot = bid >> 3, xcd = bid & 7;
  const int ctile = slot % p.ctiles;
  const int ptile = xcd * p.ptiles_per_xcd + slot / p.ctiles;
  const int tiles_x = p.W >> 4, tpi = tiles_x * (p.H >> 4);
  if (ptile >= p.N * tpi) return;
  const int n = ptile / tpi, trem = ptile - n * tpi;
  const int ty0 = (trem / tiles_x) << 4, tx0 = (trem % tiles_x) << 4;
  const int cbase = ctile * TC;
  const int Kdim = 9 * p.C;
  stage_affine<TC>(p, aff, cbase, tid);

  const srd_t xsrd = make_srd(reinterpret_cast<const T*>(p.x) + (long)n * p.xbs);
  const srd_t wsrd = make_srd(reinterpret_cast<const T*>(p.w) + (long)cbase * Kdim);
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;

  unsigned xvoff[XDMA];
#pragma unroll
  for (int i = 0; i < XDMA; ++i) {
    const int c = i * 256 + tid;
    const int hp = c >> 2, sl = c & 3;
    const int hy = hp / HWID, hx = hp - hy * HWID;
    const int iy = ty0 - 1 + hy, ix = tx0 - 1 + hx;
    const bool ok = hp < NHP && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
    xvoff[i] = ok ? (unsigned)((((long)iy * p.W + ix) * p.ldx + (sl ^ ((hp >> 2) & 3)) * EPC) * ES) : OOB;
  }
  unsigned wvoff[WDMA];   // piece c of a column: tap row r = c / (TC*4), weight row, 16-byte slot
#pragma unroll
  for (int i = 0; i < WDMA; ++i) {
    const int c = i * 256 + tid;
    const int r = c / (TC * 4), rem = c - r * (TC * 4);
    const int row = rem >> 2, sl = rem & 3;
    const int srow = (row / WCH) * WCH + epi_row_channel(row % WCH);      // staged row order of conv_epilogue.h PERM, per wave block of WCH rows
    wvoff[i] = (cbase + srow < p.K) ? (unsigned)(((long)srow * Kdim + (long)r * 3 * p.C + (sl ^ ((row >> 2) & 3)) * EPC) * ES) : OOB;
  }
  const int hp0 = (8 * wr) * HWID + lr;                                            // + rr * 18 + s
  const int arow = wc * WCH + lr;                                                  // + f * 16
  const int aoff = XBYTES + arow * BKB + ((lq ^ ((arow >> 2) & 3)) << 4);          // + buf * WGRP + r * WTAP + f * 16 * BKB

  f32x4 acc[FC][FP];
#pragma unroll
  for (int i = 0; i < FC; ++i)
#pragma unroll
    for (int j = 0; j < FP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nslabs = p.C / BKE, nsteps = 3 * nslabs;
  auto stage_w = [&](int g) {   // weights of column step g (slab g / 3, filter column g % 3) -> buffer g & 1
    const int cc = g / 3, s = g - 3 * cc;
    const int wsoff = (s * p.C) * ES + cc * BKB;
#pragma unroll
    for (int i = 0; i < WDMA; ++i) lds_dma16(wsrd, wvoff[i], wsoff, lds0 + XBYTES + (g & 1) * WGRP + (i * 256 + wave * 64) * 16);
  };
  auto stage_x = [&](int cc) {
#pragma unroll
    for (int i = 0; i < XDMA; ++i) lds_dma16(xsrd, xvoff[i], cc * BKB, lds0 + (i * 256 + wave * 64) * 16);
  };
  stage_x(0);
  stage_w(0);
#pragma unroll 1
  for (int g0 = 0; g0 < nsteps; g0 += 6) {
#pragma unroll
    for (int u = 0; u < 6; ++u) {   // unrolled over (two slabs x three columns): buffer parity and s are compile-time
      const int g = g0 + u;
      if (g >= nsteps) continue;  // odd slab count: the second half of the last round is empty (uniform over the block)
      const int s = u % 3;
      wait_vm<0>();               // my pieces of this step's weights (and, at s == 0, of the slab's halo) have landed
      lds_barrier();              // everyone's have; everyone is done with the previous step's weight buffer
      if (g + 1 < nsteps && !MTBT_ABL(p, 1)) stage_w(g + 1);
      uint4 b[FP + 2];
#pragma unroll
      for (int rr = 0; rr < FP + 2; ++rr) {
        const int hp = hp0 + rr * HWID + s;
        b[rr] = MTBT_ABL(p, 8) ? uint4{1u, 2u, 3u, (unsigned)rr} : *reinterpret_cast<const uint4*>(smem + hp * BKB + ((lq ^ ((hp >> 2) & 3)) << 4));
      }
      if (s == 2 && g + 1 < nsteps && !MTBT_ABL(p, 1)) {   // the halo is free once every wave holds this column's fragments: request the next slab
        lds_barrier();
        stage_x(g / 3 + 1);
      }
      const char* wb = smem + aoff + (u & 1) * WGRP;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        uint4 a[FC];
#pragma unroll
        for (int f = 0; f < FC; ++f) a[f] = MTBT_ABL(p, 8) ? uint4{1u, 2u, 3u, (unsigned)f} : *reinterpret_cast<const uint4*>(wb + r * WTAP + f * 16 * BKB);
        if (MTBT_ABL(p, 4)) {  // ablation: fragment reads without MFMAs (keep the reads alive)
#pragma unroll
          for (int i = 0; i < FC; ++i) acc[i][0].x += __uint_as_float(a[i].x ^ b[i + r].y ^ b[i + 4 + r].z);
          continue;
        }
#pragma unroll
        for (int i = 0; i < FC; ++i)
#pragma unroll
          for (int j = 0; j < FP; ++j) {
            if constexpr (sizeof(T) == 2) {
              acc[i][j] = mfma_16x16x32<T>(a[i], b[j + r], acc[i][j]);
            } else {
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[i].x), __uint_as_float(b[j + r].x), acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[i].y), __uint_as_float(b[j + r].y), acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[i].z), __uint_as_float(b[j + r].z), acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[i].w), __uint_as_float(b[j + r].w), acc[i][j], 0, 0, 0);
            }
          }
      }
    }
  }
  __syncthreads();  // LDS is free for the epilogue slabs

  const EpiSeq seq{(long)(ty0 + 8 * wr) * p.W + tx0, p.W, 0x7fffffffffffffffL, (long)n * p.ybs, (long)n * p.rbs};
  conv_epilogue<T, TC, FC, FP, false, MTBT_RR_RESPF, (sizeof(T) == 2), true>(p, acc, smem + wave * (2 * 16 * (WCH * 4 + 16)), aff, cbase, wc * WCH, lane,
                               [&](int j, int row, int ch, long& yoff, long& roff) -> bool {
    const long pixoff = (long)(ty0 + 8 * wr + j) * p.W + tx0 + row;
    yoff = (long)n * p.ybs + pixoff * p.ldy + ch;
    roff = (long)n * p.rbs + pixoff * p.ldr + ch;
    return true;
  }, seq, true, (long)ptile * DIRECT_RR_CS_ROWS + wr);       // column-sum partial rows: 2 per tile (the wave's row half; the channel halves write disjoint columns)
