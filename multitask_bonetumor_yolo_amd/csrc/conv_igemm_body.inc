// Body of conv_igemm_kernel / conv_igemm_batch_kernel (conv_igemm.inc), included as text inside both: the enclosing kernel provides the template
// parameters, `p` (const ConvP) and `bid`, the workgroup's index inside ITS convolution (blockIdx.x for a single call and for a batch member).
// Text, not a __device__ function: the single-call kernel compiles exactly as before the batched form existed.
  constexpr int EPC = 16 / (int)sizeof(T);   // elements per 16-byte chunk
  constexpr int CPR = BKB / 16;              // chunks per LDS row
  constexpr int BKE = BKB / (int)sizeof(T);  // reduction elements per step
  constexpr int WC = TC / WAVES_C, WP = TP / WAVES_P;
  constexpr int FC = WC / 16, FP = WP / 16;
  constexpr int TCS = ((TC * CPR + 255) / 256) * 256 / CPR;  // staged weight rows, padded so every wave issues the same DMA count
  constexpr int WCH = TCS * CPR / 256, XCH = TP * CPR / 256;
  static_assert(WCH * 256 == TCS * CPR && XCH * 256 == TP * CPR, "whole wave-instructions");
  constexpr int KSUB = BKB / 64;             // 16-B chunk groups (of 4) per row
  constexpr int BUF = (TCS + TP) * BKB;
  constexpr int G = WCH + XCH;               // LDS-DMA instructions per stage per wave
  constexpr int D = NBUF - 1;                // stages in flight ahead of the one being computed
  static_assert(WAVES_C * WAVES_P == 4, "4 waves");
  static_assert(WC % 16 == 0 && WP % 16 == 0, "wave tile");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int EPI = 2 * 4 * 16 * ((TC / WAVES_C) * 4 + 16);      // two slab regions per wave (conv_epilogue.h, DB)
  constexpr int AFF_OFF = (NBUF * BUF > EPI) ? NBUF * BUF : EPI;   // scale/shift copy: past the tiles AND the epilogue slabs
  float* aff = reinterpret_cast<float*>(smem + AFF_OFF);

  const int tid = threadIdx.x;
  // XCD-aware tile order: workgroups b and b+8 share an XCD (and its L2).  Each XCD gets a CONTIGUOUS range
  // of pixel tiles (neighbouring tiles share their 3x3 halo rows in that L2) and, inside it, the channel
  // tiles of one pixel tile on consecutive slots (they re-read the same input).  Pure speed: any placement
  // gives the same result.  The grid is padded to 8 * ceil(ptiles/8) pixel tiles.
  const int slot = bid >> 3, xcd = bid & 7;
  const int ctile = slot % p.ctiles;
  const int ptile = xcd * p.ptiles_per_xcd + slot / p.ctiles;
  if ((long)ptile * TP >= p.M) return;
  const int cbase = ctile * TC;
  const int pbase = ptile * TP;
  const int HoWo = p.Ho * p.Wo;
  const int Kdim = p.R * p.S * p.C;
  stage_affine<TC>(p, aff, cbase, tid);  // visible to every wave after the K loop's barriers

  // ---- staging descriptors (fixed over the whole reduction) ----
  // Operand tiles go global -> LDS by LDS-DMA through raw BUFFER descriptors (buffer_load_dwordx4 ... lds): no
  // VGPR round trip, no ds_write, and the address arithmetic leaves the vector ALU:
  //   address = SRD base (scalar, per workgroup) + soffset (scalar, the (r,s,c) step of the reduction)
  //           + voffset (per lane, CONSTANT over the loop: the lane's pixel / weight row and 16-byte slot).
  // im2col padding: a lane whose tap falls outside the image gets voffset = 0x80000000, beyond the
  // descriptor's 2 GiB range -- the hardware range check then writes ZEROS to LDS (probed on gfx950:
  // tools/probes/buffer_lds_oob.hip).  Tap validity is a per-lane bit mask built once.
  // One wave-instruction writes 64 x 16 B = 1 KiB of LDS LINEARLY (lane l -> base + 16 l), so chunk
  // c = i*256 + wave*64 + lane lands at LDS offset 16 c = (row c/CPR, slot c%CPR); the bank swizzle is applied
  // on the SOURCE side: that slot is fed with global chunk q = slot ^ swz(row), and fragment reads use the
  // same involution.
  constexpr unsigned OOB = 0x80000000u;
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_first = pbase / HoWo;                                    // first image this tile touches
  const long padoff = ((long)p.pad * p.W + p.pad) * p.ldx;             // keeps every valid voffset >= 0
  // The descriptors are four plain scalar words and the DMA is issued from inline asm (lds_dma16 below):
  // hipcc then does not track it, so it cannot force vmcnt(0) in front of the fragment reads and the
  // counted-vmcnt pipeline below really keeps D tiles in flight.  (An __amdgpu_buffer_rsrc_t builtin in this
  // template also makes the HOST pass silently drop the kernel's launch stub.)
  const srd_t xsrd = make_srd(reinterpret_cast<const T*>(p.x) + ((long)n_first * p.xbs - padoff));
  const srd_t wsrd = make_srd(reinterpret_cast<const T*>(p.w) + (long)cbase * Kdim);
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;  // LDS byte address of smem
  unsigned xvoff[XCH], xmask[XCH];
  // 1 x 1 / stride 1 / no padding over a dense batch (most launches of the network): the input row of output pixel `pix` IS row `pix` -- no
  // divisions, no tap mask (the general set-up below is ~400 instructions per thread in front of the first DMA of every tile)
  const bool flat = p.R * p.S == 1 && p.stride == 1 && p.pad == 0 && p.xbs == (long)HoWo * p.ldx;
#pragma unroll
  for (int i = 0; i < XCH; ++i) {
    const int c = tid + i * 256;
    const int row = c / CPR, q = (c % CPR) ^ swz<CPR>(row);
    const int pix = pbase + row;
    const bool ok = pix < p.M;
    if (flat) {
      xmask[i] = ok ? 1u : 0u;
      xvoff[i] = ok ? (unsigned)(((long)(pix - n_first * HoWo) * p.ldx + q * EPC) * (long)sizeof(T)) : OOB;
      continue;
    }
    const int pp = ok ? pix : pbase;
    const int n = pp / HoWo;
    const int rem = pp - n * HoWo;
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    const int iy0 = oy * p.stride - p.pad, ix0 = ox * p.stride - p.pad;
    xvoff[i] = (unsigned)(((long)(n - n_first) * p.xbs + ((long)iy0 * p.W + ix0) * p.ldx + padoff + q * EPC) * (long)sizeof(T));
    unsigned m = 0;
    for (int r = 0; r < p.R; ++r)
      for (int s2 = 0; s2 < p.S; ++s2)
        if ((unsigned)(iy0 + r) < (unsigned)p.H && (unsigned)(ix0 + s2) < (unsigned)p.W) m |= 1u << (r * p.S + s2);
    xmask[i] = ok ? m : 0u;
    if (p.R * p.S == 1 && !(m & 1u && ok)) xvoff[i] = OOB;  // 1x1: validity is folded into the offset, no per-step test
  }
  // PERM (conv_epilogue.h): inside each wave's block of WC weight rows the STAGED order is permuted (LDS row r <- weight row epi_row_channel(r)), so
  // that a lane's accumulators of a fragment pair are 8 consecutive output channels and the epilogue stores 16-byte pieces straight from them
  constexpr bool PERM = (FC % 2 == 0);
  unsigned wvoff[WCH];
#pragma unroll
  for (int i = 0; i < WCH; ++i) {
    const int c = tid + i * 256;
    const int row = c / CPR, q = (c % CPR) ^ swz<CPR>(row);
    const int srow = PERM ? (row / WC) * WC + epi_row_channel(row % WC) : row;       // the weight row this LDS row holds
    const bool ok = (row < TC) && (cbase + srow < p.K);
    wvoff[i] = ok ? (unsigned)(((long)srow * Kdim + q * EPC) * (long)sizeof(T)) : OOB;
  }

  // ---- wave / lane geometry ----
  const int wave = tid >> 6, lane = tid & 63;
  const int wc = wave / WAVES_P, wp = wave % WAVES_P;
  const int lr = lane & 15, lq = lane >> 4;
  // fragment addresses = one base per 64-byte K sub-step (+ compile-time fragment / buffer offsets, which the
  // ds_read immediate field absorbs): rows 16 apart share the swizzle, so only ks changes the XOR term
  int abase[KSUB], bbase[KSUB];
#pragma unroll
  for (int ks = 0; ks < KSUB; ++ks) {
    const int arow = wc * WC + lr, brow = wp * WP + lr;
    abase[ks] = arow * BKB + (((ks * 4 + lq) ^ swz<CPR>(arow)) << 4);
    bbase[ks] = TCS * BKB + brow * BKB + (((ks * 4 + lq) ^ swz<CPR>(brow)) << 4);
  }

  f32x4 acc[FC][FP];
#pragma unroll
  for (int i = 0; i < FC; ++i)
#pragma unroll
    for (int j = 0; j < FP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // reduction walk state (wave-uniform, lives in SGPRs)
  int kr = 0, ks_ = 0, kc = 0;  // filter row, filter col, channel offset of the step being LOADED
  int kw = 0;                   // linear k offset (elements) of that step in KRSC order
  const int nsteps = Kdim / BKE;

  const bool single_tap = (p.R * p.S == 1);
  auto stage_tile = [&](int bufidx) {
    const int tap = kr * p.S + ks_;
    const int xsoff = (int)((((long)kr * p.W + ks_) * p.ldx + kc) * (long)sizeof(T));
    const int wsoff = kw * (int)sizeof(T);
    const unsigned base = lds0 + bufidx * BUF + wave_u * 1024;
#pragma unroll
    for (int i = 0; i < XCH; ++i) {
      const unsigned vo = (single_tap || ((xmask[i] >> tap) & 1u)) ? xvoff[i] : OOB;
      lds_dma16(xsrd, vo, xsoff, base + TCS * BKB + i * 4096);
    }
#pragma unroll
    for (int i = 0; i < WCH; ++i) lds_dma16(wsrd, wvoff[i], wsoff, base + i * 4096);
    kw += BKE;
    kc += BKE;
    if (kc == p.C) { kc = 0; if (++ks_ == p.S) { ks_ = 0; ++kr; } }
  };

  // Software pipeline over NBUF LDS stages: D = NBUF-1 tiles are in flight ahead of the one being
  // multiplied.  Per step: counted vmcnt (this wave's pieces of tile t have landed; later tiles stay in
  // flight) -> raw s_barrier (everyone's pieces landed, everyone finished reading tile t-1) -> issue the DMA
  // of tile t+D into the buffer tile t-1 used -> fragment reads + MFMAs of tile t.
#pragma unroll
  for (int d = 0; d < D; ++d)
    if (d < nsteps) stage_tile(d);

  for (int t0 = 0; t0 < nsteps; t0 += NBUF) {
#pragma unroll
    for (int u = 0; u < NBUF; ++u) {  // unrolled: buffer offsets become ds_read immediates
      const int t = t0 + u;
      if (t >= nsteps) break;
      wait_stages<G, D - 1>(nsteps - 1 - t);
      lds_barrier();
      if (t + D < nsteps && !MTBT_ABL(p, 1)) stage_tile((u + D) % NBUF);
      if (MTBT_ABL(p, 2)) continue;
      const char* cur = smem + u * BUF;
#pragma unroll
      for (int ks = 0; ks < KSUB; ++ks) {
        uint4 a[FC], b[FP];
#pragma unroll
        for (int f = 0; f < FC; ++f) a[f] = MTBT_ABL(p, 8) ? uint4{1u, 2u, 3u, (unsigned)f} : *reinterpret_cast<const uint4*>(cur + abase[ks] + f * 16 * BKB);
#pragma unroll
        for (int f = 0; f < FP; ++f) b[f] = MTBT_ABL(p, 8) ? uint4{1u, 2u, 3u, (unsigned)f} : *reinterpret_cast<const uint4*>(cur + bbase[ks] + f * 16 * BKB);
        if (MTBT_ABL(p, 4)) {  // ablation: fragment reads without MFMAs (keep the reads alive)
#pragma unroll
          for (int f = 0; f < FC; ++f) { const unsigned z = a[f].x ^ a[f].y ^ a[f].z ^ a[f].w; asm volatile("" ::"v"(z)); }
#pragma unroll
          for (int f = 0; f < FP; ++f) { const unsigned z = b[f].x ^ b[f].y ^ b[f].z ^ b[f].w; asm volatile("" ::"v"(z)); }
          continue;
        }
#pragma unroll
        for (int i = 0; i < FC; ++i)
#pragma unroll
          for (int j = 0; j < FP; ++j) {
            if constexpr (sizeof(T) == 2) {
              acc[i][j] = mfma_16x16x32<T>(a[i], b[j], acc[i][j]);
            } else {
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[i].x), __uint_as_float(b[j].x), acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[i].y), __uint_as_float(b[j].y), acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[i].z), __uint_as_float(b[j].z), acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[i].w), __uint_as_float(b[j].w), acc[i][j], 0, 0, 0);
            }
          }
      }
    }
  }
  __syncthreads();  // all tiles consumed: the staging buffers are free for the epilogue
  if (MTBT_ABL(p, 16)) return;

  // ---- epilogue (conv_epilogue.h): slabs of 16 pixels x WC channels per wave ----
  const int Cq = p.K >> 2;  // ConvT: channels per (dy,dx) quadrant
  const EpiSeq seq{(long)pbase + wp * WP, 16, (long)p.M, 0, 0};   // linear outputs: pixel index = GEMM row
  conv_epilogue<T, TC, FC, FP, true, 1, (sizeof(T) == 2), PERM>(p, acc, smem + wave * (2 * 16 * (WC * 4 + 16)), aff, cbase, wc * WC, lane,
                               [&](int j, int row, int ch, long& yoff, long& roff) -> bool {
    const int pix = pbase + wp * WP + j * 16 + row;
    if (pix >= p.M) return false;
    if (p.y_linear) {
      yoff = (long)pix * p.ldy + ch;
      roff = (long)pix * p.ldr + ch;
    } else if (p.out_mode == MTBT_OUT_CONVT2X2) {
      const int n = pix / HoWo, rem = pix - n * HoWo;
      const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
      const int quad = ch / Cq, chout = ch - quad * Cq;
      const long opix = (long)(2 * oy + (quad >> 1)) * (2 * p.Wo) + (2 * ox + (quad & 1));
      yoff = (long)n * p.ybs + opix * p.ldy + chout;
      roff = (long)n * p.rbs + opix * p.ldr + chout;
    } else {
      const int n = pix / HoWo, rem = pix - n * HoWo;
      yoff = (long)n * p.ybs + (long)rem * p.ldy + ch;
      roff = (long)n * p.rbs + (long)rem * p.ldr + ch;
    }
    return true;
  }, seq, p.y_linear != 0, (long)ptile * WAVES_P + wp);   // column-sum partial rows: WAVES_P per pixel tile
