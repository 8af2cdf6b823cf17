// Body of dwconv_kernel / dwconv_mult_kernel (dwconv.inc), included as text inside both.  The enclosing kernel provides the template
// parameters, the arguments of dwconv_kernel, and: cg = first channel of this workgroup's chunk of the OUTPUT (and of the weights and the
// epilogue vectors), C = their pixel pitch; cgx / Cx = the same for the INPUT.  The plain form has them equal; the depth-multiplier form reads
// input chunk (chunk mod Cx / 128) of a narrower tensor.  Text, not a __device__ function: the plain kernels compile exactly as before.
  const int Cn = C - cg;
  const T* __restrict__ x = x_ + cgx;
  const T* __restrict__ w = w_ + cg;
  T* __restrict__ y = y_ + cg;
  T* __restrict__ raw = raw_ ? raw_ + cg : nullptr;
  const T* res = res_ ? res_ + cg : nullptr;
  const float* __restrict__ bias = bias_ ? bias_ + cg : nullptr;
  const float* __restrict__ lnw = lnw_ ? lnw_ + cg : nullptr;
  const float* __restrict__ lnb = lnb_ ? lnb_ + cg : nullptr;
  const float* __restrict__ scale = scale_ ? scale_ + cg : nullptr;
  const float* __restrict__ shift = shift_ ? shift_ + cg : nullptr;
  constexpr int PAD = KS / 2, YB = 2, SPAN = XB + KS - 1, ROWS = YB + KS - 1;
  constexpr int IH = TH + KS - 1, IW = TW + KS - 1;
  constexpr int ES = (int)sizeof(T), PIXB = CC * ES;  // bytes per staged pixel
  constexpr int NW = (TH / 2) * (TW / XB);            // waves
  // staging geometry: one LDS-DMA wave-instruction = 1 KiB = PXI whole pixels of ONE halo row
  constexpr int PARTS = PIXB / 16, PXI = 64 / PARTS, IWP = ((IW + PXI - 1) / PXI) * PXI, SEGS = IWP / PXI;
  constexpr int NDMA = IH * SEGS, DPW = (NDMA + NW - 1) / NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* tile = smem;                                  // [IH][IWP][CC] T
  constexpr int TILEB = IH * IWP * PIXB;
  // LayerNorm scratch: its own region when C <= 128 (the next tile's DMA is already landing in `tile` during the
  // epilogue); with several chunks it reuses the tile (LDS would otherwise not fit two workgroups per CU)
  constexpr int NTI_ = (KS * KS + (64 / (PIXB / 16)) - 1) / (64 / (PIXB / 16));
  // single chunk: the scratch sits behind the tile (and behind the taps when those live in LDS): the next tile's DMA lands during the epilogue
  constexpr int REDOFF = MAXCH == 1 ? TILEB + (REGT ? 0 : NTI_ * 1024) : 0;
  // several chunks: the chunk's KS*KS taps ride along with the halo tile ([tap][CC] T right behind it, PXI taps per
  // DMA wave-instruction) -- read row by row from L2 instead, each filter row waited ~1 us for its taps
  constexpr int NTI = (KS * KS + PXI - 1) / PXI;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const int total = N * tiles_y * tiles_x;
  const int sy = wave / (TW / XB), sx = wave % (TW / XB);  // sub-tile of this wave
  const int nchunks = (Cn + CC - 1) / CC;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  const unsigned rowbytes = (unsigned)(W * Cx * ES);
  const unsigned vlane = (unsigned)((lane / PARTS) * Cx * ES + (lane % PARTS) * 16);  // lane's piece inside a DMA segment

  // tile walk: workgroups b, b+8, ... share an XCD; each XCD owns a contiguous range of tiles
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per_xcd = (total + 7) >> 3, step = gridDim.x >> 3;
  const int t_end = min(total, (xcd + 1) * per_xcd);

  // Taps (fp32 pairs of this lane's channel pair).  One chunk (C <= 128): all KS*KS stay in registers across the tiles.
  // More chunks: registers are needed for the accumulators of every chunk, so the taps are fetched row by row (KS at a
  // time, straight from L2) inside the unrolled row loop -- only two filter rows are live at once.
  constexpr bool REGTAPS = REGT;        // all KS*KS taps in registers (single-chunk default); else they ride with the halo DMA into LDS
  f32x2 wr[REGTAPS ? KS * KS : 1];
  if (REGT && lane * 2 < Cn) {
#pragma unroll
    for (int t = 0; t < KS * KS; ++t) wr[REGTAPS ? t : 0] = Pair<T>::ld(w + (unsigned)(t * C + lane * 2));
  }

  // per-channel epilogue vectors of this lane's channel pairs: loaded once (a load inside the epilogue would expose a
  // full memory round trip per tile)
  f32x2 e0[MAXCH], e1[MAXCH], e2[MAXCH];  // LN: bias, ln weight, ln bias ; else: scale, shift, -
#pragma unroll
  for (int k = 0; k < MAXCH; ++k) {
    const int c0 = k * CC + lane * 2;
    e0[k] = e1[k] = e2[k] = f32x2{0.f, 0.f};
    if (c0 < Cn) {
      if constexpr (LN) {
        e0[k] = *reinterpret_cast<const f32x2*>(bias + c0);
        e1[k] = *reinterpret_cast<const f32x2*>(lnw + c0);
        e2[k] = *reinterpret_cast<const f32x2*>(lnb + c0);
      } else {
        e0[k] = *reinterpret_cast<const f32x2*>(scale + c0);
        e1[k] = *reinterpret_cast<const f32x2*>(shift + c0);
      }
    }
  }

  // Halo tile global -> LDS by LDS-DMA (conv_dma.h), addresses on the SCALAR
  // unit: one buffer descriptor per halo row (base = that image row, num_records = its bytes); rows above / below the
  // image use an empty descriptor and columns outside it an out-of-range offset: both land as zeros.  Per instruction
  // the vector unit only adds one scalar to the lane's constant piece offset and tests its column.  Every wave issues its
  // DPW pieces back to back; the caller waits once (s_waitcnt vmcnt(0) + barrier).
  auto stage = [&](int tl_, int cb, bool with_taps) {
    const int tx_ = tl_ % tiles_x, ty_ = (tl_ / tiles_x) % tiles_y, n_ = tl_ / (tiles_x * tiles_y);
    const char* xn = reinterpret_cast<const char*>(x + (long)n_ * H * W * Cx);
#pragma unroll
    for (int d = 0; d < DPW; ++d) {
      const int j = d * NW + wave_u;
      if (NDMA % NW != 0 && j >= NDMA) break;
      const int row = j / SEGS, seg = j - row * SEGS;
      const int iy = ty_ * TH + row - PAD;
      const bool rowok = (unsigned)iy < (unsigned)H;
      srd_t srd = make_srd(xn + (long)(rowok ? iy : 0) * rowbytes);
      // (the row's bytes from THIS chunk's first channel on: `x` is shifted by cgx, and a descriptor of the whole row's length would reach
      // cgx channels past the row -- past the tensor on its last row, where a last chunk narrower than 128 channels reads them)
      srd.z = __builtin_amdgcn_readfirstlane(rowok ? rowbytes - (unsigned)(cgx * ES) : 0u);
      srd.w = __builtin_amdgcn_readfirstlane(srd.w);
      const int ix0 = tx_ * TW - PAD + seg * PXI;                // first pixel of this segment (may be < 0)
      const unsigned vo = (unsigned)(ix0 + lane / PARTS) < (unsigned)W ? vlane + (unsigned)((ix0 * Cx + cb) * ES) : 0x80000000u;
      if (!(dbg & 2)) lds_dma16(srd, vo, 0, __builtin_amdgcn_readfirstlane(lds0 + (row * IWP + seg * PXI) * PIXB));
    }
    if (!REGT && with_taps) {
      srd_t wsrd = make_srd(w);
      wsrd.z = __builtin_amdgcn_readfirstlane((unsigned)(KS * KS * C * ES));   // taps past the last read as zeros
#pragma unroll
      for (int d = 0; d < (NTI + NW - 1) / NW; ++d) {
        const int j = d * NW + wave_u;
        if (NTI % NW != 0 && j >= NTI) break;
        lds_dma16(wsrd, vlane + (unsigned)(cb * ES), j * PXI * C * ES, __builtin_amdgcn_readfirstlane(lds0 + TILEB + j * 1024));
      }
    }
  };
  bool first = true;

  for (int tl = xcd * per_xcd + slot; tl < t_end; tl += step) {
    const int tx = tl % tiles_x, ty = (tl / tiles_x) % tiles_y, n = tl / (tiles_x * tiles_y);
    const int ty0 = ty * TH, tx0 = tx * TW;

    f32x2 acc[MAXCH][YB][XB];
#pragma unroll
    for (int k = 0; k < MAXCH; ++k)
#pragma unroll
      for (int a = 0; a < YB; ++a)
#pragma unroll
        for (int i = 0; i < XB; ++i) acc[k][a][i] = f32x2{0.f, 0.f};

    auto chunk = [&](int k) {
      const int cb = k * CC;                       // chunk base channel
      const int cc = min(CC, Cn - cb);              // channels in this chunk (multiple of 8)
      const bool active = lane * 2 < cc;
      if (MAXCH > 1 || first) {                    // (one chunk: every later tile was requested during the previous epilogue)
        // Restaging barrier = lds_barrier(), NOT a plain __syncthreads(): the DMA below lands through the vector-memory path,
        // which is not ordered with the LDS queue, so every wave's ds_reads of the previous chunk must have RETURNED
        // (lgkmcnt(0)) before any wave restages.  A workgroup-scope __syncthreads() does not wait for outstanding LDS
        // reads, and the compiler may park the FMAs that consume them behind the barrier: the tail of an in-flight read --
        // lanes 48..63, the last 16-lane pass -- then picks up bytes of the NEXT chunk.  That is the failure the removed
        // two / three-chunk kernel showed next to MFMA kernels (LDS port contention widens the window); see DESIGN.md 4.
        lds_barrier();
        stage(tl, cb, MAXCH > 1 || first);   // (single chunk: the taps never change, staged once)
      }
      wait_vm<0>();
      __syncthreads();
      if (active && !(dbg & 1)) {
        const char* lp = tile + ((sy * YB) * IWP + sx * XB) * PIXB + lane * 2 * ES;
        const T* wb = w + cb;
        const unsigned lane2 = (unsigned)lane * 2;
        // Fully unrolled (tap registers need compile-time indices) and software-pipelined by hand: row r+1's inputs (LDS)
        // and, with several chunks, filter row r+1's taps (L2) are requested before row r's FMAs; a scheduling barrier
        // per row keeps the compiler from hoisting ALL rows' loads to the top (which spills).  One input row (SPAN
        // pairs) feeds YB output rows.
        f32x2 wrow[3][KS], in[2][SPAN];
        auto taps = [&](int ky) {
          // scalar base + one shared lane offset.  The empty asm makes the row's base opaque HERE: otherwise the addresses
          // of all 49 x chunks taps are loop-invariant, get hoisted out of the tile loop and spill.
#pragma unroll
          for (int kx = 0; kx < KS; ++kx) wrow[ky % 3][kx] = Pair<T>::ld(smem + TILEB + (ky * KS + kx) * PIXB + lane2 * ES);
        };
        auto inputs = [&](int r) {
#pragma unroll
          for (int j = 0; j < SPAN; ++j) in[r & 1][j] = Pair<T>::ld(lp + (r * IWP + j) * PIXB);
        };
        if (!REGTAPS) taps(0);
        inputs(0);
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
          if (!REGTAPS && r + 1 < KS) taps(r + 1);
          if (r + 1 < ROWS) inputs(r + 1);
#pragma unroll
          for (int a = 0; a < YB; ++a) {
            const int ky = r - a;
            if (ky >= 0 && ky < KS) {
#pragma unroll
              for (int kx = 0; kx < KS; ++kx) {
                const f32x2 wv = REGTAPS ? wr[REGTAPS ? ky * KS + kx : 0] : wrow[ky % 3][kx];
#pragma unroll
                for (int i = 0; i < XB; ++i) acc[k][a][i] = fma2(in[r & 1][i + kx], wv, acc[k][a][i]);
              }
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    };
#pragma clang loop unroll(full)
    for (int k = 0; k < MAXCH; ++k)
      if (k < nchunks) chunk(k);     // (uniform; a `break` would keep the loop rolled and acc[k] in scratch)
    first = false;
    const int oy0 = ty0 + sy * YB, ox0 = tx0 + sx * XB;
    T* yt = y + (((long)n * H + oy0) * W + ox0) * C;     // wave-uniform base; per-lane offsets below stay 32-bit
    const unsigned rowel = (unsigned)(W * C);
    if (dbg & 4) { if (acc[0][0][0].x == 123.f) st_elem<T>(y, 0.f); if (MAXCH == 1) { __syncthreads(); if (tl + step < t_end) stage(tl + step, 0, false); } continue; }
    if (MAXCH == 1) {   // one chunk: request the next tile now, it lands while this tile's epilogue runs
      lds_barrier();    // every wave's reads of the staged tile have returned (see the restaging barrier in chunk())
      if (tl + step < t_end) stage(tl + step, 0, false);
    }
    if constexpr (LN) {
      // + bias, per-pixel statistics over all C channels (held by this wave), normalise, store
      if (MAXCH > 1) lds_barrier();    // every wave is done with the staged tile: its LDS is reused for the reductions
      float* red = reinterpret_cast<float*>(smem + REDOFF) + wave * (16 * 64 + 16);
      float s[16];  // wave_sum16 reduces 16 values; sub-tiles with fewer pixels leave the rest zero
#pragma unroll
      for (int pq = 0; pq < 16; ++pq) s[pq] = 0.f;
#pragma unroll
      for (int k = 0; k < MAXCH; ++k) {
        const int c0 = k * CC + lane * 2;
        if (k < nchunks && c0 < Cn) {
          const f32x2 bv = e0[k];
#pragma unroll
          for (int a = 0; a < YB; ++a)
#pragma unroll
            for (int i = 0; i < XB; ++i) {
              acc[k][a][i] += bv;
              s[a * XB + i] += acc[k][a][i].x + acc[k][a][i].y;
            }
        }
      }
      if (raw) {   // training forward: keep the LayerNorm input (conv + bias) for the LayerNorm backward
        T* rt = raw + (((long)n * H + oy0) * W + ox0) * C;
#pragma unroll
        for (int k = 0; k < MAXCH; ++k) {
          const int c0 = k * CC + lane * 2;
          if (k < nchunks && c0 < Cn) {
#pragma unroll
            for (int a = 0; a < YB; ++a) {
              if (!FULL && oy0 + a >= H) continue;
#pragma unroll
              for (int i = 0; i < XB; ++i) {
                if (!FULL && ox0 + i >= W) continue;
                Pair<T>::st(rt + (a * rowel + (unsigned)(i * C + c0)), acc[k][a][i]);
              }
            }
          }
        }
      }
      wave_sum16(s, red, lane);
      const float invC = 1.0f / C;
      float q[16];
#pragma unroll
      for (int pq = 0; pq < 16; ++pq) { s[pq] *= invC; q[pq] = 0.f; }
#pragma unroll
      for (int k = 0; k < MAXCH; ++k) {
        if (k < nchunks && k * CC + lane * 2 < Cn) {
#pragma unroll
          for (int a = 0; a < YB; ++a)
#pragma unroll
            for (int i = 0; i < XB; ++i) {
              const f32x2 d = acc[k][a][i] - s[a * XB + i];
              acc[k][a][i] = d;                       // keep the centred value: the normalisation below reuses it
              q[a * XB + i] += d.x * d.x + d.y * d.y;
            }
        }
      }
      wave_sum16(q, red, lane);
#pragma unroll
      for (int pq = 0; pq < YB * XB; ++pq) q[pq] = rsqrtf(q[pq] * invC + eps);
#pragma unroll
      for (int k = 0; k < MAXCH; ++k) {
        const int c0 = k * CC + lane * 2;
        if (k < nchunks && c0 < Cn) {
          const f32x2 gw = e1[k], gb = e2[k];
#pragma unroll
          for (int a = 0; a < YB; ++a) {
            if (!FULL && oy0 + a >= H) continue;
#pragma unroll
            for (int i = 0; i < XB; ++i) {
              if (!FULL && ox0 + i >= W) continue;
              Pair<T>::st(yt + (a * rowel + (unsigned)(i * C + c0)), fma2(acc[k][a][i] * q[a * XB + i], gw, gb));
            }
          }
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < MAXCH; ++k) {
        const int c0 = k * CC + lane * 2;
        if (k < nchunks && c0 < Cn) {
          const f32x2 sc = e0[k], sh = e1[k];
          // the residual (the depthwise input gradient accumulating into a buffer that already holds the other branch's gradient: it may BE y)
          // is read for ALL of the lane's outputs before the first store.  One load next to each store made every output wait for its own round
          // trip -- the possible aliasing keeps the compiler from moving a load above the previous store: 16 dependent latencies per tile, the
          // depthwise input gradient of stage 0 ran 325 us where the forward kernel, LayerNorm included, takes 221 (round 3).
          typename Pair<T>::raw_t rv[YB][XB];       // (as they lie in memory: one register per pair for the 16-bit types)
          if (res) {
#pragma unroll
            for (int a = 0; a < YB; ++a)
#pragma unroll
              for (int i = 0; i < XB; ++i) {
                rv[a][i] = Pair<T>::zero();
                if (FULL || (oy0 + a < H && ox0 + i < W))
                  rv[a][i] = Pair<T>::ld_raw(res + (((long)n * H + oy0) * W + ox0) * C + (a * rowel + (unsigned)(i * C + c0)));
              }
          }
#pragma unroll
          for (int a = 0; a < YB; ++a) {
            if (!FULL && oy0 + a >= H) continue;
#pragma unroll
            for (int i = 0; i < XB; ++i) {
              if (!FULL && ox0 + i >= W) continue;
              const f32x2 v = fma2(acc[k][a][i], sc, sh);
              f32x2 o = ACT >= 0 ? f32x2{act_apply(v.x, ACT), act_apply(v.y, ACT)} : f32x2{act_apply(v.x, act), act_apply(v.y, act)};
              if (res) o += Pair<T>::cvt(rv[a][i]);
              Pair<T>::st(yt + (a * rowel + (unsigned)(i * C + c0)), o);
            }
          }
        }
      }
    }
  }
