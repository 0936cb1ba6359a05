// Patch-resident implicit GEMM for stride-1 convolutions (bf16), included by conv.hip inside
// its anonymous namespace.
//
// The im2col pipeline above re-fetches every input pixel once per filter tap (L2 -> LDS), and at
// 128x64 tiles the LDS-DMA fill, not the matrix pipe, sets the pace (DESIGN.md §4).  Here a
// workgroup owns TR consecutive GLOBAL output rows (row index over the whole batch, R = b*Ho + ho)
// x TC output columns and loads the input window it needs ONCE:
//
//   padded row space:  every image has Hp = Ho + KH - 1 padded input rows (PT zero rows on top);
//                      output row R = (b, ho) starts at padded row P(R) = R + b*(KH-1), and a tile
//                      of consecutive output rows needs a CONTIGUOUS range of padded rows, also
//                      across image boundaries.
//   LDS patch:         [NR padded rows][PW = TC + KW - 1 pixels][PXBp bytes]; vertical / horizontal
//                      padding is materialised as zeros (DMA lanes read the zero page).
//                      PXBp = Cin*2, plus 32 bytes when Cin*2 is a multiple of 64: the pixel stride is
//                      then an odd multiple of 32 B and the 16 pixels x 2 chunks a ds_read_b128 lane
//                      group touches fall into 16 different 16-byte bank groups, for every tap shift.
//   k order:           unchanged (kh, kw, c) flat, weights stay [Cout][Kpad].  Inside one kernel row
//                      the (kw, c) index is contiguous in the patch, so the pixel operand of k-chunk
//                      j is  base(pixel) + koff(j)  with a per-lane (c, kw) counter that adds the
//                      pixel padding / row skip when it wraps.
//
// Only the weight k-tiles stream through the LDS-DMA ring ([BN rows][128 B], same swizzle as above):
// BN*128 bytes per 64-deep k-tile instead of (BM+BN)*128.  WM x WN waves split pixels x channels; a
// wave owns TM x TN 16x16 tiles (16*TM pixels x 16*TN channels), so a k-step costs TM + TN fragment
// reads for TM*TN MFMAs, and the 8- and 12-wave variants put 2-3 waves on every SIMD of the CU that
// share ONE patch (the fill and its latency are paid once per BM x BN outputs).
//
// Results are bit-identical to conv_igemm_dma_body: same operands, same k order per accumulator.

struct PatchGeo {
  int TC, TR, ncol;      // output columns / global output rows per tile, column tiles per row
  int PW, PXBp, CPP, CPPp, cmagic;   // patch row width (pixels), padded pixel bytes, 16-B chunks per pixel (data / padded)
  int NR, Hp, rowB;      // patch rows allocated, padded rows per image, bytes per patch row
  int gapB;              // extra bytes in front of every further image of the tile (see patch_geometry)
  int lds_bytes;
};

constexpr int kPatchMaxParts = 8;   // 1-KiB DMA pieces per patch row (host: patch_geometry)

// WM x WN waves: WM splits the pixels, WN the output channels; a wave owns TM x TN 16x16 tiles.
// NSTAGE_ = kLoaderWaves + n (conv.hip): four extra waves share the patch fill and own the weight ring, the WM x WN
// waves only read fragments and issue MFMAs after their share of the fill.
template <typename HT, int TM, int TN, int WM, int WN, int NSTAGE_>
__device__ __forceinline__ void conv_patch_body(const ConvArgs& a, const int tile_m, const int block_n) {
  constexpr int NSTAGE = ring_stages(NSTAGE_);
  constexpr bool SPEC = NSTAGE_ >= kLoaderWaves;
  constexpr int NWC = WM * WN;                 // waves that own output tiles
  constexpr int NWA = NWC + (SPEC ? 4 : 0);    // all waves: they share the patch fill
  constexpr int NW = SPEC ? 4 : NWC;           // waves that issue the weight ring
  constexpr int BN = 16 * TN * WN;
  constexpr int W_STAGE = BN * 128;
  constexpr int IPW_B = BN / 8 / NW;          // weight DMA instructions per wave per k-tile
  constexpr int AHEAD = NSTAGE - 1;
  static_assert(BN % (8 * NW) == 0, "the weight rows of a k-tile must split evenly over the waves");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) unsigned char*)smem);
  constexpr uint32_t PATCH0 = NSTAGE * W_STAGE;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_id = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool loader = SPEC && wave_id >= NWC;
  const int wave = loader ? wave_id - NWC : wave_id;     // index inside its role
  const int wm = wave / WN, wn = wave % WN;
  const bf16_t* __restrict__ xg = (const bf16_t*)a.x;
  const bf16_t* __restrict__ wg = (const bf16_t*)a.w;
  const bf16_t* zp = (const bf16_t*)a.zero;
  const int bn0 = block_n * BN;

  STAMP(0);
  // ---- tile geometry (wave-uniform) ------------------------------------------------------
  const int ct = tile_m % a.p_ncol, rt = tile_m / a.p_ncol;
  const int w0 = ct * a.p_TC;
  const int TCt = min(a.p_TC, a.Wo - w0);
  const int GR = a.B * a.Ho;
  const int R0 = rt * a.p_TR;
  const int TRt = min(a.p_TR, GR - R0);
  const int b0 = R0 / a.Ho;
  const int P0 = R0 + b0 * (a.KH - 1);
  const int b_last = (R0 + TRt - 1) / a.Ho;
  const int NRt = min(a.p_NR, TRt + (b_last - b0 + 1) * (a.KH - 1));     // padded rows this tile reads
  const int npx = TRt * TCt;
  const int PXBp = a.p_PXBp, PW = a.p_PW;

  // ---- patch fill: wave w loads padded rows w, w+NW, ... ---------------------------------
  // A lane's (column, chunk) inside a row does not depend on the row: computed once per 1-KiB piece.
  {
    const int rowslots = PW * a.p_CPPp;
    const int parts = (rowslots + 63) >> 6;
    int loff[kPatchMaxParts];         // element offset of the lane's chunk from the start of the image row
    bool lok[kPatchMaxParts], lact[kPatchMaxParts];
#pragma unroll
    for (int part = 0; part < kPatchMaxParts; ++part) {
      const int slot = part * 64 + lane;
      const int col = (slot * a.p_cmagic) >> 16;
      const int ch = slot - col * a.p_CPPp;
      const int wi = w0 + col - a.PL;
      lact[part] = slot < rowslots;
      lok[part] = lact[part] & (ch < a.p_CPP) & ((unsigned)wi < (unsigned)a.W);
      loff[part] = wi * a.x_cs + ch * 8;
    }
    const float rcpHp = 1.0f / (float)a.p_Hp;
    for (int q = wave_id; q < NRt; q += NWA) {
      const int Pq = P0 + q;
      const int b = (int)(((float)Pq + 0.5f) * rcpHp);
      const int hi = Pq - b * a.p_Hp - a.PT;
      const bool rowok = (b < a.B) & ((unsigned)hi < (unsigned)a.H);
      const bf16_t* rowsrc = xg + (((b * a.H + hi) * a.W) * a.x_cs + a.x_co);
      unsigned char* dst = smem + PATCH0 + q * a.p_rowB + (b - b0) * a.p_gapB;
#pragma unroll
      for (int part = 0; part < kPatchMaxParts; ++part) {
        if (part < parts) {
          const bf16_t* src = (rowok & lok[part]) ? rowsrc + loff[part] : zp;
          if (lact[part]) dma16(src, dst + part * 1024);
        }
      }
    }
  }

  STAMP(1);
  // ---- weight k-tiles --------------------------------------------------------------------
  const int slot8 = lane & 7, rsub = lane >> 3;
  const bf16_t* wsrc[IPW_B];
  bool nok[IPW_B];
#pragma unroll
  for (int i = 0; i < IPW_B; ++i) {
    const int gb = wave * IPW_B + i;
    const int n = bn0 + gb * 8 + rsub;
    nok[i] = n < a.Cout;
    const int chunk = slot8 ^ ((4 * (gb & 1) + (rsub >> 1)) & 7);
    wsrc[i] = wg + (size_t)(nok[i] ? n : 0) * a.Kpad + chunk * 8;
  }
  const int nk = a.Kpad / 64;
  auto issue_w = [&](int kt, int stage) {
    unsigned char* sbase = smem + stage * W_STAGE;
#pragma unroll
    for (int i = 0; i < IPW_B; ++i) {
      const int gb = wave * IPW_B + i;
      const bf16_t* src = nok[i] ? wsrc[i] + (size_t)kt * 64 : zp;
      dma16(src, sbase + gb * 1024);
    }
  };
  if constexpr (SPEC) {
    if (loader) {
      // the counted waits below also cover this wave's patch pieces (issued before the ring tiles, retired in order)
#pragma unroll
      for (int p = 0; p < AHEAD; ++p)
        if (p < nk) issue_w(p, p);
      for (int kt = 0; kt < nk; ++kt) {
        const int pending = min(AHEAD - 1, nk - 1 - kt);
        if (pending >= 2)
          wait_vmcnt<2 * IPW_B>();
        else if (pending == 1)
          wait_vmcnt<IPW_B>();
        else
          wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (kt + AHEAD < nk) issue_w(kt + AHEAD, (kt + AHEAD) % NSTAGE);
      }
      return;
    }
  } else {
#pragma unroll
    for (int p = 0; p < AHEAD; ++p)
      if (p < nk) issue_w(p, p);
  }

  // ---- per-lane pixel bases ----------------------------------------------------------------
  const int fr = lane & 15, fg = lane >> 4;
  uint32_t xb[TM];
  int mrow[TM];
  {
    const float rcpTC = 1.0f / (float)TCt, rcpHo = 1.0f / (float)a.Ho;
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      const int t = (wm * TM + j) * 16 + fr;
      const bool ok = t < npx;
      const int tt = ok ? t : 0;
      const int tr = (int)(((float)tt + 0.5f) * rcpTC);
      const int tc = tt - tr * TCt;
      const int R = R0 + tr;
      const int b = (int)(((float)R + 0.5f) * rcpHo);
      const int q = tr + (b - b0) * (a.KH - 1);
      xb[j] = lds0 + PATCH0 + (uint32_t)(q * a.p_rowB + (b - b0) * a.p_gapB + tc * PXBp + fg * 16);
      mrow[j] = ok ? R * a.Wo + w0 + tc : -1;
    }
  }
  // k walk of this lane's chunk: c = channel of the chunk inside its pixel, kw = filter column
  int kc = fg * 8, kkw = 0;
  uint32_t koff = 0;
  const int padB = PXBp - a.Cin * 2;
  const int rowskipB = a.p_rowB - a.KW * PXBp;
  auto advance = [&]() {
    kc += 32;
    koff += 64;
    const bool wrap = kc >= a.Cin;
    kc = wrap ? kc - a.Cin : kc;
    koff += wrap ? padB : 0;
    kkw += wrap ? 1 : 0;
    const bool wrap2 = kkw == a.KW;
    kkw = wrap2 ? 0 : kkw;
    koff += wrap2 ? rowskipB : 0;
  };

  f32x4_t acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const uint32_t sw = (fr >> 1) & 7;
  const uint32_t w_off0 = (wn * TN * 16 + fr) * 128 + (((0 + fg) ^ sw) & 7) * 16;
  const uint32_t w_off1 = (wn * TN * 16 + fr) * 128 + (((4 + fg) ^ sw) & 7) * 16;

  STAMP(2);
  int krem = a.K - fg * 8;      // > 0 while this lane's chunk is a real k (the Kpad tail multiplies zero weights)
  for (int kt = 0; kt < nk; ++kt) {
    const int stage = kt % NSTAGE;
    if constexpr (SPEC) {
      if (kt == 0) wait_vmcnt<0>();          // this wave's share of the patch fill
    } else {
      const int pending = min(AHEAD - 1, nk - 1 - kt);
      if (pending >= 2)
        wait_vmcnt<2 * IPW_B>();
      else if (pending == 1)
        wait_vmcnt<IPW_B>();
      else
        wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();
    if (kt == 0) { STAMP(3); }
    if constexpr (!SPEC) {
      if (kt + AHEAD < nk) issue_w(kt + AHEAD, (kt + AHEAD) % NSTAGE);
    }
    const uint32_t sb = lds0 + stage * W_STAGE;
    const uint32_t k0 = krem > 0 ? koff : 0u;
    advance();
    const uint32_t k1 = krem > 32 ? koff : 0u;
    advance();
    krem -= 64;
    u32x4_t xf0[TM], xf1[TM], wf0[TN], wf1[TN];
    static_for<0, TN>([&](auto i) { wf0[i] = lds_read128<decltype(i)::value * 2048>(sb + w_off0); });
    static_for<0, TM>([&](auto j) { xf0[j] = lds_read128<0>(xb[decltype(j)::value] + k0); });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, TN>([&](auto i) { wf1[i] = lds_read128<decltype(i)::value * 2048>(sb + w_off1); });
    static_for<0, TM>([&](auto j) { xf1[j] = lds_read128<0>(xb[decltype(j)::value] + k1); });
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j)
        acc[i][j] = Half16<HT>::mfma(__builtin_bit_cast(bf16x8_t, wf0[i]),
                                                            __builtin_bit_cast(bf16x8_t, xf0[j]), acc[i][j]);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j)
        acc[i][j] = Half16<HT>::mfma(__builtin_bit_cast(bf16x8_t, wf1[i]),
                                                            __builtin_bit_cast(bf16x8_t, xf1[j]), acc[i][j]);
  }

  STAMP(4);
  conv_store_tiles<HT, TN, TM>(a, acc, bn0 + wn * TN * 16, fg * 4, mrow);
  STAMP(5);
}

template <typename HT, int TM, int TN, int WM, int WN, int NSTAGE>
__global__ __launch_bounds__(dma_threads(WM, WN, NSTAGE)) void conv_patch_kernel(ConvArgs a) {
  constexpr int BN = 16 * TN * WN;
  const int tiles_n = (a.Cout + BN - 1) / BN;
  const int l = xcd_tile_index(a.tiles_m * tiles_n);
  if (l < 0) return;
  conv_patch_body<HT, TM, TN, WM, WN, NSTAGE>(a, l / tiles_n, l % tiles_n);
}

// Grouped launch (the same-depth convs of an Inception block): flat workgroup id -> (member, tile).
template <typename HT, int TM, int TN, int WM, int WN, int NSTAGE>
__global__ __launch_bounds__(dma_threads(WM, WN, NSTAGE)) void conv_patch_grouped_kernel(const ConvArgs* __restrict__ args, int n, int total) {
  constexpr int BN = 16 * TN * WN;
  const int bid = blockIdx.x;
  if (bid >= total) return;
  int p = 0;
  for (int i = 1; i < n; ++i)
    if (bid >= args[i].blk0) p = i;
  const ConvArgs a = args[p];
  const int local = bid - a.blk0;
  if (a.member_kind == 1) {
    pool_bn_relu_member<HT>(a, local);
    return;
  }
  const int tiles_n = (a.Cout + BN - 1) / BN;
  conv_patch_body<HT, TM, TN, WM, WN, NSTAGE>(a, local / tiles_n, local % tiles_n);
}

// Host side: tile geometry for a BM-pixel tile.  Returns false when the layer is not
// eligible (stride, channel granularity, LDS).
static bool patch_geometry(const ConvArgs& a, int BM, int BN, int nstage, PatchGeo& g) {
  if (a.SH != 1 || a.SW != 1 || a.Cin < 32 || a.Cin % 16 != 0 || a.x_cs % 8 != 0 || a.x_co % 8 != 0) return false;
  const int PXB = a.Cin * 2;
  const int PXBp = PXB + ((PXB % 64 == 0) ? 32 : 0);
  const int ring = nstage * BN * 128;
  const long GR = (long)a.B * a.Ho;
  double best = -1.0;
  for (int ncol = 1; ncol <= a.Wo; ++ncol) {
    const int TC = (a.Wo + ncol - 1) / ncol;
    if (TC > BM) continue;
    if ((ncol - 1) * TC >= a.Wo) continue;        // an empty last column tile
    int TR = BM / TC;
    if (TR > GR) TR = (int)GR;
    if (TR < 1) continue;
    const int PW = TC + a.KW - 1;
    const int cross = (a.Ho - 1 + TR - 1) / a.Ho;
    const int NR = TR + (a.KH - 1) * (cross + 1);
    // Bank pattern of a pixel-operand read: the 16 pixels of an MFMA column tile are CONSECUTIVE tile pixels, and the
    // pixel stride (an odd multiple of 32 B) spreads 16 consecutive patch pixels over 16 distinct 16-byte bank groups.
    // A column tile that wraps to the next output row (TC is not a multiple of 16: 52, 25) continues KW - 1 pixels
    // further on, which breaks the pattern (2-way conflicts: SQ_LDS_BANK_CONFLICT 26-37 % of the LDS cycles in
    // profiles/r03_cnn_mfma_counters_1280.json).  The row pitch is therefore padded so that rowB == TC * PXBp (mod 256):
    // the first pixel of the next row lands on the banks its predecessor's successor would have had.  The same for the
    // KH - 1 halo rows between two images of a tile: gapB makes (KH - 1) * rowB + gapB == 0 (mod 256).
    // Two workgroups per CU are worth far more than the clean bank pattern (52x52 3x3 80 -> 192, 256 x 64 tile: 1.14 ms
    // at 79.8 KB against 1.95 ms once the padding pushed it over 80 KB): the padded pitch is dropped where it costs
    // the second workgroup.
    if ((long)PW * (PXBp / 16) * (PXBp / 16) >= 60000) continue;   // exactness range of the cmagic division
    if (PW * (PXBp / 16) > 64 * kPatchMaxParts) continue;          // DMA pieces per patch row
    int rowB = PW * PXBp + (((TC - PW) * PXBp) % 256 + 256) % 256;
    int gapB = (256 - ((a.KH - 1) * rowB) % 256) % 256;
    long lds = (long)NR * rowB + (long)(cross + 1) * gapB + ring;
    const long lds_plain = (long)NR * PW * PXBp + ring;
    if (lds > 160 * 1024 || (lds > 80 * 1024 && lds_plain <= 80 * 1024)) {
      rowB = PW * PXBp;
      gapB = 0;
      lds = lds_plain;
    }
    if (lds > 160 * 1024) continue;
    // useful pixels per tile slot, discounted by the DMA lanes the patch fill issues per useful 16-byte chunk
    // (halo rows / columns, the 32-byte pixel padding, 64-lane granularity of a patch row)
    double eff = (double)a.Wo * TR / ((double)ncol * BM);
    const int parts = (PW * (PXBp / 16) + 63) / 64;
    const double amp = (double)NR * parts * 64 / ((double)TR * TC * (a.Cin / 8));
    eff /= (1.0 + 0.25 * amp);
    if (lds > 80 * 1024) eff *= 0.85;              // one workgroup per CU
    if (eff > best) {
      best = eff;
      g.TC = TC; g.TR = TR; g.ncol = ncol; g.PW = PW; g.PXBp = PXBp; g.CPP = a.Cin / 8; g.CPPp = PXBp / 16;
      g.cmagic = (65536 + g.CPPp - 1) / g.CPPp;
      g.NR = NR; g.Hp = a.Ho + a.KH - 1; g.rowB = rowB; g.gapB = gapB; g.lds_bytes = (int)lds;
    }
  }
  return best > 0;
}

static void apply_geometry(ConvArgs& b, const PatchGeo& g) {
  b.p_TC = g.TC; b.p_TR = g.TR; b.p_ncol = g.ncol; b.p_PW = g.PW; b.p_PXBp = g.PXBp; b.p_CPP = g.CPP;
  b.p_CPPp = g.CPPp; b.p_cmagic = g.cmagic; b.p_NR = g.NR; b.p_Hp = g.Hp; b.p_rowB = g.rowB; b.p_gapB = g.gapB;
  const long GR = (long)b.B * b.Ho;
  b.tiles_m = (int)((GR + g.TR - 1) / g.TR) * g.ncol;
}

template <typename HT, int TM, int TN, int WM = 4, int WN = 1, int NSTAGE = 3>
int launch_patch(const ConvArgs& a, hipStream_t st) {
  PatchGeo g;
  constexpr int BM = 16 * TM * WM, BN = 16 * TN * WN;
  if (!patch_geometry(a, BM, BN, ring_stages(NSTAGE), g)) {
    comic_set_error("conv: layer not eligible for the patch kernel (stride %d, Cin %d)", a.SH, a.Cin);
    return 3;
  }
  static PerDeviceOnce attr_once__;
  bool& attr_set = attr_once__.slot();   // hipFuncSetAttribute holds per device
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)conv_patch_kernel<HT, TM, TN, WM, WN, NSTAGE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024) != hipSuccess) {
      comic_set_error("conv: cannot reserve LDS for the patch kernel");
      return 1;
    }
    attr_set = true;
  }
  ConvArgs b = a;
  apply_geometry(b, g);
  const long total = (long)b.tiles_m * cdiv(a.Cout, BN);
  if (total >= (1L << 31) - 8) {
    comic_set_error("conv: too many tiles");
    return 1;
  }
  const int lds = std::max(g.lds_bytes, a.min_lds);
  hipLaunchKernelGGL((conv_patch_kernel<HT, TM, TN, WM, WN, NSTAGE>), dim3((unsigned)((total + 7) / 8 * 8)),
                     dim3(dma_threads(WM, WN, NSTAGE)), lds, st, b);
  return 0;
}

template <typename HT, int TM, int TN, int WM = 4, int WN = 1, int NSTAGE = 3>
int launch_patch_grouped(const ConvArgs* args_dev, int n, int total_blocks, int lds_bytes, hipStream_t st) {
  static PerDeviceOnce attr_once__;
  bool& attr_set = attr_once__.slot();   // hipFuncSetAttribute holds per device
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)conv_patch_grouped_kernel<HT, TM, TN, WM, WN, NSTAGE>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
      comic_set_error("conv: cannot reserve LDS for the grouped patch kernel");
      return 1;
    }
    attr_set = true;
  }
  const int lds = lds_bytes;
  hipLaunchKernelGGL((conv_patch_grouped_kernel<HT, TM, TN, WM, WN, NSTAGE>), dim3((unsigned)total_blocks),
                     dim3(dma_threads(WM, WN, NSTAGE)), lds, st, args_dev, n, total_blocks);
  return 0;
}

// (BM, BN, ring stages) of the patch tile ids 13..25, in the order of launch_dma_tile's switch
// ids 48..53: four MFMA waves + four loader waves (512 threads)
struct PatchTile { int BM, BN, threads; };
constexpr PatchTile kPatchTiles[19] = {{256, 64, 256}, {256, 32, 256}, {256, 96, 256}, {128, 64, 256}, {128, 32, 256},
                                       {128, 96, 256}, {256, 128, 512}, {256, 192, 768}, {512, 64, 512}, {256, 64, 512},
                                       {256, 192, 512}, {128, 128, 512}, {128, 192, 512},
                                       {256, 64, 512}, {256, 32, 512}, {256, 96, 512}, {128, 96, 512}, {128, 192, 512},
                                       {128, 128, 512}};
constexpr int kPatchLoaderTile0 = 48;
inline int patch_tile_index(int tile) { return tile >= kPatchLoaderTile0 ? 13 + (tile - kPatchLoaderTile0) : tile - 13; }

template <typename HT>
int launch_patch_grouped_tile(int tile, const ConvArgs* args_dev, int n, int total_blocks, int lds, hipStream_t st) {
  switch (tile) {
    case 13: return launch_patch_grouped<HT, 4, 4>(args_dev, n, total_blocks, lds, st);
    case 14: return launch_patch_grouped<HT, 4, 2>(args_dev, n, total_blocks, lds, st);
    case 15: return launch_patch_grouped<HT, 4, 6>(args_dev, n, total_blocks, lds, st);
    case 16: return launch_patch_grouped<HT, 2, 4>(args_dev, n, total_blocks, lds, st);
    case 17: return launch_patch_grouped<HT, 2, 2>(args_dev, n, total_blocks, lds, st);
    case 18: return launch_patch_grouped<HT, 2, 6>(args_dev, n, total_blocks, lds, st);
    case 19: return launch_patch_grouped<HT, 4, 4, 4, 2>(args_dev, n, total_blocks, lds, st);
    case 20: return launch_patch_grouped<HT, 4, 4, 4, 3>(args_dev, n, total_blocks, lds, st);
    case 21: return launch_patch_grouped<HT, 4, 4, 8, 1>(args_dev, n, total_blocks, lds, st);
    case 22: return launch_patch_grouped<HT, 4, 2, 4, 2>(args_dev, n, total_blocks, lds, st);
    case 23: return launch_patch_grouped<HT, 4, 6, 4, 2>(args_dev, n, total_blocks, lds, st);
    case 24: return launch_patch_grouped<HT, 2, 4, 4, 2>(args_dev, n, total_blocks, lds, st);
    case 25: return launch_patch_grouped<HT, 2, 6, 4, 2>(args_dev, n, total_blocks, lds, st);
    case 48: return launch_patch_grouped<HT, 4, 4, 4, 1, kLoaderWaves + 3>(args_dev, n, total_blocks, lds, st);
    case 49: return launch_patch_grouped<HT, 4, 2, 4, 1, kLoaderWaves + 3>(args_dev, n, total_blocks, lds, st);
    case 50: return launch_patch_grouped<HT, 4, 6, 4, 1, kLoaderWaves + 3>(args_dev, n, total_blocks, lds, st);
    case 51: return launch_patch_grouped<HT, 2, 6, 4, 1, kLoaderWaves + 3>(args_dev, n, total_blocks, lds, st);
    case 52: return launch_patch_grouped<HT, 4, 6, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, lds, st);
    case 53: return launch_patch_grouped<HT, 4, 4, 2, 2, kLoaderWaves + 3>(args_dev, n, total_blocks, lds, st);
    default:
      comic_set_error("conv: unknown patch tile id %d", tile);
      return 2;
  }
}
