// The f16mx stem for float32 NCHW input as a 12-wave kernel of its own (included by stem.hip, inside namespace oibl,
// behind stem_parts.h, whose parts it shares with the 16-wave kernel vgg_stem_mx_kernel of stem_mx16.h: formats,
// roles and numerics are described there).
//
// vgg_stem_mx_kernel gives a consumer wave 32 output channels x 64 pixels: per tap 12 ds_read_b128 for 6 matrix
// instructions — every pixel fragment is read once per output-channel half, every weight fragment by all four
// waves — and the four consumers are bound by the LDS port, not by the matrix pipe.  Here a consumer
// wave holds BOTH output-channel halves of its 64 pixels (64 accumulators): per tap 8 weight reads + 8 pixel reads
// for 12 matrix instructions, a third fewer operand bytes.  That needs more than the 128 VGPRs a 16-wave workgroup
// leaves a wave, hence 12 waves (168 VGPRs): 4 consumers, 8 producers.
//
//   tile = stage A (input half 0, halo buffer 0), stage B (input half 1, buffer 1), ONE epilogue (both output halves)
//   producers, stage A: conv1_1 half 1 of this tile -> buffer 1, then convert the next tile's window
//              stage B: conv1_1 half 0 of the next tile -> buffer 0, gather the tile after next
//   The 11 blocks of 32 halo pixels go to 8 waves: wave pw owns block pw, waves 0-2 also block pw + 8 (per SIMD that
//   is three blocks, as with twelve waves).  The block loop is NOT unrolled (one conv1_1 body per site).
//
// Weights: a stage needs all 72 KB (9 taps x 64 out x 32 in), so the next stage's image cannot land beside it; it
// is refilled by tap group.  Behind the MID barrier of a stage (every consumer is past tap 4) the next stage's taps 0-4
// stream into those slots; its taps 5-8 stream at the head of that next stage.  The streaming waves (producers 4-7:
// they wait at the barriers, the consumers do not) wait for their pieces in front of the mid and the end barrier, so each
// group has landed, workgroup-wide, before its first read (the table at produce_stage).  144 KB per tile.
//
// Synchronisation is s_barrier only: 1 after the prologue + M12_BARRIERS_PER_TILE per tile, the same compile-time
// sequence (mid A, end A, mid B, end B) in both roles; nothing that is conditional skips a barrier.
//
// Numerics: every output element accumulates its taps of input half 0, then of half 1, in tap order, f16 slot 0, f16
// slot 1, scaled e2m3 — the order of stages S1, S2 of vgg_stem_mx_kernel; pooling, bias, clamp, mx_pack_half and
// the stores are the same functions (stem_parts.h): the lines are bit-identical (tests/test_gpu_stem_mx12.py).
constexpr int M12_PROD = 8;                 // producer waves
constexpr int M12_BARRIERS_PER_TILE = 4;    // mid A, end A, mid B, end B
constexpr int M12_LO_TAPS = 5;              // taps 0-4: refilled behind the mid barrier; taps 5-8 at the head of a stage

__global__ __launch_bounds__(64 * (4 + M12_PROD)) void stem_mx12_kernel(StemParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const wl = smem;                 // [tap][output half c][32 rows][f16mx line of the stage's input half]
  char* const hb = smem + S3_W_BYTES;    // halo buffer h: channels 32h..32h+31 of the current tile
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const StemTiles tiles = stem_xcd_tiles(p.ntiles);
  const int first = tiles.first, stride = tiles.stride, niter = tiles.niter;
  const int Ho = p.H >> 1, Wo = p.W >> 1;
  stem_bias_to_lds(smem, p.b1, p.b2, p.act_scale);
  float range_seen = 0.f;   // (mx_raise_if_out_of_range)
  using H0 = std::integral_constant<int, 0>;
  using H1 = std::integral_constant<int, 1>;

  if (wave >= 4) {
    // ================================ producers (waves 4-11) ====================================
    // The producers' parts of stem_parts.h — gather as nine rows of three pixels, conv1_1 in split bf16, half-line
    // packing, the conflict-free lane -> pixel map — over one or two blocks per wave.
    // (the lane id is made inside each role: a value computed in front of the role split stays live through both)
    const int lane = fresh_lane_id(), half = lane >> 5, l31 = lane & 31;
    const int pprio = p.prod_prio & 3;
    stem_raise_prio(pprio);
    const int pw = wave - 4;                                  // 0..7
    const int nb = pw + M12_PROD < ST_BLOCKS ? 2 : 1;         // blocks pw and (waves 0-2) pw + 8 of the 11
    const __amdgpu_buffer_rsrc_t rs_x =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, (int)p.x_bytes, 0x00020000);
    bf16x8_t wh[2][2], wlo[2][2];
    stem_w1_fragments<K_ROWS, true>(p.w1, p.act_scale, half, l31, wh, wlo);
    const float* const bias_l = reinterpret_cast<const float*>(smem + S3_BIAS_OFF) + 16 * half;
    const int lpix = mx_lane_pixel(l31);
    auto row_of = [&](int bi) __attribute__((always_inline)) { return 32 * (pw + M12_PROD * bi) + lpix; };
    int g_swz[2], g_rel[2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
      int hy, hx;
      stem_halo_yx(row_of(bi), hy, hx);
      g_swz[bi] = c64_swz(hy, hx);
      g_rel[bi] = hy * p.W + hx;
    }
    float xv[2][16];
    int xfix[2] = {0, 0};   // image edge: 1 = this pixel's rows were fetched from x (not x - 1), 2 = from x - 2
    auto issue_loads = [&](int tile) __attribute__((always_inline)) {
      const StemTile t = stem_tile(p, tile);
#pragma unroll
      for (int bi = 0; bi < 2; ++bi) {
        if (bi >= nb) continue;   // wave-uniform
        xfix[bi] = mx_gather_rows(rs_x, p, t, row_of(bi), g_rel[bi], half, xv[bi]);
      }
    };
    bf16x8_t xh[2][2], xl[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          xh[bi][s][e] = 0;
          xl[bi][s][e] = 0;
        }
    auto convert = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int bi = 0; bi < 2; ++bi) {
        if (bi >= nb) continue;
        mx_edge_fix(xv[bi], xfix[bi]);
        x3_split_window(xv[bi], xh[bi], xl[bi]);
      }
    };
    // conv1_1 of channel half h on block bi, bias + clamp + half-line packing, halo lines -> LDS.  bi is a RUN-TIME,
    // wave-uniform index: the body is not cloned per block — one conv1_1 body per site keeps the text at 234 matrix
    // instructions — and its 16 fragment registers are SELECTED: 16 v_cndmask (+ 1 for the swizzle) of the ~220 vector
    // instructions of a block and half, ~7 % of the producers' vector work, ~0.2k of a block's 3.0k ticks.  That is the
    // price of the pinned count on the role that bounds the kernel.  Moving block 1's fragments behind a scalar branch
    // instead (8 v_mov_b64 per block, 8 more on block 1) measured no better: producer work 12.7-12.8k against 12.5-12.6k ticks
    // per tile, the launch 1.31 against 1.29 ms (profiles/stem_mx12_ab.txt).
    auto produce_one = [&](int tile, auto h_c, int bi, char* buf) __attribute__((always_inline)) {
      constexpr int h = decltype(h_c)::value;
      const StemTile t = stem_tile(p, tile);
      const bf16x8_t bh0 = bi ? xh[1][0] : xh[0][0], bh1 = bi ? xh[1][1] : xh[0][1];
      const bf16x8_t bl0 = bi ? xl[1][0] : xl[0][0], bl1 = bi ? xl[1][1] : xl[0][1];
      f32x16_t acc;
      stem_bias16(bias_l + 32 * h, 4, acc);
      acc = conv1_1_sextet(wh[h], wlo[h], bh0, bh1, bl0, bl1, acc);
      stem_restore_prio(pprio);
      const int r = row_of(bi);
      MxHalfLine L;
      mx_clamp_pack_half(acc, stem_halo_pixel_in_image(p, t, r), L, range_seen);
      if (r < ST_HALO_PX)   // (block 10 has 12 surplus lanes)
        mx_write_half_line(buf + r * 128, bi ? g_swz[1] : g_swz[0], half, L);
    };
    // conv1_2's weights: LDS row (tap * 2 + c) * 32 + m = the f16mx line of output channel 32 c + chan(m), the stage's
    // input group; 16-byte slots swizzled by (m >> 1) & 7.  One LDS-DMA instruction fills 8 rows; piece 4 j + k holds
    // rows m = 8 k .. 8 k + 7 of (tap, c) = (j >> 1, j & 1).  Waves 4-7 stream the pieces k = pw & 3 (the lane's part of
    // the source offset is ONE register): taps 0-4 = j 0..9 (10 pieces per wave), taps 5-8 = j 10..17 (8 per wave).
    // The streaming sits with the producers because they wait at the barriers and the consumers do not (a piece costs
    // its issuer 60-185 cycles), and with waves 4-7 because they have one block of halo pixels: waves 0-2 have two.
    const int wk = pw & 3;
    const int wm_row = 8 * wk + (lane >> 3);
    const unsigned w_voff = (unsigned)((16 * ((wm_row >> 2) & 1) + 4 * (wm_row >> 3) + (wm_row & 3)) * 256 +
                                       ((lane & 7) ^ (4 * (wk & 1) + (lane >> 4))) * 16);
    const __amdgpu_buffer_rsrc_t rs_w2 =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p.w2), 0, 9 * 64 * 256, 0x00020000);
    auto stream_w = [&](int h, auto lo_c) __attribute__((always_inline)) {
      constexpr bool lo = decltype(lo_c)::value;
      constexpr int j0 = lo ? 0 : 2 * M12_LO_TAPS, j1 = lo ? 2 * M12_LO_TAPS : 18;
      if (pw < 4) return;   // wave-uniform
#pragma unroll
      for (int j = j0; j < j1; ++j) {
        buf_glds16(rs_w2, w_voff, (unsigned)(((j >> 1) * 64 + 32 * (j & 1)) * 256 + h * 128), wl + (j * 4 + wk) * 1024);
      }
    };
    const bool prof = p.prof != nullptr && blockIdx.x == 0 && wave == 4;
    unsigned long long pt[2] = {0, 0}, t0 = 0;   // work, wait
    auto barrier = [&]() __attribute__((always_inline)) {
      const unsigned long long t1 = prof ? __builtin_amdgcn_s_memtime() : 0;
      __builtin_amdgcn_s_barrier();
      if (prof) {
        const unsigned long long t2 = __builtin_amdgcn_s_memtime();
        pt[0] += t1 - t0;
        pt[1] += t2 - t1;
        t0 = t2;
      }
    };
    // One stage of a tile.  h = the conv1_1 half PRODUCED (beside it the consumers multiply input half h ^ 1);
    // MIDPOS = the block behind which the MID barrier stands; conv_after = convert the next tile's window behind the
    // blocks; nh = input half of the NEXT stage (< 0: none); late_tile = the tile whose gathers go out (< 0: none).
    // What a wave issues to the vector-memory counter, in order, and what each wait leaves in flight:
    //
    //                     waves 0-3 (no streaming; 0-2 two blocks)      waves 4-7 (streaming, one block)
    //   stage A  head     -                                             8 pieces: taps 5-8 of input half 0
    //            blocks   both blocks (MIDPOS = 1)                      its block
    //            MID      no wait                                       vmcnt(0): the 8 pieces (and the older gathers of
    //                                                                   tile it+1, a stage old) have landed
    //            behind   -                                             10 pieces: taps 0-4 of input half 1
    //            then     convert tile it+1 (the compiler waits for ITS gathers)            likewise
    //            END      no wait                                       vmcnt(0): the 10 pieces have landed
    //   stage B  head     -                                             8 pieces: taps 5-8 of input half 1
    //            block 0  block 0 (MIDPOS = 0)                          its block
    //            MID      no wait                                       vmcnt(0): the 8 pieces
    //            behind   gathers of tile it+2 (5 per block)            10 pieces: taps 0-4 of the next tile's input
    //                                                                   half 0, THEN the 5 gathers of tile it+2
    //            block 1  block 1 (waves 0-2)                           -
    //            END      no wait: the gathers stay in flight           tile it+2 interior: vmcnt(5) — the 5 gathers,
    //                                                                   the newest, stay in flight; else vmcnt(0)
    //
    // A wave that streams nothing has nothing another wave reads through the counter: its LDS writes are covered by
    // lgkmcnt(0), its gathers by the compiler's own waits in convert().  The ONE counted wait counts only gathers of an
    // INTERIOR tile: every lane of those is in range and touches memory.  On a border tile a block can lie wholly outside
    // the image, all 64 lanes of its gathers carry the out-of-range offset, and such an instruction was seen to retire
    // ahead of older in-range loads (counted waits may only count instructions that touch memory) — behind
    // it a weight piece could still be in flight at END; there the wait is vmcnt(0), on border tiles only.
    // The block loop stays a loop (run-time trip count) and produce_one selects its operands: see produce_one.
    // (Measured per tile: a block 3.0k cycles, taps 0-4 2.6k, taps 5-8 2.1k, the epilogue 3.1k: hence the placement.)
    static_assert(4 + M12_PROD >= ST_BLOCKS, "the streaming waves 4-7 must have one block: their counted wait is vmcnt(5)");
    const bool streams = pw >= 4;   // wave-uniform
    auto produce_stage = [&](int tile, auto h_c, char* buf, bool active, auto mid_c, int nh, int late_tile,
                             auto midpos_c, bool conv_after) __attribute__((always_inline)) {
      constexpr bool MID = decltype(mid_c)::value;
      constexpr int MIDPOS = decltype(midpos_c)::value;
      if (MID) stream_w(decltype(h_c)::value ^ 1, std::false_type{});
      bool late_interior = false;
      if (late_tile >= 0) late_interior = stem_tile(p, late_tile).interior;
      int nblk = 2;
      asm volatile("" : "+s"(nblk));   // (a run-time trip count: the loop stays a loop)
#pragma unroll 1
      for (int bi = 0; bi < nblk; ++bi) {
        if (active && bi < nb) produce_one(tile, h_c, bi, buf);
        if (MID && bi == MIDPOS) {
          if (streams) wait_vmcnt<0>();
          barrier();
          if (nh >= 0) stream_w(nh, std::true_type{});
          if (late_tile >= 0) issue_loads(late_tile);
        }
      }
      if (conv_after) convert();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (MID) {
        if (streams) {
          if (late_interior) wait_vmcnt<5>();
          else wait_vmcnt<0>();
        }
        barrier();
      }
    };
    if (niter > 0) {
      issue_loads(first);
      convert();
      if (niter > 1) issue_loads(first + stride);
    }
    produce_stage(first, H0{}, hb, niter > 0, std::false_type{}, -1, -1, H0{}, false);
    stream_w(0, std::true_type{});
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    t0 = prof ? __builtin_amdgcn_s_memtime() : 0;
#pragma unroll 1
    for (int it = 0; it < niter; ++it) {
      // stage A: the tile's second channel half into buffer 1 (last read in stage B of the previous tile)
      const bool more = it + 1 < niter;
      produce_stage(first + it * stride, H1{}, hb + ST_HALO_BYTES, true, std::true_type{}, 1, -1, H1{}, more);
      // stage B: the first channel half of tile it+1 (its window was converted at the end of stage A, when this
      // tile's fragments were no longer needed) goes into buffer 0 (last read in stage A); the gathers of tile it+2 go out
      produce_stage(first + (it + 1) * stride, H0{}, hb, more, std::true_type{}, more ? 0 : -1,
                    it + 2 < niter ? first + (it + 2) * stride : -1, H0{}, false);
    }
    if (prof && fresh_lane_id() == 0) {
      p.prof[4] = pt[0];
      p.prof[5] = pt[1];
      p.prof[6] = 0;
      p.prof[7] = 0;
    }
    mx_raise_if_out_of_range(range_seen, p.range_flag);
    return;
  }

  // ================================== consumers (waves 0-3) =====================================
  typedef stem_u4 u4;
  const int lane = fresh_lane_id(), half = lane >> 5, l31 = lane & 31;
  stem_raise_prio((p.prod_prio >> 2) & 3);
  // pixel (B) fragment addressing: stem_pixel_addressing, mx_weight_row
  // LDS addresses are kept as INTEGERS and turned into pointers at the read (as pointers every read pays a v_add of
  // the — zero — base of the dynamic allocation: on a SIMD whose vector ALU the producers fill, each vector instruction
  // of the consumers is time).  The kernel has no static LDS: smem starts the allocation, and its base — part of every
  // address below — is a multiple of 128, which the XORed slot bits need.
  typedef const __attribute__((address_space(3))) char* lds_t;
  const int lds0 = (int)(size_t)(lds_t)smem;
  auto at = [&](int a, int off) __attribute__((always_inline)) { return (lds_t)(size_t)(unsigned)a + off; };
  int e_kx[3], pxb;
  stem_pixel_addressing(wave, half, l31, e_kx, pxb);
  pxb += lds0;
  const int w_base = lds0 + mx_weight_row(half, l31);
  __builtin_amdgcn_s_barrier();
  const bool cprof = p.prof != nullptr && blockIdx.x == 0 && wave == 0;
  unsigned long long ct[3] = {0, 0, 0}, c0 = cprof ? __builtin_amdgcn_s_memtime() : 0;
  auto barrier = [&]() __attribute__((always_inline)) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (the epilogue's stores stay in flight)
    const unsigned long long c1 = cprof ? __builtin_amdgcn_s_memtime() : 0;
    __builtin_amdgcn_s_barrier();
    if (cprof) {
      const unsigned long long c2 = __builtin_amdgcn_s_memtime();
      ct[0] += c1 - c0;
      ct[1] += c2 - c1;
      c0 = c2;
    }
  };
  f32x16_t acc[2][2];   // [output half c][pixel block i]
  // operand registers, single-buffered: a fragment is reloaded for the next tap right behind the last MFMA that reads
  // it.  MFMA order per operand part: (c0,i0) (c0,i1) (c1,i0) (c1,i1); every reload is >= 7 MFMAs ahead of its use.
  f16x8_t w0[2], w1[2], b0[2], b1[2];
  u4 wma[2], wmt[2], bma[2], bmt[2];
  // taps T0 .. T1-1 of stage h out of halo buffer h
  auto sub_pass = [&](auto h_c, auto t0_c, auto t1_c) __attribute__((always_inline)) {
    constexpr int h = decltype(h_c)::value, T0 = decltype(t0_c)::value, T1 = decltype(t1_c)::value;
    int pc;   // (volatile: one live register, pxb, for both halo buffers)
    asm volatile("v_add_u32 %0, %1, %2" : "=v"(pc) : "s"(S3_W_BYTES + h * ST_HALO_BYTES), "v"(pxb));
    auto paddr = [&](int tap, int part) __attribute__((always_inline)) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      const int c = (part == 0 ? 0 : part == 1 ? 32 : part == 2 ? 80 : 112) ^ ((ky & 1) << 6);
      int a;   // (volatile: computed where it is used — hoisted out of the tile loop the 72 addresses spill)
      asm volatile("v_xad_u32 %0, %1, %2, %3" : "=v"(a) : "v"(e_kx[kx]), "s"(c), "v"(pc));
      return a;
    };
    auto poff = [&](int tap, int i) __attribute__((always_inline)) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      return (ky * C64_HW + kx) * 128 + i * 2048;
    };
    auto waddr = [&](int kk) __attribute__((always_inline)) {
      int a = w_base;   // (volatile: ONE live register for the four slot addresses: mx_weight_row)
      if (kk) asm volatile("v_xor_b32 %0, %1, %2" : "=v"(a) : "s"(kk << 5), "v"(w_base));
      return a;
    };
    typedef const __attribute__((address_space(3))) f16x8_t* lds_h8;
    typedef const __attribute__((address_space(3))) u4* lds_u4;
    auto ld_b0 = [&](int tap, int i, int a) __attribute__((always_inline)) { b0[i] = *(lds_h8)at(a, poff(tap, i)); };
    auto ld_b1 = [&](int tap, int i, int a) __attribute__((always_inline)) { b1[i] = *(lds_h8)at(a, poff(tap, i)); };
    auto ld_bm = [&](int tap, int i, int a2, int a3) __attribute__((always_inline)) {
      bma[i] = *(lds_u4)at(a2, poff(tap, i));
      bmt[i] = *(lds_u4)at(a3, poff(tap, i));
    };
    auto ld_w0 = [&](int tap, int c, int a) __attribute__((always_inline)) { w0[c] = *(lds_h8)at(a, tap * 8192 + c * 4096); };
    auto ld_w1 = [&](int tap, int c, int a) __attribute__((always_inline)) { w1[c] = *(lds_h8)at(a, tap * 8192 + c * 4096); };
    auto ld_wm = [&](int tap, int c) __attribute__((always_inline)) {
      wma[c] = *(lds_u4)at(waddr(2), tap * 8192 + c * 4096);
      wmt[c] = *(lds_u4)at(waddr(3), tap * 8192 + c * 4096);
    };
    auto f0 = [&](int c, int i) __attribute__((always_inline)) {
      acc[c][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w0[c], b0[i], acc[c][i], 0, 0, 0);
    };
    auto f1 = [&](int c, int i) __attribute__((always_inline)) {
      acc[c][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1[c], b1[i], acc[c][i], 0, 0, 0);
    };
    auto mx = [&](int c, int i) __attribute__((always_inline)) {
      acc[c][i] = mx_scaled_mfma(wma[c], wmt[c], bma[i], bmt[i], acc[c][i]);
    };
#define M12_SB() __builtin_amdgcn_sched_barrier(0)
    {
      const int a0 = paddr(T0, 0), a1 = paddr(T0, 1), a2 = paddr(T0, 2), a3 = paddr(T0, 3), x1 = waddr(1);
      ld_w0(T0, 0, w_base);
      ld_b0(T0, 0, a0);
      ld_b0(T0, 1, a0);
      ld_w0(T0, 1, w_base);
      ld_w1(T0, 0, x1);
      ld_b1(T0, 0, a1);
      ld_b1(T0, 1, a1);
      ld_w1(T0, 1, x1);
      ld_wm(T0, 0);
      ld_bm(T0, 0, a2, a3);
      ld_bm(T0, 1, a2, a3);
      ld_wm(T0, 1);
    }
#pragma unroll
    for (int tap = T0; tap < T1; ++tap) {
      // (sched_barrier: the order below IS the schedule.  An address is computed once per operand part and tap and
      //  serves the reads of both blocks / both output halves: it lives across two MFMAs.)
      const bool more = tap + 1 < T1, late = tap > T0;
      const int n = tap + 1;
      int a = 0;
      M12_SB();
      f0(0, 0);
      M12_SB();
      if (late) ld_wm(tap, 1);   // (the last four reads of a tap are issued inside it: the counter holds 15)
      M12_SB();
      f0(0, 1);
      M12_SB();
      if (late) ld_bm(tap, 1, paddr(tap, 2), paddr(tap, 3));
      if (more) ld_w0(n, 0, w_base);
      M12_SB();
      f0(1, 0);
      M12_SB();
      if (more) {
        a = paddr(n, 0);
        ld_b0(n, 0, a);
      }
      M12_SB();
      f0(1, 1);
      M12_SB();
      if (more) {
        ld_w0(n, 1, w_base);
        ld_b0(n, 1, a);
      }
      M12_SB();
      f1(0, 0);
      M12_SB();
      f1(0, 1);
      M12_SB();
      if (more) ld_w1(n, 0, waddr(1));
      M12_SB();
      f1(1, 0);
      M12_SB();
      if (more) {
        a = paddr(n, 1);
        ld_b1(n, 0, a);
      }
      M12_SB();
      f1(1, 1);
      M12_SB();
      if (more) {
        ld_w1(n, 1, waddr(1));
        ld_b1(n, 1, a);
      }
      M12_SB();
      mx(0, 0);
      M12_SB();
      mx(0, 1);
      M12_SB();
      if (more) ld_wm(n, 0);
      M12_SB();
      mx(1, 0);
      M12_SB();
      if (more) ld_bm(n, 0, paddr(n, 2), paddr(n, 3));
      M12_SB();
      mx(1, 1);
      M12_SB();
    }
#undef M12_SB
  };
  using T0c = std::integral_constant<int, 0>;
  using TMc = std::integral_constant<int, M12_LO_TAPS>;
  using T9c = std::integral_constant<int, 9>;
  auto stage = [&](auto h_c) __attribute__((always_inline)) {
    constexpr int h = decltype(h_c)::value;
    if (h == 0) {
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[c][i][r] = 0.f;
    }
    sub_pass(h_c, T0c{}, TMc{});
    barrier();                            // MID: taps 5-8 have landed; every consumer is past taps 0-4
    sub_pass(h_c, TMc{}, T9c{});
    barrier();                            // END: the halo buffer goes back; the next stage's taps 0-4 have landed
  };
#pragma unroll 1
  for (int it = 0; it < niter; ++it) {
    stage(H0{});
    stage(H1{});
    const unsigned long long e0 = cprof ? __builtin_amdgcn_s_memtime() : 0;
    // mx_pooled_epilogue, once per output-channel half
    int n, ty, tx;
    stem_decode(p, first + it * stride, n, ty, tx);
    const int oy = ty * 4 + wave;
    const int lane_e = fresh_lane_id();
    const int half = lane_e >> 5, l31 = lane_e & 31;   // (shadow the kernel's: nothing lane-derived stays live across the stages)
    // (likewise the two constants of the epilogue: made here, the bound in a scalar register — hoisted, each holds a
    //  vector register across the stages, which have none to spare)
    float f16max = 65504.f;
    unsigned zero = 0u;
    asm volatile("" : "+s"(f16max));
    asm volatile("" : "+v"(zero));
    const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(
        p.out + ((long)n * Ho + oy) * Wo * 256, 0, oy < Ho ? Wo * 256 : 0, 0x00020000);
#pragma unroll
    for (int cz = 0; cz < 2; ++cz) {
      __builtin_amdgcn_sched_barrier(0);   // (one output half at a time: interleaved, the two epilogues spill)
      const float* const bias2 = reinterpret_cast<const float*>(smem + S3_BIAS_OFF) + 64 + 32 * cz + 16 * half;
      mx_pooled_epilogue(acc[cz][0], acc[cz][1], bias2, f16max, zero, rs_o, tx, cz, half, l31, range_seen);
    }
    if (cprof) {
      const unsigned long long e1 = __builtin_amdgcn_s_memtime();
      ct[2] += e1 - e0;
      c0 = e1;
    }
  }
  if (cprof && fresh_lane_id() == 0) {
    p.prof[0] = ct[0];   // the two stages' taps
    p.prof[1] = ct[1];   // waits at the four barriers
    p.prof[2] = ct[2];   // epilogue
    p.prof[3] = 0;
  }
  mx_raise_if_out_of_range(range_seen, p.range_flag);
}
