// vgg_stem_mx_kernel<U8>: the fused f16mx stem as a 16-wave kernel (included by stem.hip inside namespace oibl, behind
// stem_parts.h; launched by launch_vgg_stem_x3).  It serves uint8 input (U8 = true), and float32 input when the test
// hook g_stem_mx12 = 0 takes the route away from the 12-wave kernel (stem_mx12.h): the other side of
// tests/test_gpu_stem_mx12.py.
//
// Roles, tiles, passes and hand-overs are those of the bf16x3 stem (stem_x3.h); what changes is the arithmetic of
// conv1_2 (2 f16 + 1 scaled-fp6 MFMA per 32 K instead of 6 bf16 ones) and therefore every format:
//   * the halo buffers hold f16mx lines (common.h) of conv1_1's output.  A 32-channel group lies along the
//     ROWS of conv1_1's accumulator tile — a lane holds 16 of a pixel's 32 channels, lane ^ 32 the rest — and
//     which channel sits in which row is free: row 8g + 4hp + r carries channel 16hp + 4g + r, so that a lane
//     owns 16 CONSECUTIVE elements of the line and packs them alone (mx_pack_half: one cross-lane maximum);
//   * conv1_2 runs transposed for the same reason — A = weights (rows = output channels, in the same row
//     order), B = halo pixels — its 2x2 max-pool is two DPP quad steps over lanes, and the pooled pixel's
//     32 channels are again one lane pair: the f16mx lines of the output map are written straight from
//     registers (a workgroup's 32 output channels are exactly one group);
//   * conv1_2's weights are the packed f16mx tensor of oibl_pack_conv3x3_weights(OIBL_F16MX).
// conv1_1 itself stays split bf16 (K = 27: 6 MFMAs per 32 pixels x 32 channels, a quarter of a pass).
//
// The f16mx stem runs ONE workgroup per tile (the bf16x3 stem two, one per output-channel half): conv1_1 + the f16mx
// line packing of a tile's 340-pixel halo — the vector-ALU work that bounds the kernel — is done ONCE instead of in
// both workgroups of a tile, and that workgroup runs BOTH halves of conv1_2's output channels one after the other over
// the same two halo buffers:
//   stage S1  consumers: channels 0-31,  input half 0 (halo buffer 0)   producers: conv1_1 half 1 of this tile -> buffer 1
//   stage S2  consumers: channels 0-31,  input half 1 (buffer 1)         producers: convert the next tile's window, gather the one after
//             consumers: pool / pack / store channels 0-31
//   stage S3  consumers: channels 32-63, input half 0 (buffer 0)         producers: —
//   stage S4  consumers: channels 32-63, input half 1 (buffer 1)         producers: conv1_1 half 0 of the NEXT tile -> buffer 0
//             consumers: pool / pack / store channels 32-63
// (buffer 0 is last read in S3, buffer 1 in S4: the producers keep their one-stage run-ahead).  conv1_2's weights no
// longer fit as residents (2 x 72 KB): the 36 KB image of the NEXT stage (its output-channel half x input half: 9 taps x
// 32 rows x 128 B) streams from L2 into the weight buffer the PREVIOUS stage used while the current one computes —
// buffer_load ... lds issued by the consumers at the head of their pass, vmcnt(0) in front of the stage's barrier:
// 147 KB per tile through the LDS-DMA path, the same 72 KB of LDS.  (1.555 -> 1.384 ms against two workgroups per tile
// with resident weights, bit-identical: DESIGN §4.5, profiles/r06_j_stem_dual_ab.txt.)
template <bool U8>
__global__ __launch_bounds__(1024) void vgg_stem_mx_kernel(StemParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const wl = smem;                 // [weight buffer][tap][32 rows][f16mx line of one input half]
  char* const hb = smem + S3_W_BYTES;    // halo buffer h: channels 32h..32h+31 of the current tile
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const StemTiles tiles = stem_xcd_tiles(p.ntiles);
  const int first = tiles.first, stride = tiles.stride, niter = tiles.niter;
  const int Ho = p.H >> 1, Wo = p.W >> 1;
  stem_bias_to_lds(smem, p.b1, p.b2, p.act_scale);
  float range_seen = 0.f;   // (mx_raise_if_out_of_range)

  if (wave >= 4) {
    // ================================ producers (waves 4-15) ====================================
    // twelve waves, one 32-pixel block of the halo each, as in the bf16x3 stem
    const int pprio = p.prod_prio & 3;
    stem_raise_prio(pprio);
    const int pw = wave - 4;   // 0..11: producer wave pw owns block pw of the 11 (wave 15 only keeps step)
    const bool has_block = pw < ST_BLOCKS;
    const __amdgpu_buffer_rsrc_t rs_x =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, (int)p.x_bytes, 0x00020000);
    bf16x8_t wh[2][2], wlo[2][2];
    stem_w1_fragments<U8 ? K_BYTES : K_ROWS, true>(p.w1, p.act_scale, half, l31, wh, wlo);
    // accumulator registers 4 j + r of this lane = channels 16 half + 4 j + r of the pass's 32
    const float* const bias_l = reinterpret_cast<const float*>(smem + S3_BIAS_OFF) + 16 * half;
    // the halo pixel of this lane (mx_lane_pixel); kept: the swizzle of its LDS row and its element offset from the
    // tile's halo origin
    const int row = 32 * pw + mx_lane_pixel(l31);
    int g_swz, g_rel;
    {
      int hy, hx;
      stem_halo_yx(row, hy, hx);
      g_swz = c64_swz(hy, hx);
      g_rel = hy * p.W + hx;
      asm volatile("" : "+v"(g_rel));
    }
    float xv[16];
    int xfix = 0;
    U8Window u8w = {};
    float ka[3] = {0.f, 0.f, 0.f}, kb[3] = {0.f, 0.f, 0.f};
    if constexpr (U8) u8_lane_constants(p, half, ka, kb);
    // issue the input gathers of one tile; nothing waits here
    auto issue_loads = [&](int tile) __attribute__((always_inline)) {
      const StemTile t = stem_tile(p, tile);
      if constexpr (U8) {
        u8w.border = !t.interior;
        if (has_block) u8_gather_rows(rs_x, p, t, row, g_rel, u8w);
      } else {
        if (has_block) xfix = mx_gather_rows(rs_x, p, t, row, g_rel, fresh_lane_id() >> 5, xv);
      }
    };
    // the gathered window as (hi, lo) B fragments, kept for both passes of the tile
    bf16x8_t xh[2], xl[2];
    auto convert = [&]() __attribute__((always_inline)) {
      if (!has_block) return;
      if constexpr (U8) u8_convert(p, u8w, ka, kb, fresh_lane_id() >> 5, xv);
      else mx_edge_fix(xv, xfix);
      x3_split_window(xv, xh, xl);
    };
    // conv1_1 of channel half h on the converted window, bias + clamp + half-line packing, halo lines -> LDS
    auto produce = [&](int tile, auto h_c, char* buf) __attribute__((always_inline)) {
      constexpr int h = decltype(h_c)::value;
      if (!has_block) return;  // wave-uniform
      const StemTile t = stem_tile(p, tile);
      f32x16_t acc;
      stem_bias16(bias_l + 32 * h, 4, acc);
      acc = conv1_1_sextet(wh[h], wlo[h], xh[0], xh[1], xl[0], xl[1], acc);
      stem_restore_prio(pprio);
      MxHalfLine L;
      mx_clamp_pack_half(acc, stem_halo_pixel_in_image(p, t, row), L, range_seen);
      if (row >= ST_HALO_PX) return;   // (block 10 has 12 surplus lanes)
      mx_write_half_line(buf + row * 128, g_swz, fresh_lane_id() >> 5, L);   // (a fresh lane half: see fresh_lane_id)
    };

    // stage s = (tile s >> 1, channel half s & 1) goes to halo buffer s & 1; the producers run one
    // stage ahead of the consumers, the gathers one tile ahead of that
    using H0 = std::integral_constant<int, 0>;
    using H1 = std::integral_constant<int, 1>;
    const bool prof = p.prof != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && wave == 4;
    unsigned long long pt[4] = {0, 0, 0, 0};   // work, wait; of which in the stage beside the consumers' pass 0
    auto hand_over = [&](unsigned long long t0, int stage = 1) __attribute__((always_inline)) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const unsigned long long t1 = prof ? __builtin_amdgcn_s_memtime() : 0;
      __builtin_amdgcn_s_barrier();
      if (prof) {
        const unsigned long long t2 = __builtin_amdgcn_s_memtime();
        pt[0] += t1 - t0;
        pt[1] += t2 - t1;
        if (stage == 0) {
          pt[2] += t1 - t0;
          pt[3] += t2 - t1;
        }
      }
    };
    if (niter > 0) {
      issue_loads(first);
      convert();
      if (niter > 1) issue_loads(first + stride);
      produce(first, H0{}, hb);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int it = 0; it < niter; ++it) {
      // S1: the tile's second channel half into buffer 1 (last read in S4 of the previous tile)
      unsigned long long t0 = prof ? __builtin_amdgcn_s_memtime() : 0;
      produce(first + it * stride, H1{}, hb + ST_HALO_BYTES);
      hand_over(t0, 0);
      // S2: the tile's fragments are no longer needed — the window of tile it+1 (it has had a whole tile to
      // arrive) is converted and the gathers of tile it+2 go out
      t0 = prof ? __builtin_amdgcn_s_memtime() : 0;
      if (it + 1 < niter) {
        convert();
        if (it + 2 < niter) issue_loads(first + (it + 2) * stride);
      }
      hand_over(t0);
      // S3: nothing (buffer 0 is still read)
      t0 = prof ? __builtin_amdgcn_s_memtime() : 0;
      hand_over(t0);
      // S4: the first channel half of the next tile into buffer 0 (last read in S3)
      t0 = prof ? __builtin_amdgcn_s_memtime() : 0;
      if (it + 1 < niter) produce(first + (it + 1) * stride, H0{}, hb);
      hand_over(t0);
    }
    if (prof && lane == 0) {
      p.prof[4] = pt[0];
      p.prof[5] = pt[1];
      p.prof[6] = pt[2];
      p.prof[7] = pt[3];
    }
    mx_raise_if_out_of_range(range_seen, p.range_flag);
    return;
  }

  // ================================== consumers ================================================
  typedef stem_u4 u4;
  stem_raise_prio((p.prod_prio >> 2) & 3);   // test hook: the consumers' issue priority
  // conv1_2's weights: LDS row (h * 9 + tap) * 32 + m = the f16mx line of output channel co0 + chan(m),
  // input group h; 16-byte slots swizzled by (m >> 1) & 7
  const int wpiece = ((lane & 7) ^ (4 * (wave & 1) + (lane >> 4))) * 16;
  const __amdgpu_buffer_rsrc_t rs_w2 =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p.w2), 0, 9 * 64 * 256, 0x00020000);
  // the 36 KB image (output-channel half c, input half h) into weight buffer `buf`: nine LDS-DMA
  // instructions per consumer wave (buffer loads: the compiler counts them in vmcnt only — a global_load_lds it has
  // not seen waited for turns every counted lgkmcnt of the pass into lgkmcnt(0))
  auto stream_w = [&](int c, int h, int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int q = j * 4 + wave;
      const int r = q * 8 + (lane >> 3);
      const int tap = r >> 5, m = r & 31;
      const int ch = 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3);
      buf_glds16(rs_w2, (unsigned)((tap * 64 + 32 * c + ch) * 256 + h * 128 + wpiece), 0u,
                 wl + buf * (9 * 32 * 128) + q * 1024);
    }
  };
  stream_w(0, 0, 0);
  // Pixel (B) fragments (stem_pixel_addressing): lane (pixel l31 of block i, k-half hc)
  // reads fp16 slot 2 s + hc for the two f16 MFMAs and — the B side of the scaled MFMA pairs q6(lo) with
  // the weights' q6(hi) in K-block 0 and the other way round in block 1 — slots 5 - hc / 7 - hc: all of
  // them (e_kx ^ const) + pc, the constants 0, 32, 80, 112 (^ 64 on odd tap rows).
  int e_kx[3], pxb;
  stem_pixel_addressing(wave, half, l31, e_kx, pxb);
  int w_base = mx_weight_row(half, l31);
  auto w_off = [&](int kk) __attribute__((always_inline)) { return w_base ^ (kk << 5); };
  // (the builtin, not inline asm: the compiler models a pending global_load_lds as a FLAT access and turns
  //  every later lgkmcnt wait into lgkmcnt(0) until IT has seen vmcnt(0))
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
  __builtin_amdgcn_s_barrier();
  const bool cprof = p.prof != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && wave == 0;
  unsigned long long ct[3] = {0, 0, 0}, ct0w = 0;
  f32x16_t acc[2];
  // operand registers, single-buffered: a fragment is reloaded for the next tap right behind the last
  // MFMA that reads it, and the MFMA order (w0.b0, w0.b1, w1.b0, w1.b1, wm.b0, wm.b1 — accumulators
  // alternate) leaves every reload at least four MFMAs (128 cycles) before its first use.  The MX operand's
  // tail is read as ONE ds_read_b128 (mx_scaled_mfma).
  f16x8_t w0, w1, b0[2], b1[2];
  u4 wma, bma[2];
  u4 wmt, bmt[2];
  // (nc, nh) = the stage after this one (nc < 0: none): its weight image streams into the buffer this pass
  // does not read (the previous stage's, handed back behind that stage's barrier)
  auto run_pass = [&](auto h_c, int nc, int nh) __attribute__((always_inline)) {
    constexpr int h = decltype(h_c)::value;
    const unsigned long long c0 = cprof ? __builtin_amdgcn_s_memtime() : 0;
    if (nc >= 0) stream_w(nc, nh, h ^ 1);
    const int pc = pxb + S3_W_BYTES + h * ST_HALO_BYTES;
    if (h == 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    }
    auto paddr = [&](int tap, int part) __attribute__((always_inline)) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      const int c = (part == 0 ? 0 : part == 1 ? 32 : part == 2 ? 80 : 112) ^ ((ky & 1) << 6);
      int a;
      asm("v_xad_u32 %0, %1, %2, %3" : "=v"(a) : "v"(e_kx[kx]), "s"(c), "v"(pc));
      return a;
    };
    auto pbase = [&](int tap, int i) __attribute__((always_inline)) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      return smem + (ky * C64_HW + kx) * 128 + i * 2048;
    };
    auto ld_b0 = [&](int tap, int i, int a) __attribute__((always_inline)) { b0[i] = *reinterpret_cast<const f16x8_t*>(pbase(tap, i) + a); };
    auto ld_b1 = [&](int tap, int i, int a) __attribute__((always_inline)) { b1[i] = *reinterpret_cast<const f16x8_t*>(pbase(tap, i) + a); };
    auto ld_tail = [&](const char* a) __attribute__((always_inline)) -> u4 { return *reinterpret_cast<const u4*>(a); };
    auto ld_bm = [&](int tap, int i, int a2, int a3) __attribute__((always_inline)) {
      bma[i] = *reinterpret_cast<const u4*>(pbase(tap, i) + a2);
      bmt[i] = ld_tail(pbase(tap, i) + a3);
    };
    auto ld_w0 = [&](int tap) __attribute__((always_inline)) { w0 = *reinterpret_cast<const f16x8_t*>(smem + tap * 4096 + w_off(0)); };
    auto ld_w1 = [&](int tap) __attribute__((always_inline)) { w1 = *reinterpret_cast<const f16x8_t*>(smem + tap * 4096 + w_off(1)); };
    auto ld_wm = [&](int tap) __attribute__((always_inline)) {
      wma = *reinterpret_cast<const u4*>(smem + tap * 4096 + w_off(2));
      wmt = ld_tail(smem + tap * 4096 + w_off(3));
    };
    auto mx = [&](int i) __attribute__((always_inline)) { acc[i] = mx_scaled_mfma(wma, wmt, bma[i], bmt[i], acc[i]); };
    {
      const int a0 = paddr(0, 0), a1 = paddr(0, 1), a2 = paddr(0, 2), a3 = paddr(0, 3);
      ld_w0(0);
      ld_b0(0, 0, a0);
      ld_b0(0, 1, a0);
      ld_w1(0);
      ld_b1(0, 0, a1);
      ld_b1(0, 1, a1);
      ld_wm(0);
      ld_bm(0, 0, a2, a3);
      ld_bm(0, 1, a2, a3);
    }
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      // (sched_barrier: the order below IS the schedule — left alone, the scheduler sinks every reload to
      //  just in front of its use, for register pressure it does not have, and waits lgkmcnt(0) per MFMA)
      const bool more = tap + 1 < 9;
      const int n = tap + 1;
      int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
      __builtin_amdgcn_sched_barrier(0);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w0, b0[0], acc[0], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (tap > 0) ld_wm(tap);   // (not behind the previous tap's last MFMA: 15 reads in flight there, and the
                                 //  compiler answers a full lgkmcnt counter with lgkmcnt(0))
      if (more) {
        a0 = paddr(n, 0);
        ld_b0(n, 0, a0);
      }
      __builtin_amdgcn_sched_barrier(0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w0, b0[1], acc[1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (more) {
        ld_w0(n);
        ld_b0(n, 1, a0);
      }
      __builtin_amdgcn_sched_barrier(0);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1, b1[0], acc[0], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (more) {
        a1 = paddr(n, 1);
        ld_b1(n, 0, a1);
      }
      __builtin_amdgcn_sched_barrier(0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1, b1[1], acc[1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (more) {
        ld_w1(n);
        ld_b1(n, 1, a1);
      }
      __builtin_amdgcn_sched_barrier(0);
      mx(0);
      __builtin_amdgcn_sched_barrier(0);
      if (more) {
        a2 = paddr(n, 2);
        a3 = paddr(n, 3);
        ld_bm(n, 0, a2, a3);
      }
      __builtin_amdgcn_sched_barrier(0);
      mx(1);
      __builtin_amdgcn_sched_barrier(0);
      if (more) ld_bm(n, 1, a2, a3);
    }
    // every fragment read of this halo buffer has been consumed: hand it back (and the next stage's weight image
    // has landed — it has had the whole pass)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wait_vmcnt<0>();
    const unsigned long long c1 = cprof ? __builtin_amdgcn_s_memtime() : 0;
    __builtin_amdgcn_s_barrier();
    if (cprof) {
      const unsigned long long c2 = __builtin_amdgcn_s_memtime();
      ct[0] += c1 - c0;
      ct[1] += c2 - c1;
      if (h == 0) ct0w += c2 - c1;
    }
    w_base += h == 0 ? 9 * 32 * 128 : -(9 * 32 * 128);     // (a multiple of 4096: the slot bits stay)
  };
  using C0 = std::integral_constant<int, 0>;
  using C1 = std::integral_constant<int, 1>;
#pragma unroll 1
  for (int itc = 0; itc < niter * 2; ++itc) {   // (tile it, output-channel half cz)
    const int it = itc >> 1, cz = itc & 1;
    // S1 / S3 stream the image of S2 / S4 (same output half, input half 1); S2 streams (half 1, input 0); S4 the
    // next tile's (half 0, input 0)
    run_pass(C0{}, cz, 1);
    run_pass(C1{}, (cz == 0 || it + 1 < niter) ? (cz ^ 1) : -1, 0);
    const unsigned long long e0 = cprof ? __builtin_amdgcn_s_memtime() : 0;
    const int lane_e = fresh_lane_id();
    const int half = lane_e >> 5, l31 = lane_e & 31;   // (shadow the kernel's: nothing lane-derived stays live across the passes)
    const float* const bias2 = reinterpret_cast<const float*>(smem + S3_BIAS_OFF) + 64 + 32 * cz + 16 * half;
    int n, ty, tx;
    stem_decode(p, first + it * stride, n, ty, tx);
    const int oy = ty * 4 + wave;
    const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(
        p.out + ((long)n * Ho + oy) * Wo * 256, 0, oy < Ho ? Wo * 256 : 0, 0x00020000);
    mx_pooled_epilogue(acc[0], acc[1], bias2, 65504.f, 0u, rs_o, tx, cz, half, l31, range_seen);
    if (cprof) ct[2] += __builtin_amdgcn_s_memtime() - e0;
  }
  if (cprof && lane == 0) {
    p.prof[0] = ct[0];
    p.prof[1] = ct[1];
    p.prof[2] = ct[2];
    p.prof[3] = ct0w;   // of the waits: behind pass 0
  }
  mx_raise_if_out_of_range(range_seen, p.range_flag);
}
