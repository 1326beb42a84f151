// vgg_stem_x3_kernel<U8>: the fused bf16x3 stem (included by stem.hip inside namespace oibl, behind stem_parts.h;
// launched by launch_vgg_stem_x3).
// ---------------------------------------------------------------------------------------------
// VGG stem, fused, bf16x3: conv1_1 + ReLU + conv1_2 + ReLU + 2x2 max-pool in ONE launch.
//   x [N][3][H][W] fp32  ->  out [N][H/2][W/2][64] bf16x3 ((hi, lo) groups)
// Unfused, conv1_1 writes 2.5 GB of split activations per 32 images (0.86 ms, write-bound) and
// conv1_2 — Cout = 64: no ring tile shape — runs on the generic core at 45 % of the matrix pipe
// (2.5 ms): 22 % of the bf16x3 step for 13 % of its FLOPs.  The bf16 stem's plan (72 KiB of
// conv1_2 weights + two 42.5 KiB halo buffers of all 64 channels) does not survive 4-byte
// elements; this kernel keeps its producer / consumer structure and splits the work so that it does:
//   * a workgroup serves HALF of conv1_2's output channels (blockIdx.y = 0 / 1; both halves run
//     at the same time on different CUs and gather the same input window through L2): 9 taps x 2
//     channel halves x 32 cout x 128 B = 72 KiB of split weights stay resident in LDS;
//   * a tile is consumed in two PASSES, one per half of conv1_2's input channels: a halo buffer holds
//     340 pixels x [32 hi | 32 lo] of ONE 32-channel half (42.5 KiB, exactly the bf16 stem's buffer)
//     and the two buffers alternate between the passes.  Producers (waves 4-15) run conv1_1 for the
//     32 channels of the next pass (K = 27 padded to 32: lo.hi + hi.lo + hi.hi, 6 MFMAs per 32 halo
//     pixels; twelve waves, one 32-pixel block of the halo each), ReLU, split, and write the halo
//     image the consumers read; the gathered input window
//     and its (hi, lo) fragments are kept in registers for both passes of a tile.  Consumers (waves
//     0-3) accumulate both passes in registers (9 taps x 12 MFMAs per pass), then pool and store.
// Only 4 waves read LDS for the main contraction (the generic kernel has 16 competing for it).
// Numerics: operation for operation those of conv1_1_mfma_kernel<X3> followed by the generic
// bf16x3 convolution in K order (channel chunk, tap) — bit-identical to that pair (tested).
// LDS: 72 KiB + 2 x 42.5 KiB = 157 KiB.
// U8 = true: the input is the raw uint8 NHWC image, gathered and normalised by the producers (stem_parts.h, "uint8 input").
// ---------------------------------------------------------------------------------------------
template <bool U8>
__global__ __launch_bounds__(1024) void vgg_stem_x3_kernel(StemParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const wl = smem;                 // [pass h][tap][32 cout][32 hi | 32 lo of input channels 32h..]
  char* const hb = smem + S3_W_BYTES;    // halo buffer h: channels 32h..32h+31 of the current tile
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const StemTiles tiles = stem_xcd_tiles(p.ntiles);
  const int first = tiles.first, stride = tiles.stride, niter = tiles.niter;
  const int co0 = blockIdx.y * 32;       // this workgroup's conv1_2 output channels
  const int Ho = p.H >> 1, Wo = p.W >> 1;
  stem_bias_to_lds(smem, p.b1, nullptr, 1.f);

  if (wave >= 4) {
    // ================================ producers (waves 4-15) ====================================
    // Twelve producer waves (three per SIMD, one 32-pixel block each) against four consumers: with one
    // producer wave per SIMD handling three blocks, the VALU-heavy role (two splits per value, ~1400
    // dependent VALU instructions per tile at ~8 cycles each) was 1.7x the consumers' time; three
    // waves per SIMD hide each other's instruction latency.  The kernel therefore runs 16 waves per
    // workgroup at <= 128 VGPRs.  prod_prio (test hook) sets the roles' issue priorities (producers:
    // outside their MFMAs, which always go out at priority 3).  Measured (tests/gpu_stem3_prof.py):
    // every setting lands within 5 % — skewed priorities save shader cycles per tile (10.6k vs
    // 12.9k), the chip answers with a lower clock and the wall time is 2.07-2.19 ms either way; equal
    // priorities (the default, 0 / 0) are the fastest.
    const int pprio = p.prod_prio & 3;
    stem_raise_prio(pprio);
    const int pw = wave - 4;   // 0..11: producer wave pw owns block pw of the 11 (wave 15 only keeps step)
    const bool has_block = pw < ST_BLOCKS;
    const __amdgpu_buffer_rsrc_t rs_x =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, (int)p.x_bytes, 0x00020000);
    bf16x8_t wh[2][2], wlo[2][2];
    stem_w1_fragments<U8 ? K_BYTES : K_WINDOW, false>(p.w1, 1.f, half, l31, wh, wlo);
    // accumulator rows of this lane: channels 8 j + 4 half + 0..3 (j = 0..3) of the pass's 32
    const float* const bias_l = reinterpret_cast<const float*>(smem + S3_BIAS_OFF) + 4 * half;
    const int plane = p.H * p.W;

    // tile-independent lane geometry (as in vgg_stem_kernel): the halo pixel of this lane is r = 32 pw + l31; kept:
    // the swizzle of its LDS row and its element offset from the tile's halo origin (the rest is recomputed where needed)
    const int row = 32 * pw + l31;
    int g_swz, g_rel;
    {
      int hy, hx;
      stem_halo_yx(row, hy, hx);
      g_swz = c64_swz(hy, hx);
      g_rel = hy * p.W + hx;
      asm volatile("" : "+v"(g_rel));
    }
    // element offset of input element k(j) from the pixel, j = 8 s + e, k = 16 s + 8 half + e (slots
    // with k >= 27 carry zero weights and re-read a valid tap): wave-uniform per lane half, so the two
    // candidates stay in scalar registers and a lane selects (no 16 VGPRs per lane)
    auto dk_of = [&](int j) __attribute__((always_inline)) {
      const int kA = 16 * (j >> 3) + (j & 7), kB = kA + 8 >= 27 ? kA : kA + 8;
      const int oA = (kA / 9) * plane + ((kA % 9) / 3 - 1) * p.W + ((kA % 9) % 3 - 1);
      const int oB = (kB / 9) * plane + ((kB % 9) / 3 - 1) * p.W + ((kB % 9) % 3 - 1);
      int hsel = half;
      asm volatile("" : "+v"(hsel));   // not loop-invariant for the compiler: no 16 hoisted VGPRs
      return hsel ? oB : oA;
    };
    auto tap_of = [&](int j) __attribute__((always_inline)) {  // border tiles only
      const int kA = 16 * (j >> 3) + (j & 7), kB = kA + 8 >= 27 ? kA : kA + 8;
      return half ? kB % 9 : kA % 9;
    };
    float xv[16];
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
        if (!has_block) return;  // wave-uniform
        const int base = ((t.n * 3) * p.H + t.y0) * p.W + t.x0 + g_rel;
        if (t.interior) {
#pragma unroll
          for (int j = 0; j < 16; ++j)
            xv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_x, (base + dk_of(j)) * 4, 0, 0));
        } else {
          int hy, hx;
          stem_halo_yx(row, hy, hx);
          const int y = t.y0 + hy, x = t.x0 + hx;
          unsigned mk = 0;
          if (y >= 0 && y < p.H && x >= 0 && x < p.W) {
            const bool ya = y > 0, yc = y + 1 < p.H, xa = x > 0, xc = x + 1 < p.W;
            mk = (ya && xa ? 1u : 0u) | (ya ? 2u : 0u) | (ya && xc ? 4u : 0u) | (xa ? 8u : 0u) | 16u |
                 (xc ? 32u : 0u) | (yc && xa ? 64u : 0u) | (yc ? 128u : 0u) | (yc && xc ? 256u : 0u);
          }
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const bool ok = (mk >> tap_of(j)) & 1u;
            const unsigned off = ok ? (unsigned)(base + dk_of(j)) * 4u : ST_OOB;
            xv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_x, (int)off, 0, 0));
          }
        }
      }
    };
    // the gathered window as (hi, lo) B fragments, kept for both passes of the tile
    bf16x8_t xh[2], xl[2];
    auto convert = [&]() __attribute__((always_inline)) {
      if (!has_block) return;
      if constexpr (U8) u8_convert(p, u8w, ka, kb, fresh_lane_id() >> 5, xv);
      x3_split_window(xv, xh, xl);
    };
    // conv1_1 of channel half h on the converted window, bias + ReLU + split, halo tile -> LDS
    auto produce = [&](int tile, auto h_c, char* buf) __attribute__((always_inline)) {
      constexpr int h = decltype(h_c)::value;
      if (!has_block) return;  // wave-uniform
      const StemTile t = stem_tile(p, tile);
      f32x16_t acc;
      stem_bias16(bias_l + 32 * h, 8, acc);
      acc = conv1_1_sextet(wh[h], wlo[h], xh[0], xh[1], xl[0], xl[1], acc);
      stem_restore_prio(pprio);
      // D[row = channel][col = pixel]: registers 4g..4g+3 = channels 8 g + 4 half + 0..3 of the
      // lane's pixel -> hi: 8 bytes of 16-B slot g, lo: of slot 4 + g (both swizzled), + 8 half.
      const bool pix_ok = stem_halo_pixel_in_image(p, t, row);
      if (row < ST_HALO_PX) {
        char* line = buf + row * 128 + 8 * half;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          uint2 hi, lo;
          ring_split4(fmaxf(acc[4 * g], 0.f), fmaxf(acc[4 * g + 1], 0.f), fmaxf(acc[4 * g + 2], 0.f),
                      fmaxf(acc[4 * g + 3], 0.f), hi, lo);
          if (!pix_ok) {   // outside the image: conv1_2's zero padding, not a conv1_1 output
            hi = make_uint2(0u, 0u);
            lo = make_uint2(0u, 0u);
          }
          *reinterpret_cast<uint2*>(line + ((g ^ g_swz) << 4)) = hi;
          *reinterpret_cast<uint2*>(line + (((4 + g) ^ g_swz) << 4)) = lo;
        }
      }
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
      // while the consumers run pass 0 of tile it: its second channel half; then — its fragments
      // are no longer needed — the window of tile it+1 (it has had a whole tile to arrive) is
      // converted and the gathers of tile it+2 go out
      unsigned long long t0 = prof ? __builtin_amdgcn_s_memtime() : 0;
      produce(first + it * stride, H1{}, hb + ST_HALO_BYTES);
      if (it + 1 < niter) {
        convert();
        if (it + 2 < niter) issue_loads(first + (it + 2) * stride);
      }
      hand_over(t0, 0);
      // while they run pass 1: the first channel half of the next tile.  (Computing and packing it beside pass 0
      // and only writing it here was measured: 1.66 instead of 1.54 ms — that stage already carries the
      // consumers' epilogue and is bound by what the four waves of a SIMD can issue.)
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
    return;
  }

  // ================================== consumers ================================================
  stem_raise_prio((p.prod_prio >> 2) & 3);   // test hook: the consumers' issue priority
  {
    const int piece = ((lane & 7) ^ (4 * (wave & 1) + (lane >> 4))) * 16;
#pragma unroll
    for (int j = 0; j < 18; ++j) {
      const int q = j * 4 + wave;
      const int r = q * 8 + (lane >> 3);          // LDS row: (h * 9 + tap) * 32 + c
      const int h = r / 288, rem = r - 288 * h;
      const int tap = rem >> 5, c = rem & 31;
      glds16(p.w2 + ((long)(tap * 64 + co0 + c) * 256 + h * 128) + piece, wl + q * 1024);
    }
  }
  int e_kx[3], pxb;   // pixel-fragment addressing: stem_parts.h
  stem_pixel_addressing(wave, half, l31, e_kx, pxb);
  int w_off[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) w_off[kk] = l31 * 128 + (((2 * kk + half) ^ ((l31 >> 1) & 7)) << 4);
  const float bval = p.b2[co0 + l31];

  // The pooled outputs of tile i are held back and stored one pixel at a time between the matrix
  // steps of tile i+1.  A pending pixel is ONE dword per lane: lanes l31 and l31 ^ 1 exchange halves
  // (DPP + v_perm), the even lane stores the hi parts of channels (l31, l31 + 1), the odd lane the lo
  // parts of (l31 - 1, l31) — a half-wave writes the full 128-byte line of its pixel.  The store is a
  // buffer store into ONE OUTPUT ROW of the map (descriptor rebuilt per tile from scalars, zero
  // records for a row below the map): a pixel right of the map is out of range and dropped by the
  // hardware, the pixel's distance is the instruction's immediate — no mask, no compare, no branch,
  // so a pass stays one basic block and the scheduler can place the fragment reads freely.
  uint32_t pend[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) pend[e] = 0;
  __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, 0, 0x00020000);  // nothing pending
  const unsigned lane_off =
      blockIdx.y * 128 + half * 256 + ((l31 & 1) ? 64 + (l31 - 1) * 2 : l31 * 2);
  unsigned poff = lane_off;
  auto store_px = [&](int e) __attribute__((always_inline)) {
    __builtin_amdgcn_raw_buffer_store_b32(pend[e], rs_o, (int)(poff + 512u * e), 0, 0);
  };
  // (the builtin, not inline asm: the compiler models a pending global_load_lds as a FLAT access and turns
  //  every later lgkmcnt wait into lgkmcnt(0) until IT has seen vmcnt(0))
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
  __builtin_amdgcn_s_barrier();
  const bool cprof = p.prof != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && wave == 0;
  unsigned long long ct[3] = {0, 0, 0};
  f32x16_t acc[2];
  // one pass = 18 steps (tap, 16-wide half pr of the K-tile) over channel half h of the halo
  auto run_pass = [&](auto h_c) __attribute__((always_inline)) {
    constexpr int h = decltype(h_c)::value;
    const unsigned long long c0 = cprof ? __builtin_amdgcn_s_memtime() : 0;
    // LDS addresses beyond the 16-bit immediate of a DS instruction live in the base registers:
    // pc = this lane's pixel in halo buffer h, w_off[] = its weight row in pass h's weight image
    const int pc = pxb + S3_W_BYTES + h * ST_HALO_BYTES;
    if (h == 0) {
      float b = bval;
      asm volatile("" : "+v"(b));   // per pass: a hoisted 16-register splat would be spilled
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = b;
    }
    bf16x8_t fah[2][2], fal[2][2], fbh[2], fbl[2];
    auto load_step = [&](int sidx, bf16x8_t (&ah)[2], bf16x8_t (&al)[2], bf16x8_t& bh, bf16x8_t& bl)
        __attribute__((always_inline)) {
      const int tap = sidx >> 1, pr = sidx & 1;
      const int ky = tap / 3, kx = tap - 3 * ky;
      const int c = (pr << 5) ^ ((ky & 1) << 6);   // hi chunk; the lo chunk sits 4 slots on
      int a_hi, a_lo;
      asm("v_xad_u32 %0, %1, %2, %3" : "=v"(a_hi) : "v"(e_kx[kx]), "s"(c), "v"(pc));
      asm("v_xad_u32 %0, %1, %2, %3" : "=v"(a_lo) : "v"(e_kx[kx]), "s"(c ^ 64), "v"(pc));
      const char* px = smem + (ky * C64_HW + kx) * 128;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ah[i] = *reinterpret_cast<const bf16x8_t*>(px + i * 2048 + a_hi);
        al[i] = *reinterpret_cast<const bf16x8_t*>(px + i * 2048 + a_lo);
      }
      bh = *reinterpret_cast<const bf16x8_t*>(smem + tap * 4096 + w_off[pr]);
      bl = *reinterpret_cast<const bf16x8_t*>(smem + tap * 4096 + w_off[pr + 2]);
    };
    load_step(0, fah[0], fal[0], fbh[0], fbl[0]);
#pragma unroll
    for (int sidx = 0; sidx < 18; ++sidx) {
      const int b = sidx & 1;
      if (sidx + 1 < 18) load_step(sidx + 1, fah[b ^ 1], fal[b ^ 1], fbh[b ^ 1], fbl[b ^ 1]);
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fal[b][i], fbh[b], acc[i], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah[b][i], fbl[b], acc[i], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah[b][i], fbh[b], acc[i], 0, 0, 0);
      if (h == 0 && (sidx & 1) == 1 && (sidx >> 1) < 8) store_px(sidx >> 1);
      if (sidx + 1 < 18) {
        // the six fragment reads of step sidx+1 (and their two address instructions) go out one per
        // MFMA of this step: a full step of latency cover, no read burst in front of the matrix pipe
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          if (q < 2) __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          if (q == 3 && h == 0 && (sidx & 1) == 1 && (sidx >> 1) < 8)
            __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);   // this step's pending-pixel store
        }
      }
    }
    // every fragment read of this halo buffer has been consumed by the MFMAs above: hand it back
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const unsigned long long c1 = cprof ? __builtin_amdgcn_s_memtime() : 0;
    __builtin_amdgcn_s_barrier();
    if (cprof) {
      ct[0] += c1 - c0;
      ct[1] += __builtin_amdgcn_s_memtime() - c1;
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) w_off[kk] += h == 0 ? 9 * 32 * 128 : -(9 * 32 * 128);   // the other pass's image
  };
  using C0 = std::integral_constant<int, 0>;
  using C1 = std::integral_constant<int, 1>;
  const uint32_t psel = (l31 & 1) ? 0x03020706u : 0x05040100u;
  for (int it = 0; it < niter; ++it) {
    run_pass(C0{});
    run_pass(C1{});
    // pool, split, pair up: the tile's eight pixels of this lane become pending
    int n, ty, tx;
    stem_decode(p, first + it * stride, n, ty, tx);
    const int oy = ty * 4 + wave;
    rs_o = __builtin_amdgcn_make_buffer_rsrc(p.out + ((long)n * Ho + oy) * Wo * 256, 0,
                                             oy < Ho ? Wo * 256 : 0, 0x00020000);
    poff = lane_off + (unsigned)tx * (16 * 256);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float v = fmaxf(fmaxf(fmaxf(acc[i][4 * g], acc[i][4 * g + 1]),
                                    fmaxf(acc[i][4 * g + 2], acc[i][4 * g + 3])), 0.f);
        uint16_t hi, lo;
        x3_split(v, hi, lo);
        const uint32_t mine = (uint32_t)hi | ((uint32_t)lo << 16);
        const uint32_t other = (uint32_t)__builtin_amdgcn_mov_dpp((int)mine, 0xB1, 0xF, 0xF, true);  // lane ^ 1
        pend[4 * i + g] = __builtin_amdgcn_perm(other, mine, psel);
      }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) store_px(e);
  if (cprof && lane == 0) {
    p.prof[0] = ct[0];
    p.prof[1] = ct[1];
    p.prof[2] = 0;
  }
}
