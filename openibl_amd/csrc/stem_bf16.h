// vgg_stem_kernel<U8>: the fused bf16 stem (included by stem.hip inside namespace oibl, behind conv_c64.h and
// stem_parts.h; launched by launch_vgg_stem).

// ---------------------------------------------------------------------------------------------
// VGG stem, fused (bf16): conv1_1 + ReLU + conv1_2 + ReLU + 2x2 max-pool in ONE launch.
//   x [N][3][H][W] fp32  ->  out [N][H/2][W/2][64] bf16
// Unfused, conv1_1 writes its 64-channel output (39 MB / image) to HBM only for conv1_2 to read it
// straight back: together 23 % of the step for 12.6 % of its FLOPs.  Here the conv1_1 activations
// never leave the CU.  A persistent workgroup of 8 waves is split by role (waves w and w + 4 share
// a SIMD, so every SIMD hosts one wave of each role):
//   producers (waves 4-7): for the NEXT 8 x 32 output tile, gather the 3-channel input window of
//     the (8+2) x (32+2) halo straight from global memory (coalesced dword buffer loads, an
//     out-of-image tap is an out-of-range offset -> 0), run conv1_1 on the matrix cores (K = 27
//     padded to 32, transposed GEMM as in conv1_1_mfma_kernel: 4 MFMAs per 32 halo pixels),
//     bias + ReLU + bf16, and write the halo tile into LDS in exactly the swizzled image the
//     conv1_2 main loop reads (halo pixels outside the image are written as zeros: conv1_2's
//     padding);
//   consumers (waves 0-3): the conv3x3_c64_kernel main loop (resident conv1_2 weights, 144 MFMAs
//     per wave per tile out of LDS), pool in registers, store the pooled pixels directly.
// One raw s_barrier per tile hands the halo buffers over (two buffers, producer one tile ahead).
// Numerics are those of the unfused bf16 path, operation for operation (same MFMA k order, same
// rounding points) -> bit-identical output.
// LDS: 72 KiB conv1_2 weights + 2 x 42.5 KiB halo = 157 KiB.
// ---------------------------------------------------------------------------------------------
constexpr int ST_LDS_BYTES = C64_W_BYTES + 2 * ST_HALO_BYTES;
constexpr int ST_LUT_ENTRIES = 3 * 257;              // uint8 input: per channel 256 values + "0.0"
constexpr int ST_LDS_BYTES_U8 = ST_LDS_BYTES + 1552;
// U8 = true: the input is the loader's raw uint8 NHWC image; ToTensor + Normalize
// (ibl/utils/data/__init__.py:40-41: (u / 255 - mean) / std in fp32) followed by the bf16 rounding
// of the operand is a pure function of (channel, byte), so the producers look it up in a 3 x 257
// table built in LDS at kernel start with exactly that arithmetic (entry 256 = 0.0: conv1_1's
// zero padding) — bit-identical to feeding the normalised fp32 tensor, a quarter of the bytes.
template <bool U8>
__global__ __launch_bounds__(512) void vgg_stem_kernel(StemParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const wl = smem;
  char* const hb = smem + C64_W_BYTES;
  const uint16_t* const lut = reinterpret_cast<const uint16_t*>(smem + ST_LDS_BYTES);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const int first = blockIdx.x, stride = gridDim.x;
  int niter = 0;
  if (first < p.ntiles) niter = (p.ntiles - first + stride - 1) / stride;
  const int Ho = p.H >> 1, Wo = p.W >> 1;
  if constexpr (U8) {
    uint16_t* lw = reinterpret_cast<uint16_t*>(smem + ST_LDS_BYTES);
    for (int i = threadIdx.x; i < ST_LUT_ENTRIES; i += 512) {
      const int c = i / 257, u = i - 257 * c;
      const float q = (float)u / 255.0f;
      lw[i] = u == 256 ? (uint16_t)0 : f32_to_bf16_bits((q - p.mean[c]) / p.stdv[c]);
    }
    __syncthreads();
  }

  if (wave >= 4) {
    // ================================ producers ================================================
    const int pw = wave - 4;
    // The consumer wave on this SIMD keeps the matrix pipe saturated and, being the older wave,
    // wins every arbitration: without a raised priority the producer's dozen MFMAs per tile only
    // issue once the consumer's loop has ended and the two roles serialise.  The priority is
    // raised around the MFMAs only; everything else in this role runs in the consumer's shadow.
    const __amdgpu_buffer_rsrc_t rs_x =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.x), 0, (int)p.x_bytes, 0x00020000);
    // conv1_1 weights as the A operand: wf[t][s] element e <-> cout = 32 t + l31, k = 16 s + 8 half + e
    bf16x8_t wf[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = 16 * s + 8 * half + e;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const float v = k < 27 ? p.w1[(32 * t + l31) * 27 + k] : 0.f;
          wf[t][s][e] = (short)f32_to_bf16_bits(v);
        }
      }
    float bb[2][16];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) bb[t][r] = p.b1[32 * t + acc_row(r, lane)];
    const int plane = p.H * p.W;

    // Tile-independent lane geometry.  Block b of this wave covers halo pixels r = 32 b + l31
    // (clamped to the last pixel for the 12 surplus lanes of block 10: they load valid data that is
    // never written).  g_rel = element offset of the pixel from the tile's halo origin, g_dk[j] =
    // element offset of input element k(j) from the pixel (j = 8 s + e, k = 16 s + 8 half + e;
    // slots with k >= 27 carry zero weights and simply re-read a valid tap of the same window).
    int g_row[3], g_swz[3], g_hy[3], g_hx[3], g_rel[3];
#pragma unroll
    for (int bi = 0; bi < 3; ++bi) {
      const int r = 32 * (pw + 4 * bi) + l31;
      const int rc = r < ST_HALO_PX ? r : ST_HALO_PX - 1;
      g_row[bi] = r;
      g_hy[bi] = rc / C64_HW;
      g_hx[bi] = rc - g_hy[bi] * C64_HW;
      g_swz[bi] = c64_swz(g_hy[bi], g_hx[bi]);
      g_rel[bi] = (g_hy[bi] * p.W + g_hx[bi]) * (U8 ? 3 : 1);
      asm volatile("" : "+v"(g_rel[bi]));
    }
    int g_dk[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      int k = 16 * (j >> 3) + 8 * half + (j & 7);
      if (k >= 27) k -= 8;
      const int c = k / 9, t = k - 9 * c;
      g_dk[j] = U8 ? ((t / 3 - 1) * p.W + (t % 3 - 1)) * 3 + c
                   : c * plane + (t / 3 - 1) * p.W + (t % 3 - 1);
      asm volatile("" : "+v"(g_dk[j]));  // keep it in a register: re-deriving it costs a v_mul per load
    }
    // U8: table row (channel) of slot j — two compile-time candidates selected by the lane half
    auto lut_row = [&](int j) __attribute__((always_inline)) {
      const int kA = 16 * (j >> 3) + (j & 7), kB = kA + 8 >= 27 ? kA : kA + 8;
      return (half ? kB / 9 : kA / 9) * 257;
    };
    auto tap_of = [&](int j) __attribute__((always_inline)) {  // border tiles only
      const int kA = 16 * (j >> 3) + (j & 7), kB = kA + 8 >= 27 ? kA : kA + 8;
      return half ? kB % 9 : kA % 9;
    };

    float xv[3][16];
    // issue the input gathers of one tile (48 coalesced dword loads per lane); nothing waits here
    auto issue_loads = [&](int tile) __attribute__((always_inline)) {
      int n, ty, tx;
      stem_decode(p, tile, n, ty, tx);
      const int y0 = ty * 8 - 1, x0 = tx * 32 - 1;
      // element (fp32) / byte (uint8) offset of the halo origin; may be "negative" for border tiles
      const int origin = U8 ? ((n * p.H + y0) * p.W + x0) * 3 : ((n * 3) * p.H + y0) * p.W + x0;
      if (stem_is_interior(p, ty, tx)) {
#pragma unroll
        for (int bi = 0; bi < 3; ++bi) {
          if (pw + 4 * bi >= ST_BLOCKS) continue;  // wave-uniform
          const int base = origin + g_rel[bi];
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            if constexpr (U8)
              xv[bi][j] = __builtin_bit_cast(
                  float, (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rs_x, base + g_dk[j], 0, 0));
            else
              xv[bi][j] = __builtin_bit_cast(
                  float, __builtin_amdgcn_raw_buffer_load_b32(rs_x, (base + g_dk[j]) * 4, 0, 0));
          }
        }
      } else {
#pragma unroll
        for (int bi = 0; bi < 3; ++bi) {
          if (pw + 4 * bi >= ST_BLOCKS) continue;
          const int y = y0 + g_hy[bi], x = x0 + g_hx[bi];
          unsigned mk = 0;
          if (y >= 0 && y < p.H && x >= 0 && x < p.W) {
            const bool ya = y > 0, yc = y + 1 < p.H, xa = x > 0, xc = x + 1 < p.W;
            mk = (ya && xa ? 1u : 0u) | (ya ? 2u : 0u) | (ya && xc ? 4u : 0u) | (xa ? 8u : 0u) | 16u |
                 (xc ? 32u : 0u) | (yc && xa ? 64u : 0u) | (yc ? 128u : 0u) | (yc && xc ? 256u : 0u);
          }
          const int base = origin + g_rel[bi];
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const bool ok = (mk >> tap_of(j)) & 1u;
            if constexpr (U8) {
              // an invalid tap must read as 0.0 AFTER normalisation: table entry 256
              const unsigned off = ok ? (unsigned)(base + g_dk[j]) : ST_OOB;
              const unsigned u = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rs_x, (int)off, 0, 0);
              xv[bi][j] = __builtin_bit_cast(float, ok ? u : 256u);
            } else {
              const unsigned off = ok ? (unsigned)(base + g_dk[j]) * 4u : ST_OOB;
              xv[bi][j] = __builtin_bit_cast(float,
                                             __builtin_amdgcn_raw_buffer_load_b32(rs_x, (int)off, 0, 0));
            }
          }
        }
      }
    };
    // conv1_1 on the loaded window, bias + ReLU + bf16, halo tile -> LDS
    auto finish = [&](int tile, char* buf) __attribute__((always_inline)) {
      int n, ty, tx;
      stem_decode(p, tile, n, ty, tx);
      const int y0 = ty * 8 - 1, x0 = tx * 32 - 1;
      const bool interior = stem_is_interior(p, ty, tx);
#pragma unroll
      for (int bi = 0; bi < 3; ++bi) {
        if (pw + 4 * bi >= ST_BLOCKS) continue;  // wave-uniform
        bf16x8_t xf[2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            if constexpr (U8)
              xf[s][e] = (short)lut[lut_row(8 * s + e) + (int)__builtin_bit_cast(unsigned, xv[bi][8 * s + e])];
            else
              xf[s][e] = (short)f32_to_bf16_bits(xv[bi][8 * s + e]);
          }
        f32x16_t acc[2];
        __builtin_amdgcn_s_setprio(3);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[t][r] = bb[t][r];
#pragma unroll
          for (int s = 0; s < 2; ++s)
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[t][s], xf[s], acc[t], 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);
        // D[row = cout][col = pixel]: registers 4g..4g+3 = couts 32 t + 8 g + 4 half + 0..3 of the
        // lane's pixel -> 8 bytes of its 128-byte halo row, 16-B slot 4 t + g (swizzled), +8 half.
        // A halo pixel outside the image is conv1_2's zero padding, not a conv1_1 output.
        const int y = y0 + g_hy[bi], x = x0 + g_hx[bi];
        const bool pix_ok = interior || (y >= 0 && y < p.H && x >= 0 && x < p.W);
        if (g_row[bi] < ST_HALO_PX) {
          char* row = buf + g_row[bi] * 128 + 8 * half;
#pragma unroll
          for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              uint2 v;
              v.x = relu_bf16x2(pack_bf16x2(acc[t][4 * g], acc[t][4 * g + 1]));
              v.y = relu_bf16x2(pack_bf16x2(acc[t][4 * g + 2], acc[t][4 * g + 3]));
              if (!pix_ok) v = make_uint2(0u, 0u);
              *reinterpret_cast<uint2*>(row + (((4 * t + g) ^ g_swz[bi]) << 4)) = v;
            }
        }
      }
    };

    const bool prof = p.prof != nullptr && blockIdx.x == 0 && wave == 4;
    unsigned long long pt[2] = {0, 0};
    // producer runs one tile ahead of the consumers; the gathers of the tile after that are
    // already in flight while it waits at the hand-over barrier
    if (niter > 0) {
      issue_loads(first);
      finish(first, hb);
      if (niter > 1) issue_loads(first + stride);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int it = 0; it < niter; ++it) {
      const unsigned long long t0 = prof ? __builtin_amdgcn_s_memtime() : 0;
      if (it + 1 < niter) {
        finish(first + (it + 1) * stride, hb + ((it + 1) & 1) * ST_HALO_BYTES);
        if (it + 2 < niter) issue_loads(first + (it + 2) * stride);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const unsigned long long t1 = prof ? __builtin_amdgcn_s_memtime() : 0;
      __builtin_amdgcn_s_barrier();
      if (prof) {
        const unsigned long long t2 = __builtin_amdgcn_s_memtime();
        pt[0] += t1 - t0;
        pt[1] += t2 - t1;
      }
    }
    if (prof && lane == 0) {
      p.prof[4] = pt[0];
      p.prof[5] = pt[1];
    }
    return;
  }

  // ================================== consumers ================================================
  {
    const int piece = ((lane & 7) ^ (4 * (wave & 1) + (lane >> 4))) * 16;
#pragma unroll
    for (int j = 0; j < 18; ++j) {
      const int q = j * 4 + wave;
      const int r = q * 8 + (lane >> 3);
      const int tap = r >> 6, c = r & 63;
      glds16(p.w2 + ((long)(tap * 64 + c) * 64) * 2 + piece, wl + q * 1024);
    }
  }
  int lhy[2], lhx[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    lhy[i] = 2 * wave + ((l31 >> 1) & 1);
    lhx[i] = 16 * i + 2 * (l31 >> 2) + (l31 & 1);
  }
  int w_off[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) w_off[kk] = l31 * 128 + (((2 * kk + half) ^ ((l31 >> 1) & 7)) << 4);
  float bvals[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) bvals[tn] = p.b2[tn * 32 + l31];

  const bool cprof = p.prof != nullptr && blockIdx.x == 0 && wave == 0;
  unsigned long long ct[3] = {0, 0, 0};
  // The pooled outputs of tile i are held back (8 packed registers) and stored one pixel at a time
  // between the matrix steps of tile i+1, so the store issue hides in the MFMA shadow.  A pending
  // pixel is ONE dword per lane: lanes l31 and l31 ^ 1 exchange halves (DPP + v_perm), the even lane
  // stores channels (l31, l31 + 1), the odd lane channels (32 + l31 - 1, 32 + l31) — a half-wave
  // writes the full 128-byte line of its pixel — through a buffer descriptor of ONE OUTPUT ROW
  // (rebuilt per tile from scalars; zero records for a row below the map): a pixel right of the map
  // is out of range and dropped by the hardware, its distance is the instruction's immediate.  No
  // mask, no compare, no branch in the matrix loop (as in vgg_stem_x3_kernel, stem_x3.h).
  uint32_t pend[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) pend[e] = 0;
  __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, 0, 0x00020000);  // nothing pending
  const unsigned lane_off = half * 128 + ((l31 & 1) ? 64 + (l31 - 1) * 2 : l31 * 2);
  const uint32_t psel = (l31 & 1) ? 0x03020706u : 0x05040100u;
  unsigned poff = lane_off;
  auto store_px = [&](int e) __attribute__((always_inline)) {
    __builtin_amdgcn_raw_buffer_store_b32(pend[e], rs_o, (int)(poff + 256u * e), 0, 0);
  };
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), as the builtin: see the f16mx consumers
  __builtin_amdgcn_s_barrier();
  for (int it = 0; it < niter; ++it) {
    const unsigned long long c0 = cprof ? __builtin_amdgcn_s_memtime() : 0;
    const int tile = first + it * stride;
    const char* const cur = hb + (it & 1) * ST_HALO_BYTES;
    f32x16_t acc[2][2];  // start at the bias, like every convolution kernel here
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][tn][r] = bvals[tn];
    bf16x8_t fa[2][2], fb[2][2];
    auto load_step = [&](int sidx, bf16x8_t (&a)[2], bf16x8_t (&b)[2]) __attribute__((always_inline)) {
      const int tap = sidx >> 2, kk = sidx & 3;
      const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int hy = lhy[i] + ky, hx = lhx[i] + kx;
        a[i] = *reinterpret_cast<const bf16x8_t*>(
            cur + (hy * C64_HW + hx) * 128 + (((2 * kk + half) ^ c64_swz(hy, hx)) << 4));
      }
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
        b[tn] = *reinterpret_cast<const bf16x8_t*>(wl + tap * 8192 + tn * 4096 + w_off[kk]);
    };
    load_step(0, fa[0], fb[0]);
#pragma unroll
    for (int sidx = 0; sidx < 36; ++sidx) {
      if (sidx + 1 < 36) load_step(sidx + 1, fa[(sidx + 1) & 1], fb[(sidx + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
          acc[i][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[sidx & 1][i], fb[sidx & 1][tn],
                                                               acc[i][tn], 0, 0, 0);
      if ((sidx & 3) == 1 && (sidx >> 2) < 8) store_px(sidx >> 2);
    }
    // all fragment reads of `cur` have been consumed by the MFMAs above: hand the buffer back
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const unsigned long long c1 = cprof ? __builtin_amdgcn_s_memtime() : 0;
    __builtin_amdgcn_s_barrier();
    const unsigned long long c2 = cprof ? __builtin_amdgcn_s_memtime() : 0;
    // pooled epilogue from registers: lanes 0-31 / 32-63 each hold the 32 channels of one pooled
    // pixel (64 contiguous bytes); the two tn halves (low / high 16 bits) complete the 128-byte line
    int n, ty, tx;
    stem_decode(p, tile, n, ty, tx);
    const int oy = ty * 4 + wave;
    // lane's first pooled pixel (i = g = 0) of this wave's pooled row; pixel e = 4 i + g is 2 e
    // pixels = 256 e bytes further: immediate offsets on one base offset into the row's descriptor
    rs_o = __builtin_amdgcn_make_buffer_rsrc(p.out + ((long)n * Ho + oy) * Wo * 128, 0,
                                             oy < Ho ? Wo * 128 : 0, 0x00020000);
    poff = lane_off + (unsigned)tx * (16 * 128);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float v[2];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
          v[tn] = fmaxf(fmaxf(fmaxf(acc[i][tn][4 * g], acc[i][tn][4 * g + 1]),
                              fmaxf(acc[i][tn][4 * g + 2], acc[i][tn][4 * g + 3])), 0.f);
        const uint32_t mine = pack_bf16x2(v[0], v[1]);
        const uint32_t other = (uint32_t)__builtin_amdgcn_mov_dpp((int)mine, 0xB1, 0xF, 0xF, true);  // lane ^ 1
        pend[4 * i + g] = __builtin_amdgcn_perm(other, mine, psel);
      }
    if (cprof) {
      const unsigned long long c3 = __builtin_amdgcn_s_memtime();
      ct[0] += c1 - c0;
      ct[1] += c2 - c1;
      ct[2] += c3 - c2;
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) store_px(e);
  if (cprof && lane == 0) {
    p.prof[0] = ct[0];
    p.prof[1] = ct[1];
    p.prof[2] = ct[2];
  }
}
