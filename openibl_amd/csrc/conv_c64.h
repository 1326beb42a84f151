// conv3x3_c64_kernel: the bf16 Cin = 64 convolution with resident weights and an LDS halo (included by stem.hip inside
// namespace oibl; launched by launch_conv_c64).  The fused stems build on its tile, halo image and swizzle.

// ---------------------------------------------------------------------------------------------
// Cin = 64 convolutions (conv1_2, conv2_1) — "resident weights + LDS halo" kernel, bf16.
// With K = 9 * 64 the generic implicit GEMM has only nine K-steps per tile: its cost is the
// per-tile prologue / epilogue and the L2 -> LDS traffic of re-fetching every input pixel once per
// tap, not the matrix cores.  Here a persistent workgroup
//   * keeps ALL weights of its 64-output-channel slice in LDS (9 taps x 64 x 64 bf16 = 72 KiB,
//     fetched once),
//   * stages the (8+2) x (32+2) pixel halo of an 8 x 32 output tile ONCE (42.5 KiB instead of
//     9 x 32 KiB), double-buffered so the next tile's halo streams in (global_load_lds) while the
//     current one is multiplied,
//   * runs the 9 taps x 4 k-steps = 144 MFMAs per wave straight out of LDS with no barrier,
//   * reuses the consumed halo buffer as the staging area of the coalesced NHWC store.
// LDS: 72 KiB + 2 x 43 KiB = 158 KiB of the CU's 160 KiB -> one workgroup (4 waves) per CU.
// The halo image is XOR-swizzled by f(hy, hx) = ((hx >> 1) & 7) ^ ((hy & 1) << 2) (halo rows are
// 34 x 128 B = 17 bank rows, so banks depend on hx only; the hy term separates the two image rows
// a pooled quad spans): every ds_read_b128 lane group is conflict-free for all nine taps in both
// the linear and the quad-major (pooling) pixel order (checked exhaustively).
// ---------------------------------------------------------------------------------------------
constexpr int C64_HW = 34;                         // halo width  (32 + 2)
constexpr int C64_HALO_ROWS = 344;                 // 10 x 34 = 340 halo pixels, padded to 43 x 8
constexpr int C64_HALO_BYTES = C64_HALO_ROWS * 128;
constexpr int C64_W_BYTES = 9 * 64 * 128;
constexpr int C64_LDS_BYTES = C64_W_BYTES + 2 * C64_HALO_BYTES;
constexpr int C64_HALO_LOADS = 11;                 // ceil(43 wave-instructions / 4 waves)
constexpr int C64_WAVE_REGION = 10880;             // per-wave epilogue staging inside a halo buffer

struct C64Params {
  const char* in;
  const char* w;
  const float* bias;
  char* out;
  const char* zero;
  int N, H, W, cout, relu;
  int tiles_x, tiles_y;
  int ntiles;
  unsigned long long* prof;  // optional (test hook): per-phase shader-clock totals of block 0 wave 0
};

__device__ static inline int c64_swz(int hy, int hx) { return ((hx >> 1) & 7) ^ ((hy & 1) << 2); }

template <bool POOL>
__global__ __launch_bounds__(256, 1) void conv3x3_c64_kernel(C64Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const wl = smem;
  char* const hb = smem + C64_W_BYTES;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  const int co0 = blockIdx.y * 64;

  // weights of this 64-channel slice -> LDS rows r = tap * 64 + c (same swizzle as the GEMM core)
  {
    const int piece = ((lane & 7) ^ (4 * (wave & 1) + (lane >> 4))) * 16;
#pragma unroll
    for (int j = 0; j < 18; ++j) {
      const int q = j * 4 + wave;
      const int r = q * 8 + (lane >> 3);
      const int tap = r >> 6, c = r & 63;
      glds16(p.w + ((long)(tap * p.cout + co0 + c) * 64) * 2 + piece, wl + q * 1024);
    }
  }
  // halo loader: instruction j of this wave fills halo pixels r = (4j + wave) * 8 + (lane >> 3)
  int h_rel[C64_HALO_LOADS];    // hy << 8 | hx   (hy >= 10: padding row, always zero)
  int h_piece[C64_HALO_LOADS];
#pragma unroll
  for (int j = 0; j < C64_HALO_LOADS; ++j) {
    const int r = (j * 4 + wave) * 8 + (lane >> 3);
    const int hy = r / C64_HW, hx = r - hy * C64_HW;
    h_rel[j] = (hy << 8) | hx;
    h_piece[j] = ((lane & 7) ^ c64_swz(hy, hx)) * 16;
  }
  const char* const zsrc = p.zero + (lane & 7) * 16;
  const long row_bytes = (long)p.W * 128, img_bytes = (long)p.H * row_bytes;

  auto issue_halo = [&](int tile, char* buf) {
    const unsigned r2 = (unsigned)tile / (unsigned)p.tiles_x;
    const int tx = tile - (int)r2 * p.tiles_x;
    const int n = (int)(r2 / (unsigned)p.tiles_y), ty = (int)r2 - n * p.tiles_y;
    const int y0 = ty * 8 - 1, x0 = tx * 32 - 1;
    const char* base = p.in + n * img_bytes;
#pragma unroll
    for (int j = 0; j < C64_HALO_LOADS; ++j) {
      const int q = j * 4 + wave;
      if (q < C64_HALO_ROWS / 8) {  // wave-uniform
        const int hy = h_rel[j] >> 8, hx = h_rel[j] & 255;
        const int y = y0 + hy, x = x0 + hx;
        const bool ok = hy < 10 && y >= 0 && y < p.H && x >= 0 && x < p.W;
        glds16(ok ? base + y * row_bytes + (long)x * 128 + h_piece[j] : zsrc, buf + q * 1024);
      }
    }
  };

  // lane geometry inside the wave's 2 tile rows x 32 columns
  int lhy[2], lhx[2];  // halo coordinates (tap 0,0) of this lane's pixel in M-tile i
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (POOL) {
      lhy[i] = 2 * wave + ((l31 >> 1) & 1);
      lhx[i] = 16 * i + 2 * (l31 >> 2) + (l31 & 1);
    } else {
      lhy[i] = 2 * wave + i;
      lhx[i] = l31;
    }
  }
  int w_off[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) w_off[kk] = l31 * 128 + (((2 * kk + half) ^ ((l31 >> 1) & 7)) << 4);
  float bvals[2];
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) bvals[tn] = p.bias[co0 + tn * 32 + l31];

  int tile = blockIdx.x;
  if (tile < p.ntiles) issue_halo(tile, hb);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const bool prof = p.prof != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && wave == 0;
  unsigned long long pt[6] = {0, 0, 0, 0, 0, 0};
#define C64_TICK(i)                                        \
  if (prof) {                                              \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
    pt[i] += now_ - t_prev;                                \
    t_prev = now_;                                         \
  }
  for (int it = 0; tile < p.ntiles; tile += gridDim.x, ++it) {
    unsigned long long t_prev = prof ? __builtin_amdgcn_s_memtime() : 0;
    char* const cur = hb + (it & 1) * C64_HALO_BYTES;
    const int nxt = tile + (int)gridDim.x;
    if (nxt < p.ntiles) issue_halo(nxt, hb + ((it & 1) ^ 1) * C64_HALO_BYTES);
    C64_TICK(0)

    f32x16_t acc[2][2];  // start at the bias, like every convolution kernel here
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][tn][r] = bvals[tn];

    // 36 steps (tap-major, 4 k-steps per tap), fragment reads software-pipelined one step ahead:
    // with one wave per SIMD nothing else hides the LDS latency.
    bf16x8_t fa[2][2], fb[2][2];
    auto load_step = [&](int sidx, bf16x8_t (&a)[2], bf16x8_t (&b)[2]) {
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
      __builtin_amdgcn_sched_barrier(0);  // keep the next step's reads AHEAD of this step's MFMAs
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
          acc[i][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[sidx & 1][i], fb[sidx & 1][tn],
                                                               acc[i][tn], 0, 0, 0);
    }
    // The next tile's halo (issued before the MFMAs) has landed; every wave is done reading `cur`,
    // which now becomes the store staging area.  Raw s_barrier + explicit counters: __syncthreads()
    // would also wait (vmcnt(0)) for the global stores of the epilogue below, a 1-2 us bubble per
    // tile; they are left in flight and only waited for after the next tile's MFMAs.
    C64_TICK(1)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    C64_TICK(2)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    C64_TICK(3)

    const unsigned r2 = (unsigned)tile / (unsigned)p.tiles_x;
    const int tx = tile - (int)r2 * p.tiles_x;
    const int n = (int)(r2 / (unsigned)p.tiles_y), ty = (int)r2 - n * p.tiles_y;
    char* const st = cur + wave * C64_WAVE_REGION;  // wave-private: no barrier for the exchange
    if (POOL) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            float v = fmaxf(fmaxf(acc[i][tn][4 * g], acc[i][tn][4 * g + 1]),
                            fmaxf(acc[i][tn][4 * g + 2], acc[i][tn][4 * g + 3]));
            if (p.relu) v = fmaxf(v, 0.f);
            const int qx = 8 * i + 2 * g + half;
            *reinterpret_cast<uint16_t*>(st + qx * 144 + (tn * 32 + l31) * 2) = f32_to_bf16_bits(v);
          }
      __builtin_amdgcn_wave_barrier();
      const int Ho = p.H >> 1, Wo = p.W >> 1;
      const int oy = ty * 4 + wave;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int idx = k * 64 + lane, qx = idx >> 3, part = idx & 7;
        const int ox = tx * 16 + qx;
        const uint4 v = *reinterpret_cast<const uint4*>(st + qx * 144 + part * 16);
        if (oy < Ho && ox < Wo)
          *reinterpret_cast<uint4*>(p.out + (((long)n * Ho + oy) * Wo + ox) * p.cout * 2 + co0 * 2 +
                                    part * 16) = v;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float v = acc[i][tn][r];
            if (p.relu) v = fmaxf(v, 0.f);
            const int prow = i * 32 + acc_row(r, lane);
            *reinterpret_cast<uint16_t*>(st + prow * 144 + (tn * 32 + l31) * 2) = f32_to_bf16_bits(v);
          }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int idx = k * 64 + lane, prow = idx >> 3, part = idx & 7;
        const int y = ty * 8 + 2 * wave + (prow >> 5), x = tx * 32 + (prow & 31);
        const uint4 v = *reinterpret_cast<const uint4*>(st + prow * 144 + part * 16);
        if (y < p.H && x < p.W)
          *reinterpret_cast<uint4*>(p.out + (((long)n * p.H + y) * p.W + x) * p.cout * 2 + co0 * 2 +
                                    part * 16) = v;
      }
    }
    // staging reads retired before the next iteration's LDS-DMA overwrites this buffer
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    C64_TICK(4)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    C64_TICK(5)
  }
#undef C64_TICK
  if (prof && lane == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) p.prof[i] = pt[i];
  }
}
