// conv1_1 (Cin = 3) on its own: on the vector ALU in exact fp32 and on the matrix cores in bf16 / bf16x3 (included by
// stem.hip inside namespace oibl, behind stem_parts.h; launched by oibl_conv1_1_nchw).

// ---------------------------------------------------------------------------------------------
// conv1_1: x [N][3][H][W] fp32 -> out [N][H][W][64] T.   Cin = 3 gives K = 27: no MFMA shape fits
// without an explicit im2col pass, and the layer is 0.56 % of the backbone FLOPs, so it runs on
// the vector ALU in exact fp32:  lane = output channel (its 27 weights live in registers), a wave
// walks a strip of 8 pixels; the strip's input window is wave-uniform (scalar/broadcast loads) and
// every store is one full NHWC line (64 channels contiguous).
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void conv1_1_kernel(const float* __restrict__ x,
                                                      const float* __restrict__ w,
                                                      const float* __restrict__ bias,
                                                      T* __restrict__ out, int N, int H, int W) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int spr = (W + 7) >> 3;  // strips per row
  const long nstrips = (long)N * H * spr;
  const long strip = (long)blockIdx.x * 4 + wave;
  if (strip >= nstrips) return;
  const int n = (int)(strip / ((long)H * spr));
  const int rem = (int)(strip - (long)n * H * spr);
  const int y = rem / spr;
  const int x0 = (rem - y * spr) * 8;

  float wr[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) wr[k] = w[lane * 27 + k];
  const float b = bias[lane];
  float acc[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) acc[p] = b;

#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int yy = y + ky - 1;
      if (yy < 0 || yy >= H) continue;  // wave-uniform
      const float* row = x + (((size_t)n * 3 + c) * H + yy) * W;
      float v[10];
#pragma unroll
      for (int i = 0; i < 10; ++i) {
        const int xx = x0 - 1 + i;
        v[i] = (xx >= 0 && xx < W) ? row[xx] : 0.f;
      }
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int p = 0; p < 8; ++p) acc[p] = fmaf(v[p + kx], wr[c * 9 + ky * 3 + kx], acc[p]);
    }
  }
  T* o = out + (((size_t)n * H + y) * W + x0) * 64 + lane;
#pragma unroll
  for (int p = 0; p < 8; ++p)
    if (x0 + p < W) Elem<T>::store(o + (size_t)p * 64, fmaxf(acc[p], 0.f));
}

// ---------------------------------------------------------------------------------------------
// conv1_1 on the matrix cores (bf16 precision only): K = 27 is padded to 32 = two k-steps of
// v_mfma_f32_32x32x16_bf16.  The GEMM is run transposed (D[cout][pixel] = W . X^T): the weights
// are the A operand (kept in registers for the whole kernel) and 32 pixels of an image row are
// the B operand, so that each lane ends up with 4 CONSECUTIVE output channels of one pixel per
// register quad -> 8-byte packed bf16 writes into an LDS staging tile and full 128-byte NHWC
// lines on the way out.  The layer is bound by writing its 64-channel output (39 MB / image in
// bf16), not by the MFMA work.
//   workgroup = 4 waves = 128 consecutive pixels of one image row; persistent over row segments;
//   input patch (3 channels x 3 rows x 130 columns, zero padded) staged in LDS as fp32, rounded
//   to bf16 when the fragments are built.
// ---------------------------------------------------------------------------------------------
constexpr int C11_TW = 128;
constexpr int C11_PITCH = 132;
constexpr int C11_ZERO = 9 * C11_PITCH;  // index of a zero float (k >= 27)


// X3 = bf16x3: weights and pixels are split into (hi, lo) fragments, 3 MFMAs per k-step, and the
// output is written as groups of [32 hi | 32 lo] (256 B per pixel).
template <bool X3>
__global__ __launch_bounds__(256) void conv1_1_mfma_kernel(const float* __restrict__ x,
                                                           const float* __restrict__ w,
                                                           const float* __restrict__ bias,
                                                           char* __restrict__ out, int N, int H,
                                                           int W, int tiles_per_row, long ntiles) {
  constexpr int PX_BYTES = X3 ? 256 : 128, OPITCH = PX_BYTES + 16;
  __shared__ __attribute__((aligned(16))) float patch[9 * C11_PITCH + 4];
  __shared__ __attribute__((aligned(16))) char ostage_all[4 * 32 * OPITCH];  // per wave: 32 px
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int half = lane >> 5, l31 = lane & 31;

  // A operand: weights.  wf[t][s] element e  <->  cout = 32 t + l31,  k = 16 s + 8 half + e
  bf16x8_t wf[2][2], wl[2][2];
  int koff[2][8];  // LDS float offset of input element k (relative to the pixel's column)
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = 16 * s + 8 * half + e;
      koff[s][e] = k < 27 ? (k / 3) * C11_PITCH + (k % 3) : -1;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float v = k < 27 ? w[(32 * t + l31) * 27 + k] : 0.f;
        uint16_t hi, lo;
        x3_split(v, hi, lo);
        wf[t][s][e] = (short)hi;
        wl[t][s][e] = (short)lo;
      }
    }
  float bb[2][16];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) bb[t][r] = bias[32 * t + acc_row(r, lane)];
  if (threadIdx.x < 4) patch[C11_ZERO + threadIdx.x] = 0.f;

  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int tx = (int)(tile % tiles_per_row);
    const long ny = tile / tiles_per_row;
    const int y = (int)(ny % H), n = (int)(ny / H);
    const int x0 = tx * C11_TW;
    __syncthreads();  // the previous tile's fragment reads are done
    for (int i = threadIdx.x; i < 9 * 130; i += 256) {
      const int r = i / 130, col = i - r * 130;
      const int yy = y + (r % 3) - 1, xx = x0 - 1 + col;
      float v = 0.f;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W)
        v = x[(((size_t)n * 3 + r / 3) * H + yy) * W + xx];
      patch[r * C11_PITCH + col] = v;
    }
    __syncthreads();

    const int px = wave * 32 + l31;  // pixel column inside the tile
    bf16x8_t xf[2], xl[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = koff[s][e] >= 0 ? patch[koff[s][e] + px] : 0.f;
        uint16_t hi, lo;
        x3_split(v, hi, lo);
        xf[s][e] = (short)hi;
        xl[s][e] = (short)lo;
      }
    f32x16_t acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = bb[t][r];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if constexpr (X3) {
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[t][s], xf[s], acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[t][s], xl[s], acc[t], 0, 0, 0);
        }
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[t][s], xf[s], acc[t], 0, 0, 0);
      }
    }
    // D[row = cout][col = pixel]: registers 4g..4g+3 = couts 32t + 8g + 4*half + 0..3 of pixel l31
    char* ost = ostage_all + wave * 32 * OPITCH;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if constexpr (X3) {
          uint2 hi, lo;
          ring_split4(fmaxf(acc[t][4 * g], 0.f), fmaxf(acc[t][4 * g + 1], 0.f),
                      fmaxf(acc[t][4 * g + 2], 0.f), fmaxf(acc[t][4 * g + 3], 0.f), hi, lo);
          char* q = ost + l31 * OPITCH + t * 128 + (8 * g + 4 * half) * 2;
          *reinterpret_cast<uint2*>(q) = hi;
          *reinterpret_cast<uint2*>(q + 64) = lo;
        } else {
          uint2 v;
          v.x = relu_bf16x2(pack_bf16x2(acc[t][4 * g], acc[t][4 * g + 1]));
          v.y = relu_bf16x2(pack_bf16x2(acc[t][4 * g + 2], acc[t][4 * g + 3]));
          *reinterpret_cast<uint2*>(ost + l31 * OPITCH + (32 * t + 8 * g + 4 * half) * 2) = v;
        }
      }
    __builtin_amdgcn_wave_barrier();  // same-wave exchange through LDS: DS ops retire in order
    char* orow = out + (((size_t)n * H + y) * W + x0 + wave * 32) * PX_BYTES;
    constexpr int PARTS = PX_BYTES / 16;
#pragma unroll
    for (int it = 0; it < 32 * PARTS / 64; ++it) {
      const int idx = it * 64 + lane, p = idx / PARTS, part = idx % PARTS;
      const uint4 v = *reinterpret_cast<const uint4*>(ost + p * OPITCH + part * 16);
      if (x0 + wave * 32 + p < W)
        *reinterpret_cast<uint4*>(orow + (size_t)p * PX_BYTES + part * 16) = v;
    }
    __builtin_amdgcn_wave_barrier();
  }
}
