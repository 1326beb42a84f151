// Gradients of a 3x3 / pad 1 / stride 1 convolution (+ the ReLU behind it) on gfx950: nn.Conv2d(C, C, 3, padding=1)
// followed by nn.ReLU as torch autograd differentiates them (ibl/models/vgg.py:41-42, 61-62), for the three conv5
// layers the reference trains (C = 512 in and out), NHWC fp32 activations, the state-dict's OIHW weight.
//
// With M = N H W pixels, dZ = grad_out where out_act > 0 (else 0; all of grad_out without out_act):
//   grad_w[co][ci][ky][kx] = sum_m dZ[m][co] in[m + (ky-1, kx-1)][ci]       zeros outside the map
//   grad_b[co]             = sum_m dZ[m][co]
//   grad_in                = conv3x3(dZ; w'[ci][co][ky][kx] = w[co][ci][2-ky][2-kx]), pad 1, no bias, no ReLU
//
//   cb_mask_kernel     dZ into the workspace (only with out_act; the stages read grad_out itself without)
//   cb_wgrad_kernel    the weight gradient: per tap a [512 x 512] = dZ^T . shift(in) contraction over the M pixels, both
//                      operands read K-outer / channel-inner straight from NHWC, `in` shifted by the tap with border
//                      predication.  One workgroup per (128 x 128 tile, tap, K split): 4 waves of 64 x 64 on
//                      v_mfma_f32_32x32x2_f32, 32 pixels per LDS step, the next step's global loads in flight behind
//                      the current step's MFMAs.  The pixels are cut into SEGMENTS of CB_SEG = 256: one accumulator
//                      chain (a plain fmaf chain whose error grows with its length) never runs longer than a segment;
//                      a finished segment is added to a second register tile.  K split s of S <= CB_SMAX takes the
//                      segments s, s + S, ... and writes one fp32 partial [9][512][512].
//   cb_wreduce_kernel  grad_w = sum_s partial[s] in fp64, in split order, rounded once, written OIHW
//   cb_bsum_kernel     per 256-pixel segment the 512 column sums in fp64: two halves in pixel order, first + second
//   cb_breduce_kernel  grad_b = the segments' sums in fp64, in segment order, rounded once
//   cb_packT_kernel    w' packed [tap][ci][co] (the forward kernel's layout with the roles of Cin / Cout swapped) and a
//                      zero bias; grad_in is then the exact-fp32 forward convolution of dZ (oibl_conv3x3_nhwc,
//                      OIBL_F32, one pass: every output pixel is one fixed-order sum over its own 9 x 512 products)
// No floating-point atomics and no data-dependent order anywhere: bit-identical from run to run; an output does not
// depend on which others are asked for; the pixel decomposition of grad_in is per output pixel, so an image's rows
// do not depend on its batch mates.
#include "gemm_core.h"

namespace oibl {

constexpr int CB_C = 512;
constexpr int CB_SEG = 256;          // pixels per accumulator chain (and per bias-sum block)
constexpr int CB_SMAX = 7;           // K splits of the weight gradient: 16 x 9 x 7 = 1008 workgroups, two rounds of the
                                     // 512 that 256 CUs hold at two per CU (8 splits: 1152, a third round a quarter full)
constexpr int CB_LP = 160;           // floats per LDS row of a 32-pixel x 128-channel step: the two lane halves of a
                                     // fragment read (rows p, p + 1) land 32 banks apart
constexpr size_t CB_TAPS_CC = (size_t)9 * CB_C * CB_C;

__global__ __launch_bounds__(256) void cb_mask_kernel(const float4* __restrict__ g, const float4* __restrict__ act,
                                                      float4* __restrict__ dz, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 a = act[i];
    float4 v = g[i];
    v.x = a.x > 0.f ? v.x : 0.f;
    v.y = a.y > 0.f ? v.y : 0.f;
    v.z = a.z > 0.f ? v.z : 0.f;
    v.w = a.w > 0.f ? v.w : 0.f;
    dz[i] = v;
  }
}

// grid (16 tiles: co tile = x >> 2, ci tile = x & 3; 9 taps; S splits)
// (M < 2^31: pixel indices and their divisions are 32-bit)
__global__ __launch_bounds__(256, 2) void cb_wgrad_kernel(const float* __restrict__ in, const float* __restrict__ dz,
                                                          float* __restrict__ partial, int H, int W, int M, int S) {
  constexpr int C = CB_C;
  __shared__ __attribute__((aligned(16))) float a_s[32 * CB_LP];   // dZ      [32 pixels][128 co]
  __shared__ __attribute__((aligned(16))) float b_s[32 * CB_LP];   // shifted [32 pixels][128 ci]
  const int co0 = ((int)blockIdx.x >> 2) * 128, ci0 = ((int)blockIdx.x & 3) * 128;
  const int tap = blockIdx.y, s = blockIdx.z;
  const int dy = tap / 3 - 1, dx = tap % 3 - 1;
  const int shift = dy * W + dx;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, kh = lane >> 5;
  // staging roles: a step is 32 pixels x 128 channels = 1024 float4 per operand, 4 per thread: pixel (t >> 5) + 8 q
  const int sp = (int)threadIdx.x >> 5, sc = ((int)threadIdx.x & 31) * 4;

  f32x16_t acc[2][2], tot[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = tot[i][j][r] = 0.f;

  float4 pa[4], pb[4];
  auto prefetch = [&](unsigned m0) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned m = m0 + sp + 8 * q;
      pa[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      pb[q] = pa[q];
      if (m < (unsigned)M) {
        pa[q] = *reinterpret_cast<const float4*>(dz + (size_t)m * C + co0 + sc);
        const unsigned row = m / (unsigned)W;
        const int x = (int)(m - row * (unsigned)W);
        const int y = (int)(row % (unsigned)H);
        if ((unsigned)(y + dy) < (unsigned)H && (unsigned)(x + dx) < (unsigned)W)
          pb[q] = *reinterpret_cast<const float4*>(in + (size_t)((int)m + shift) * C + ci0 + sc);
      }
    }
  };
  // step g of this split: segment s + S (g / 8), its pixels [32 (g % 8), + 32)
  // (64-bit: the step behind the last one may lie beyond 2^31)
  auto step_base = [&](int g) -> long { return ((long)s + (long)S * (g >> 3)) * CB_SEG + 32 * (g & 7); };

  int g = 0;
  prefetch((unsigned)step_base(0));
  for (;;) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      *reinterpret_cast<float4*>(a_s + (sp + 8 * q) * CB_LP + sc) = pa[q];
      *reinterpret_cast<float4*>(b_s + (sp + 8 * q) * CB_LP + sc) = pb[q];
    }
    __syncthreads();
    const long nb = step_base(g + 1);
    const bool more = nb < M;          // (the segments of a split ascend: once beyond M, always beyond M)
    if (more) prefetch((unsigned)nb);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int p = 2 * k + kh;
      const float a0 = a_s[p * CB_LP + wm * 64 + l31], a1 = a_s[p * CB_LP + wm * 64 + 32 + l31];
      const float b0 = b_s[p * CB_LP + wn * 64 + l31], b1 = b_s[p * CB_LP + wn * 64 + 32 + l31];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
    if ((g & 7) == 7 || !more) {       // the segment's chain ends here
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            tot[i][j][r] += acc[i][j][r];
            acc[i][j][r] = 0.f;
          }
    }
    if (!more) break;
    ++g;
  }
  float* out = partial + ((size_t)s * 9 + tap) * C * C;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + wm * 64 + 32 * i + acc_row(r, lane);
        const int ci = ci0 + wn * 64 + 32 * j + l31;
        out[(size_t)co * C + ci] = tot[i][j][r];
      }
}

// one thread per (co, ci): the nine taps of the S partials, fp64, split order -> grad_w[co][ci][3][3]
__global__ __launch_bounds__(256) void cb_wreduce_kernel(const float* __restrict__ partial, float* __restrict__ gw,
                                                         int S) {
  constexpr int CC = CB_C * CB_C;
  const int i = blockIdx.x * 256 + threadIdx.x;   // co * 512 + ci
  if (i >= CC) return;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    double v = 0.0;
    for (int s = 0; s < S; ++s) v += (double)partial[((size_t)s * 9 + tap) * CC + i];
    gw[(size_t)i * 9 + tap] = (float)v;
  }
}

// block = one 256-pixel segment: thread t the channels 4 (t & 127) .. + 3 of the segment's first (t < 128) or second
// 128 pixels, in pixel order; the two halves are added through LDS, first + second
__global__ __launch_bounds__(256) void cb_bsum_kernel(const float* __restrict__ dz, double* __restrict__ part, long M) {
  __shared__ double hi_s[CB_C];
  const int half = (int)threadIdx.x >> 7, c4 = ((int)threadIdx.x & 127) * 4;
  const long m0 = (long)blockIdx.x * CB_SEG + 128 * half;
  const long m1 = m0 + 128 < M ? m0 + 128 : M;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 8
  for (long m = m0; m < m1; ++m) {
    const float4 v = *reinterpret_cast<const float4*>(dz + (size_t)m * CB_C + c4);
    s0 += (double)v.x;
    s1 += (double)v.y;
    s2 += (double)v.z;
    s3 += (double)v.w;
  }
  if (half) {
    hi_s[c4] = s0;
    hi_s[c4 + 1] = s1;
    hi_s[c4 + 2] = s2;
    hi_s[c4 + 3] = s3;
  }
  __syncthreads();
  if (!half) {
    double* o = part + (size_t)blockIdx.x * CB_C + c4;
    o[0] = s0 + hi_s[c4];
    o[1] = s1 + hi_s[c4 + 1];
    o[2] = s2 + hi_s[c4 + 2];
    o[3] = s3 + hi_s[c4 + 3];
  }
}
__global__ __launch_bounds__(512) void cb_breduce_kernel(const double* __restrict__ part, float* __restrict__ gb,
                                                         int nseg) {
  double v = 0.0;
  for (int s = 0; s < nseg; ++s) v += part[(size_t)s * CB_C + threadIdx.x];
  gb[threadIdx.x] = (float)v;
}

// w [co][ci][9] -> packed[tap][ci][co] = w[co][ci][8 - tap] (taps flipped, channels swapped), through a 32 x 32 x 9
// LDS tile (288 contiguous floats in per co, 32 contiguous floats out per (tap, ci)); block 0 also clears the bias
__global__ __launch_bounds__(256) void cb_packT_kernel(const float* __restrict__ w, float* __restrict__ packed,
                                                       float* __restrict__ zero_bias) {
  constexpr int C = CB_C;
  __shared__ float tile[32][289];
  const int co0 = ((int)blockIdx.x >> 4) * 32, ci0 = ((int)blockIdx.x & 15) * 32;
  for (int idx = threadIdx.x; idx < 32 * 288; idx += 256) {
    const int col = idx / 288, j = idx - col * 288;
    tile[col][j] = w[((size_t)(co0 + col) * C + ci0) * 9 + j];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 9 * 32 * 32; idx += 256) {
    const int col = idx & 31, cil = (idx >> 5) & 31, tap = idx >> 10;
    packed[((size_t)tap * C + ci0 + cil) * C + co0 + col] = tile[col][cil * 9 + (8 - tap)];
  }
  if (blockIdx.x == 0) {
    zero_bias[threadIdx.x] = 0.f;
    zero_bias[256 + threadIdx.x] = 0.f;
  }
}

static int cb_nseg(long M) { return (int)((M + CB_SEG - 1) / CB_SEG); }
static int cb_splits(long M) {
  const int n = cb_nseg(M);
  return n < CB_SMAX ? n : CB_SMAX;
}

}  // namespace oibl

using namespace oibl;

extern "C" {

// workspace: dZ [M][512] | weight-gradient partials [S][9][512][512] | bias sums [nseg][512] fp64 |
//            (with grad_in) w' [9][512][512] | zero bias [512]
static size_t cb_off_wp(long M) { return align_up((size_t)M * CB_C * sizeof(float), 256); }
static size_t cb_off_bp(long M) { return cb_off_wp(M) + align_up((size_t)cb_splits(M) * CB_TAPS_CC * sizeof(float), 256); }
static size_t cb_off_wt(long M) { return cb_off_bp(M) + align_up((size_t)cb_nseg(M) * CB_C * sizeof(double), 256); }
static size_t cb_off_zb(long M) { return cb_off_wt(M) + align_up(CB_TAPS_CC * sizeof(float), 256); }

size_t oibl_conv3x3_backward_workspace_bytes(int N, int H, int W, int cin, int cout, int want_grad_in) {
  if (N < 1 || H < 1 || W < 1 || cin != CB_C || cout != CB_C) return 0;
  const long M = (long)N * H * W;
  if (M >= 0x7fffffffL) return 0;
  return want_grad_in ? cb_off_zb(M) + align_up(CB_C * sizeof(float), 256) : cb_off_wt(M);
}

int oibl_conv3x3_backward(const float* in, int N, int H, int W, int cin, const float* w_oihw, int cout,
                          const float* out_act, const float* grad_out, float* grad_w, float* grad_b, float* grad_in,
                          void* ws, size_t ws_bytes, void* stream) {
  OIBL_REQUIRE(in && w_oihw && grad_out && ws, "conv3x3_backward: null pointer");
  OIBL_REQUIRE(grad_w || grad_b || grad_in, "conv3x3_backward: no output requested");
  OIBL_REQUIRE(cin == CB_C && cout == CB_C, "conv3x3_backward: kernels are built for Cin = Cout = 512 (got %d, %d)", cin,
               cout);
  OIBL_REQUIRE(N > 0 && H > 0 && W > 0, "conv3x3_backward: bad shape N=%d H=%d W=%d", N, H, W);
  const long M = (long)N * H * W;
  OIBL_REQUIRE(M < 0x7fffffffL, "conv3x3_backward: N*H*W must be < 2^31 (split the batch)");
  OIBL_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)w_oihw % 16 == 0 && (uintptr_t)out_act % 16 == 0 &&
                   (uintptr_t)grad_out % 16 == 0 && (uintptr_t)grad_w % 16 == 0 && (uintptr_t)grad_b % 16 == 0 &&
                   (uintptr_t)grad_in % 16 == 0,
               "conv3x3_backward: pointers must be 16-byte aligned");
  const size_t need = oibl_conv3x3_backward_workspace_bytes(N, H, W, cin, cout, grad_in != nullptr);
  if ((uintptr_t)ws % 256 != 0) {
    set_error("conv3x3_backward: workspace must be 256-byte aligned");
    return OIBL_E_WORKSPACE;
  }
  if (ws_bytes < need) {
    set_error("conv3x3_backward: workspace %zu < required %zu bytes", ws_bytes, need);
    return OIBL_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* wsb = (char*)ws;
  const int nseg = cb_nseg(M), S = cb_splits(M);
  const float* dz = grad_out;
  if (out_act) {
    float* dzm = (float*)wsb;
    const size_t n4 = (size_t)M * (CB_C / 4);
    const size_t blocks = (n4 + 255) / 256;
    hipLaunchKernelGGL(cb_mask_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, st,
                       (const float4*)grad_out, (const float4*)out_act, (float4*)dzm, n4);
    OIBL_LAUNCH_CHECK();
    dz = dzm;
  }
  if (grad_w) {
    float* partial = (float*)(wsb + cb_off_wp(M));
    hipLaunchKernelGGL(cb_wgrad_kernel, dim3(16, 9, (unsigned)S), dim3(256), 0, st, in, dz, partial, H, W, (int)M, S);
    OIBL_LAUNCH_CHECK();
    hipLaunchKernelGGL(cb_wreduce_kernel, dim3(CB_C * CB_C / 256), dim3(256), 0, st, (const float*)partial, grad_w, S);
    OIBL_LAUNCH_CHECK();
  }
  if (grad_b) {
    double* part = (double*)(wsb + cb_off_bp(M));
    hipLaunchKernelGGL(cb_bsum_kernel, dim3((unsigned)nseg), dim3(256), 0, st, dz, part, M);
    OIBL_LAUNCH_CHECK();
    hipLaunchKernelGGL(cb_breduce_kernel, dim3(1), dim3(512), 0, st, (const double*)part, grad_b, nseg);
    OIBL_LAUNCH_CHECK();
  }
  if (grad_in) {
    float* wt = (float*)(wsb + cb_off_wt(M));
    float* zb = (float*)(wsb + cb_off_zb(M));
    hipLaunchKernelGGL(cb_packT_kernel, dim3(256), dim3(256), 0, st, w_oihw, wt, zb);
    OIBL_LAUNCH_CHECK();
    return oibl_conv3x3_nhwc(dz, N, H, W, CB_C, wt, zb, CB_C, 0, 0, OIBL_F32, grad_in, stream);
  }
  return OIBL_OK;
}

}  // extern "C"
