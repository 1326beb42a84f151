// Gradients of the NetVLAD descriptor head on gfx950: NetVLAD.forward (ibl/models/netvlad.py:44-61) followed by
// the intra-normalisation and the L2 normalisation of EmbedNet.forward (netvlad.py:78-80), differentiated with
// respect to conv.weight ([K][C]), centroids ([K][C]) and the conv5 map ([N][P][C], NHWC).
//
// Per image, x_p the P rows of the map, w_k / c_k the rows of assign_w / centroids, eps = 1e-12:
//   forward    r_p = max(|x_p|, eps), xh_p = x_p / r_p (normalize_input == 0: xh = x)
//              s_pk = w_k . xh_p, a_p = softmax_k(s_p), A_k = sum_p a_pk
//              V_k = sum_p a_pk xh_p - A_k c_k, t_k = max(|V_k|, eps), U_k = V_k / t_k
//              g = max(|U|_F, eps), Y = U / g                      (vlad_norm, k-major)
//   backward   dU = (G - Y <Y, G>) / g                              G = dL/dY, <.,.> over all K C entries
//              dV_k = (dU_k - U_k <U_k, dU_k>) / t_k
//              dC_k = -A_k dV_k                                     summed over the images
//              da_pk = <dV_k, xh_p> - <dV_k, c_k>
//              ds_pk = a_pk (da_pk - sum_j a_pj da_pj)
//              dW_k = sum_p ds_pk xh_p                              summed over the images
//              dxh_p = sum_k (a_pk dV_k + ds_pk w_k)
//              dx_p = (dxh_p - xh_p <xh_p, dxh_p>) / r_p
//   where a max(., eps) is active its denominator is a constant (torch's clamp_min): the projection term is dropped.
//
// The reference keeps residual[N][K][C][P] for autograd (157 MB per 30 x 40 image); nothing of that size exists
// here.  The call is stateless: it recomputes r, a and V from the map, then
//   nvb_assign_kernel        one workgroup per (32-pixel chunk, image): the chunk's 32 x 512 values in LDS, |x_p| and
//                            the logits in fp64 on the vector unit (see the kernel: its a is a more accurate
//                            evaluation than the forward kernels', not their bits), softmax      -> r[P], a[P][64]
//   nvb_aggregate_kernel<0>  netvlad_aggregate_kernel's scheme on v_mfma_f32_32x32x2_f32, one workgroup per (image,
//                            64 channels), all the image's pixels in order; A in fp64            -> V[K][C], A[K]
//   nvb_rowstats_kernel      one wave per (image, cluster): t_k, |U_k|^2, <U_k, G_k>
//   nvb_dv_kernel            one wave per (image, cluster): g, <Y, G>, dU, dV (over V), <dV_k, c_k>, the image's
//                            dC = -A_k dV_k — these two kernels in fp64 throughout
//   nvb_contract_kernel      the chunk against the image's dV on the matrix cores (every wave contracts its 128
//                            channels, the four partial [32 x 64] tiles are added through LDS): da, ds -> ds[P][64]
//   nvb_aggregate_kernel<1>  the aggregation with ds in the place of a                           -> dW of the image
//   nvb_dx_kernel            one workgroup per (32-pixel chunk, image): dxh = [a | ds] . [dV ; w] (32 x 512 over
//                            128) on the same instruction, the projection, the division          -> grad_feat
//   nvb_reduce_kernel        dW = sum_n dW_n (fp32), dC = sum_n dC_n (fp64, rounded once), both in image order
// No floating-point atomics: every sum has a fixed order, results are bit-identical from run to run, and the pixel
// decomposition (chunks of 32 in pixel order) depends on P alone, so an image's grad_feat rows do not depend on its
// batch mates.  Three of the four heavy contractions (V / dW, da, dxh) are exact fp32 on the matrix cores.  What
// feeds dC is wider: a tuple loss's dL/dY sum to zero over a tuple, so the images' dC contributions cancel (60-fold
// on near-identical maps) and every fp32 rounding of a contribution is multiplied by that factor — the logits, the
// norms, the normalisations' backward and the per-image dC are therefore fp64.
#include "gemm_core.h"

namespace oibl {

constexpr int NVB_C = 512;
constexpr int NVB_K = 64;
constexpr int NVB_XP = 516;          // floats per LDS row of the chunk: 16-byte aligned, +4 banks per pixel
constexpr int NVB_LP = 65;           // pitch of the [32][64] partial tiles
constexpr int NVB_AP = 129;          // pitch of the [32][128] operand tile [a | ds]
constexpr int NVB_CONTRACT_LDS = (32 * NVB_XP + 4 * 32 * NVB_LP + 32) * 4;
constexpr int NVB_DX_LDS = (32 * NVB_XP + 32 * NVB_AP + 4 * 32 + 32 + 32) * 4;
constexpr float NVB_EPS = 1e-12f;

__device__ static inline double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the chunk [p0, p0 + 32) of one image -> x_s[32][NVB_XP]; pixels beyond P read as zeros
__device__ static inline void nvb_load_chunk(const float* __restrict__ fimg, int p0, int P, float* x_s) {
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int idx = (int)threadIdx.x + 256 * q;          // float4 index inside the chunk
    const int px = idx >> 7, c4 = (idx & 127) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p0 + px < P) v = *reinterpret_cast<const float4*>(fimg + (size_t)(p0 + px) * NVB_C + c4);
    *reinterpret_cast<float4*>(x_s + px * NVB_XP + c4) = v;
  }
}

// rn[p] = |x_p| (1 without normalize) and a[p][k] = softmax_k(w_k . x_p / r_p) for one 32-pixel chunk of one image.
// The logits and the norm are accumulated in fp64 on the vector unit, not on the fp32 matrix cores: a tuple loss makes
// the images' contributions to dC cancel (60-fold on near-identical maps), and the rounding of fp32 logits alone —
// 512-term sums whose terms are far larger than the sum — then costs 8e-7 to 3e-6 of dC.  This `a` is therefore NOT
// the forward kernels' `a` bit for bit (netvlad.hip forms its logits on the fp32 matrix cores): the backward
// differentiates the same function from a more accurate evaluation of it.  Eight threads per pixel, thread `sub`
// the clusters sub, sub + 8, ..., sub + 56; the weights pass through LDS in four slices of 128 channels, [cluster]
// [channel] as in memory (coalesced 512-byte row pieces in, the eight rows of a wave's reads on distinct banks).
constexpr int NVB_WP = 132;          // floats per LDS row of the weight slice: 16-byte aligned, +4 banks per cluster
constexpr int NVB_ASSIGN_LDS = (32 * NVB_XP + NVB_K * NVB_WP) * 4;
__global__ __launch_bounds__(256) void nvb_assign_kernel(const float* __restrict__ feat, const float* __restrict__ w,
                                                         float* __restrict__ rn, float* __restrict__ a, int P,
                                                         int normalize) {
  constexpr int C = NVB_C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const x_s = reinterpret_cast<float*>(smem);             // [32][NVB_XP]
  float* const w_s = x_s + 32 * NVB_XP;                           // [64 clusters][NVB_WP]: 128 channels of a slice
  const int n = blockIdx.y, p0 = blockIdx.x * 32;
  const int px = (int)threadIdx.x >> 3, sub = (int)threadIdx.x & 7;
  nvb_load_chunk(feat + (size_t)n * P * C, p0, P, x_s);
  double acc[8], ss = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.0;
  for (int c0 = 0; c0 < C; c0 += 128) {
    __syncthreads();                                              // the chunk is in LDS / the last slice is consumed
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = (int)threadIdx.x + 256 * q;
      const int c4 = idx & 31, k = idx >> 5;                      // k < 64; 32 lanes walk one row's 512 bytes
      *reinterpret_cast<float4*>(w_s + k * NVB_WP + 4 * c4) =
          *reinterpret_cast<const float4*>(w + (size_t)k * C + c0 + 4 * c4);
    }
    __syncthreads();
    const float* xr = x_s + px * NVB_XP + c0;
    const float* wr = w_s + sub * NVB_WP;
#pragma unroll 2
    for (int c = 0; c < 128; c += 4) {
      const float4 xv = *reinterpret_cast<const float4*>(xr + c);
      const double x0 = (double)xv.x, x1 = (double)xv.y, x2 = (double)xv.z, x3 = (double)xv.w;
      ss = fma(x0, x0, ss);
      ss = fma(x1, x1, ss);
      ss = fma(x2, x2, ss);
      ss = fma(x3, x3, ss);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float4 wv = *reinterpret_cast<const float4*>(wr + 8 * j * NVB_WP + c);
        acc[j] = fma(x0, (double)wv.x, acc[j]);
        acc[j] = fma(x1, (double)wv.y, acc[j]);
        acc[j] = fma(x2, (double)wv.z, acc[j]);
        acc[j] = fma(x3, (double)wv.w, acc[j]);
      }
    }
  }
  const double rd = normalize ? sqrt(ss) : 1.0;
  const double invd = 1.0 / fmax(rd, (double)NVB_EPS);
  float l[8], mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    l[j] = (float)(acc[j] * invd);
    mx = fmaxf(mx, l[j]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
  float ssum = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    l[j] = expf(l[j] - mx);
    ssum += l[j];
  }
  ssum += __shfl_xor(ssum, 1, 64);
  ssum += __shfl_xor(ssum, 2, 64);
  ssum += __shfl_xor(ssum, 4, 64);
  const float is = 1.0f / ssum;
  if (p0 + px < P) {
    float* dst = a + ((size_t)n * P + p0 + px) * NVB_K + sub;
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[8 * j] = l[j] * is;         // the eight threads of a pixel: 32 bytes per j
    if (sub == 0) rn[(size_t)n * P + p0 + px] = (float)rd;
  }
}

// ds[p][k] = a_pk (da_pk - sum_j a_pj da_pj), da_pk = dV_k . x_p / r_p - dvc_k, for one 32-pixel chunk of one image:
// the chunk in LDS, every wave contracts its 128 channels against the image's dV on v_mfma_f32_32x32x2_f32, the four
// partial [32 x 64] tiles are added through LDS.  `out` may alias `a` (every element is read and written by the same
// thread).
__global__ __launch_bounds__(256) void nvb_contract_kernel(const float* __restrict__ feat, const float* __restrict__ B,
                                                           const float* __restrict__ dvc, const float* __restrict__ rn,
                                                           const float* a, float* out, int P) {
  constexpr int C = NVB_C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const x_s = reinterpret_cast<float*>(smem);             // [32][NVB_XP]
  float* const lp_s = x_s + 32 * NVB_XP;                          // [4 waves][32][NVB_LP]
  float* const inv_s = lp_s + 4 * 32 * NVB_LP;                    // [32]
  const int n = blockIdx.y, p0 = blockIdx.x * 32;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l31 = lane & 31, kh = lane >> 5;
  const float* fimg = feat + (size_t)n * P * C;
  B += (size_t)n * NVB_K * C;

  nvb_load_chunk(fimg, p0, P, x_s);
  if (threadIdx.x < 32) {
    const int p = p0 + (int)threadIdx.x;
    inv_s[threadIdx.x] = p < P ? 1.0f / fmaxf(rn[(size_t)n * P + p], NVB_EPS) : 0.f;
  }
  __syncthreads();
  {  // partial contraction over this wave's 128 channels: [32 pixels] x [64 rows of B]
    f32x16_t lg[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) lg[ct][r] = 0.f;
    const float* xa = x_s + l31 * NVB_XP + 128 * wave + 4 * kh;
    const float* wb = B + (size_t)l31 * C + 128 * wave + 4 * kh;
#pragma unroll 4
    for (int j = 0; j < 16; ++j) {
      const float4 av = *reinterpret_cast<const float4*>(xa + 8 * j);
      const float4 b0 = *reinterpret_cast<const float4*>(wb + 8 * j);
      const float4 b1 = *reinterpret_cast<const float4*>(wb + (size_t)32 * C + 8 * j);
      lg[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b0.x, lg[0], 0, 0, 0);
      lg[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b1.x, lg[1], 0, 0, 0);
      lg[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b0.y, lg[0], 0, 0, 0);
      lg[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b1.y, lg[1], 0, 0, 0);
      lg[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b0.z, lg[0], 0, 0, 0);
      lg[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b1.z, lg[1], 0, 0, 0);
      lg[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b0.w, lg[0], 0, 0, 0);
      lg[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b1.w, lg[1], 0, 0, 0);
    }
    float* lw = lp_s + wave * 32 * NVB_LP;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) lw[acc_row(r, lane) * NVB_LP + 32 * ct + l31] = lg[ct][r];
  }
  __syncthreads();
  {  // eight threads per pixel, eight clusters each
    const int px = (int)threadIdx.x >> 3, sub = (int)threadIdx.x & 7;
    const float iv = inv_s[px];
    const bool live = p0 + px < P;
    float l[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int o = px * NVB_LP + sub * 8 + k;
      l[k] = (lp_s[o] + lp_s[32 * NVB_LP + o] + lp_s[2 * 32 * NVB_LP + o] + lp_s[3 * 32 * NVB_LP + o]) * iv;
    }
    float* dst = out + ((size_t)n * P + p0 + px) * NVB_K + sub * 8;
    {
      float av[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) av[k] = 0.f;
      if (live) {
        const float* src = a + ((size_t)n * P + p0 + px) * NVB_K + sub * 8;
        const float4 a0 = *reinterpret_cast<const float4*>(src), a1 = *reinterpret_cast<const float4*>(src + 4);
        av[0] = a0.x; av[1] = a0.y; av[2] = a0.z; av[3] = a0.w;
        av[4] = a1.x; av[5] = a1.y; av[6] = a1.z; av[7] = a1.w;
      }
      float dot = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        l[k] -= dvc[n * NVB_K + sub * 8 + k];
        dot = fmaf(av[k], l[k], dot);
      }
      dot += __shfl_xor(dot, 1, 64);
      dot += __shfl_xor(dot, 2, 64);
      dot += __shfl_xor(dot, 4, 64);
      if (live) {
        *reinterpret_cast<float4*>(dst) = make_float4(av[0] * (l[0] - dot), av[1] * (l[1] - dot),
                                                      av[2] * (l[2] - dot), av[3] * (l[3] - dot));
        *reinterpret_cast<float4*>(dst + 4) = make_float4(av[4] * (l[4] - dot), av[5] * (l[5] - dot),
                                                          av[6] * (l[6] - dot), av[7] * (l[7] - dot));
      }
    }
  }
}

// out[n][k][c0..c0+63] = sum_p a[p][k] xh[p][c] for one image and one 64-channel slice, the pixels in order.
// MODE 0: minus (sum_p a[p][k]) centroids[k][c], and A[n][k] = sum_p a[p][k] (every slice computes the same sums
// in the same order; slice 0 writes them).  MODE 1: the plain sum (a = ds: the image's dW).
// 4 waves as 2 (clusters) x 2 (channels), one 32x32 fp32 accumulator tile each.
template <int MODE>
__global__ __launch_bounds__(256) void nvb_aggregate_kernel(const float* __restrict__ feat,
                                                            const float* __restrict__ rn, const float* __restrict__ a,
                                                            const float* __restrict__ centroids,
                                                            float* __restrict__ out, double* __restrict__ A, int P) {
  constexpr int C = NVB_C;
  __shared__ __attribute__((aligned(16))) float a_s[32][64];
  __shared__ __attribute__((aligned(16))) float x_s[32][64];
  __shared__ float s_sum[64];
  const int n = blockIdx.x, c0 = blockIdx.y * 64;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const float* fbase = feat + (size_t)n * P * C + c0;
  const float* abase = a + (size_t)n * P * 64;
  const float* rbase = rn + (size_t)n * P;

  f32x16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  double colsum = 0.0;  // threads 0..63: sum_p a[p][tid], in fp64 (1200 terms of a 30 x 40 map)

  // staging roles: a chunk = 32 x 64 floats = 512 float4 (2 per thread); x chunk = 32 pixels x 64 channels
  // (8 threads per pixel, 8 channels each).  The next chunk's loads are issued before the current chunk's MFMAs.
  const int xp = threadIdx.x >> 3, xc = (threadIdx.x & 7) * 8;
  float4 pa[2], px0, px1;
  float psc;
  auto prefetch = [&](int p0) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = threadIdx.x + q * 256;  // float4 index
      const int pr = idx >> 4, cq = (idx & 15) * 4;
      pa[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p0 + pr < P) pa[q] = *reinterpret_cast<const float4*>(abase + (size_t)(p0 + pr) * 64 + cq);
    }
    px0 = make_float4(0.f, 0.f, 0.f, 0.f);
    px1 = px0;
    psc = 0.f;
    if (p0 + xp < P) {
      psc = 1.0f / fmaxf(rbase[p0 + xp], NVB_EPS);
      const float* src = fbase + (size_t)(p0 + xp) * C + xc;
      px0 = *reinterpret_cast<const float4*>(src);
      px1 = *reinterpret_cast<const float4*>(src + 4);
    }
  };
  prefetch(0);
  for (int p0 = 0; p0 < P; p0 += 32) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = threadIdx.x + q * 256;
      *reinterpret_cast<float4*>(&a_s[idx >> 4][(idx & 15) * 4]) = pa[q];
    }
    *reinterpret_cast<float4*>(&x_s[xp][xc]) = make_float4(px0.x * psc, px0.y * psc, px0.z * psc, px0.w * psc);
    *reinterpret_cast<float4*>(&x_s[xp][xc + 4]) = make_float4(px1.x * psc, px1.y * psc, px1.z * psc, px1.w * psc);
    __syncthreads();
    if (p0 + 32 < P) prefetch(p0 + 32);
    if (MODE == 0 && threadIdx.x < 64) {
#pragma unroll
      for (int p = 0; p < 32; ++p) colsum += (double)a_s[p][threadIdx.x];
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int p = 2 * s + (lane >> 5);
      const float av = a_s[p][wm * 32 + (lane & 31)];
      const float bv = x_s[p][wn * 32 + (lane & 31)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  if (MODE == 0) {
    if (threadIdx.x < 64) {
      s_sum[threadIdx.x] = (float)colsum;
      if (blockIdx.y == 0) A[n * 64 + threadIdx.x] = colsum;
    }
    __syncthreads();
  }
  const int ch = c0 + wn * 32 + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int k = wm * 32 + acc_row(r, lane);
    float v = acc[r];
    if (MODE == 0) v -= s_sum[k] * centroids[(size_t)k * C + ch];
    out[((size_t)n * 64 + k) * C + ch] = v;
  }
}

// one wave per (image, cluster) row of V: st[row] = { |V_k| , |U_k|^2 , <U_k, G_k> }, U_k = V_k / max(|V_k|, eps).
// This kernel and the next evaluate the two normalisations' backward in fp64 from the fp32 rows: a tuple loss makes
// the images' dC contributions cancel (its dL/dY sum to zero over a tuple; 60-fold on near-identical maps), which
// multiplies every fp32 rounding of a contribution by that factor.
__global__ __launch_bounds__(256) void nvb_rowstats_kernel(const float* __restrict__ V, const float* __restrict__ G,
                                                           double* __restrict__ st, long rows) {
  constexpr int C = NVB_C;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* v = V + row * C;
  const float* g = G + row * C;
  double vv[8], gg[8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float4 a = *reinterpret_cast<const float4*>(v + 256 * h + 4 * lane);
    const float4 b = *reinterpret_cast<const float4*>(g + 256 * h + 4 * lane);
    vv[4 * h] = a.x; vv[4 * h + 1] = a.y; vv[4 * h + 2] = a.z; vv[4 * h + 3] = a.w;
    gg[4 * h] = b.x; gg[4 * h + 1] = b.y; gg[4 * h + 2] = b.z; gg[4 * h + 3] = b.w;
  }
  double ss = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) ss += vv[i] * vv[i];
  ss = wave_sum_f64(ss);
  const double t = sqrt(ss);
  const double it = 1.0 / fmax(t, (double)NVB_EPS);
  double s2 = 0.0, ug = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const double u = vv[i] * it;
    s2 += u * u;
    ug += u * gg[i];
  }
  s2 = wave_sum_f64(s2);
  ug = wave_sum_f64(ug);
  if (lane == 0) {
    st[3 * row] = t;
    st[3 * row + 1] = s2;
    st[3 * row + 2] = ug;
  }
}

// one wave per (image, cluster) row: V_k -> dV_k in place (fp32, the operand of the later contractions),
// dvc[row] = <dV_k, c_k>, and, where dCp is given, the image's dC row -A_k dV_k in fp64
__global__ __launch_bounds__(256) void nvb_dv_kernel(float* __restrict__ V, const float* __restrict__ G,
                                                     const double* __restrict__ st, const double* __restrict__ A,
                                                     const float* __restrict__ centroids, float* __restrict__ dvc,
                                                     double* __restrict__ dCp, long rows) {
  constexpr int C = NVB_C, K = NVB_K;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long n = row / K;
  const int k = (int)(row - n * K);
  // |U|_F^2 and <U, G> of the image: lane j holds cluster j's, the same fixed-order sum in every wave of the image
  const double S2 = wave_sum_f64(st[3 * (n * K + lane) + 1]);
  const double UG = wave_sum_f64(st[3 * (n * K + lane) + 2]);
  const double gn = sqrt(S2);
  const bool g_clamped = gn < (double)NVB_EPS;
  const double ig = 1.0 / fmax(gn, (double)NVB_EPS);
  const double yg = g_clamped ? 0.0 : UG * ig;                      // <Y, G>; a clamped g is a constant
  const double t = st[3 * row];
  const bool t_clamped = t < (double)NVB_EPS;
  const double it = 1.0 / fmax(t, (double)NVB_EPS);
  float* v = V + row * C;
  const float* g = G + row * C;
  const float* c = centroids + (size_t)k * C;
  double u[8], du[8], cc[8];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float4 a = *reinterpret_cast<const float4*>(v + 256 * h + 4 * lane);
    const float4 b = *reinterpret_cast<const float4*>(g + 256 * h + 4 * lane);
    const float4 d = *reinterpret_cast<const float4*>(c + 256 * h + 4 * lane);
    u[4 * h] = a.x * it; u[4 * h + 1] = a.y * it; u[4 * h + 2] = a.z * it; u[4 * h + 3] = a.w * it;
    du[4 * h] = b.x; du[4 * h + 1] = b.y; du[4 * h + 2] = b.z; du[4 * h + 3] = b.w;
    cc[4 * h] = d.x; cc[4 * h + 1] = d.y; cc[4 * h + 2] = d.z; cc[4 * h + 3] = d.w;
  }
  double dot = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    du[i] = (du[i] - u[i] * ig * yg) * ig;
    dot += u[i] * du[i];
  }
  const double fd = t_clamped ? 0.0 : wave_sum_f64(dot);
  double dc = 0.0;
  double dv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    dv[i] = (du[i] - u[i] * fd) * it;
    dc += dv[i] * cc[i];
  }
  dc = wave_sum_f64(dc);
#pragma unroll
  for (int h = 0; h < 2; ++h)
    *reinterpret_cast<float4*>(v + 256 * h + 4 * lane) =
        make_float4((float)dv[4 * h], (float)dv[4 * h + 1], (float)dv[4 * h + 2], (float)dv[4 * h + 3]);
  if (dCp != nullptr) {
    const double na = -A[row];
    double* o = dCp + row * C;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 4; ++i) o[256 * h + 4 * lane + i] = na * dv[4 * h + i];
  }
  if (lane == 0) dvc[row] = (float)dc;
}

// grad_feat of one 32-pixel chunk of one image: dxh[p][c] = sum_k a[p][k] dV[k][c] + sum_k ds[p][k] w[k][c], every
// wave its 128 channels (4 accumulator tiles of 32 pixels x 32 channels, 128 contraction steps), then
// dx_p = (dxh_p - xh_p <xh_p, dxh_p>) / r_p.
__global__ __launch_bounds__(256) void nvb_dx_kernel(const float* __restrict__ feat, const float* __restrict__ rn,
                                                     const float* __restrict__ a, const float* __restrict__ ds,
                                                     const float* __restrict__ dV, const float* __restrict__ w,
                                                     float* __restrict__ grad_feat, int P, int normalize) {
  constexpr int C = NVB_C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const x_s = reinterpret_cast<float*>(smem);             // [32][NVB_XP]
  float* const ad_s = x_s + 32 * NVB_XP;                          // [32][NVB_AP]: a | ds
  float* const red_s = ad_s + 32 * NVB_AP;                        // [4 waves][32]
  float* const inv_s = red_s + 4 * 32;                            // [32]
  float* const dot_s = inv_s + 32;                                // [32]
  const int n = blockIdx.y, p0 = blockIdx.x * 32;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l31 = lane & 31, kh = lane >> 5;
  const float* fimg = feat + (size_t)n * P * C;
  dV += (size_t)n * NVB_K * C;

  nvb_load_chunk(fimg, p0, P, x_s);
#pragma unroll
  for (int q = 0; q < 4; ++q) {                                   // 32 x 128 floats = 1024 float4
    const int idx = (int)threadIdx.x + 256 * q;
    const int px = idx >> 5, k4 = (idx & 31) * 4;                 // k4 < 64: a, else ds
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p0 + px < P) {
      const float* src = (k4 < 64 ? a : ds) + ((size_t)n * P + p0 + px) * NVB_K + (k4 & 63);
      v = *reinterpret_cast<const float4*>(src);
    }
    float* d = ad_s + px * NVB_AP + k4;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  if (threadIdx.x < 32) {
    const int p = p0 + (int)threadIdx.x;
    inv_s[threadIdx.x] = p < P ? 1.0f / fmaxf(rn[(size_t)n * P + p], NVB_EPS) : 0.f;
    // the projection is dropped where the input is not normalised or its norm sits on the clamp
    dot_s[threadIdx.x] = 0.f;
  }
  __syncthreads();

  f32x16_t acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
  const float* arow = ad_s + l31 * NVB_AP + kh;
  const int cb = 128 * wave + l31;
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    const float* Bm = (half == 0 ? dV : w) + (size_t)kh * C + cb;
    const float* ar = arow + 64 * half;
#pragma unroll 4
    for (int s = 0; s < 32; ++s) {
      const float av = ar[2 * s];
      const float* br = Bm + (size_t)(2 * s) * C;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, br[32 * ct], acc[ct], 0, 0, 0);
    }
  }
  if (normalize) {
    // <x_p, dxh_p>: this wave's 128 channels, then the four waves in wave order
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int px = acc_row(r, lane);
      float v = 0.f;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) v = fmaf(acc[ct][r], x_s[px * NVB_XP + cb + 32 * ct], v);
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 8, 64);
      v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 1, 64);
      if (l31 == 0) red_s[wave * 32 + px] = v;
    }
    __syncthreads();
    if (threadIdx.x < 32) {
      const int p = p0 + (int)threadIdx.x;
      const float iv = inv_s[threadIdx.x];
      const bool clamped = p < P ? rn[(size_t)n * P + p] < NVB_EPS : true;
      const float d = ((red_s[threadIdx.x] + red_s[32 + threadIdx.x]) + red_s[64 + threadIdx.x]) + red_s[96 + threadIdx.x];
      dot_s[threadIdx.x] = clamped ? 0.f : d * iv * iv;         // <xh_p, dxh_p> / r_p: it multiplies x_p below
    }
    __syncthreads();
  }
  float* gimg = grad_feat + (size_t)n * P * C;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int px = acc_row(r, lane);
    if (p0 + px < P) {
      const float iv = inv_s[px], d = dot_s[px];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int ch = cb + 32 * ct;
        gimg[(size_t)(p0 + px) * C + ch] = (acc[ct][r] - x_s[px * NVB_XP + ch] * d) * iv;
      }
    }
  }
}

// dW = sum_n dWp[n] (fp32), dC = sum_n dCp[n] (fp64, rounded once), both in image order; either output may be null
__global__ __launch_bounds__(256) void nvb_reduce_kernel(const float* __restrict__ dWp, const double* __restrict__ dCp,
                                                         float* __restrict__ dW, float* __restrict__ dC, int N) {
  constexpr int KC = NVB_K * NVB_C;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= KC) return;
  if (dW) {
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += dWp[(size_t)n * KC + i];
    dW[i] = s;
  }
  if (dC) {
    double s = 0.0;
    for (int n = 0; n < N; ++n) s += dCp[(size_t)n * KC + i];
    dC[i] = (float)s;
  }
}

}  // namespace oibl

using namespace oibl;

extern "C" {

// workspace: r [N][P] | a [N][P][64] | V -> dV [N][K][C] | stats [N][K][3] fp64 | A [N][K] fp64 | dvc [N][K] |
//            dW of every image [N][K][C] | dC of every image [N][K][C] fp64 |
//            ds [N][P][64] (only with grad_feat: without it ds overwrites a)
static size_t nvb_off_a(int N, int P) { return align_up((size_t)N * P * sizeof(float), 256); }
static size_t nvb_off_v(int N, int P) { return nvb_off_a(N, P) + align_up((size_t)N * P * 64 * sizeof(float), 256); }
static size_t nvb_off_st(int N, int P, int K, int C) {
  return nvb_off_v(N, P) + align_up((size_t)N * K * C * sizeof(float), 256);
}
static size_t nvb_off_A(int N, int P, int K, int C) {
  return nvb_off_st(N, P, K, C) + align_up((size_t)N * K * 3 * sizeof(double), 256);
}
static size_t nvb_off_dvc(int N, int P, int K, int C) {
  return nvb_off_A(N, P, K, C) + align_up((size_t)N * K * sizeof(double), 256);
}
static size_t nvb_off_dwp(int N, int P, int K, int C) {
  return nvb_off_dvc(N, P, K, C) + align_up((size_t)N * K * sizeof(float), 256);
}
static size_t nvb_off_dcp(int N, int P, int K, int C) {
  return nvb_off_dwp(N, P, K, C) + align_up((size_t)N * K * C * sizeof(float), 256);
}
static size_t nvb_off_ds(int N, int P, int K, int C) {
  return nvb_off_dcp(N, P, K, C) + align_up((size_t)N * K * C * sizeof(double), 256);
}

size_t oibl_netvlad_backward_workspace_bytes(int N, int P, int K, int C, int want_grad_feat) {
  if (N <= 0 || P <= 0 || K != NVB_K || C != NVB_C) return 0;
  return nvb_off_ds(N, P, K, C) + (want_grad_feat ? align_up((size_t)N * P * 64 * sizeof(float), 256) : 0);
}

int oibl_netvlad_backward(const void* feat, int N, int P, int K, int C, int precision, const float* assign_w,
                          const float* centroids, int normalize_input, const float* grad_vlad_norm,
                          float* grad_assign_w, float* grad_centroids, float* grad_feat, void* ws, size_t ws_bytes,
                          void* stream) {
  OIBL_REQUIRE(feat && assign_w && centroids && grad_vlad_norm && ws, "netvlad_backward: null pointer");
  OIBL_REQUIRE(grad_assign_w || grad_centroids || grad_feat, "netvlad_backward: no output requested");
  OIBL_REQUIRE(precision == OIBL_F32, "netvlad_backward: the feature map must be fp32 (got precision %d)", precision);
  OIBL_REQUIRE(K == NVB_K, "netvlad_backward: kernels are built for num_clusters = 64 (got %d)", K);
  OIBL_REQUIRE(C == NVB_C, "netvlad_backward: kernels are built for dim = 512 (got %d)", C);
  OIBL_REQUIRE(N > 0 && P > 0, "netvlad_backward: bad shape N=%d P=%d", N, P);
  OIBL_REQUIRE(N <= 65535, "netvlad_backward: at most 65535 images per call (got %d)", N);
  OIBL_REQUIRE((uintptr_t)feat % 16 == 0 && (uintptr_t)assign_w % 16 == 0 && (uintptr_t)centroids % 16 == 0 &&
                   (uintptr_t)grad_vlad_norm % 16 == 0 && (uintptr_t)grad_feat % 16 == 0,
               "netvlad_backward: feat, assign_w, centroids, grad_vlad_norm and grad_feat must be 16-byte aligned");
  const size_t need = oibl_netvlad_backward_workspace_bytes(N, P, K, C, grad_feat != nullptr);
  if ((uintptr_t)ws % 256 != 0) {
    set_error("netvlad_backward: workspace must be 256-byte aligned");
    return OIBL_E_WORKSPACE;
  }
  if (ws_bytes < need) {
    set_error("netvlad_backward: workspace %zu < required %zu bytes", ws_bytes, need);
    return OIBL_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* wsb = (char*)ws;
  const float* x = (const float*)feat;
  float* rn = (float*)wsb;
  float* a = (float*)(wsb + nvb_off_a(N, P));
  float* V = (float*)(wsb + nvb_off_v(N, P));
  double* stats = (double*)(wsb + nvb_off_st(N, P, K, C));
  double* A = (double*)(wsb + nvb_off_A(N, P, K, C));
  float* dvc = (float*)(wsb + nvb_off_dvc(N, P, K, C));
  float* dWp = (float*)(wsb + nvb_off_dwp(N, P, K, C));
  double* dCp = grad_centroids ? (double*)(wsb + nvb_off_dcp(N, P, K, C)) : nullptr;
  float* ds = grad_feat ? (float*)(wsb + nvb_off_ds(N, P, K, C)) : a;
  const dim3 pgrid((unsigned)((P + 31) / 32), (unsigned)N);
  const long vrows = (long)N * K;
  const unsigned rgrid = (unsigned)((vrows + 3) / 4);

  OIBL_SET_MAX_LDS(nvb_assign_kernel, NVB_ASSIGN_LDS);
  hipLaunchKernelGGL(nvb_assign_kernel, pgrid, dim3(256), NVB_ASSIGN_LDS, st, x, assign_w, rn, a, P, normalize_input);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(nvb_aggregate_kernel<0>, dim3((unsigned)N, C / 64), dim3(256), 0, st, x, (const float*)rn,
                     (const float*)a, centroids, V, A, P);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(nvb_rowstats_kernel, dim3(rgrid), dim3(256), 0, st, (const float*)V, grad_vlad_norm, stats, vrows);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(nvb_dv_kernel, dim3(rgrid), dim3(256), 0, st, V, grad_vlad_norm, (const double*)stats,
                     (const double*)A, centroids, dvc, dCp, vrows);
  OIBL_LAUNCH_CHECK();
  if (grad_assign_w || grad_feat) {
    OIBL_SET_MAX_LDS(nvb_contract_kernel, NVB_CONTRACT_LDS);
    hipLaunchKernelGGL(nvb_contract_kernel, pgrid, dim3(256), NVB_CONTRACT_LDS, st, x, (const float*)V,
                       (const float*)dvc, (const float*)rn, (const float*)a, ds, P);
    OIBL_LAUNCH_CHECK();
  }
  if (grad_assign_w) {
    hipLaunchKernelGGL(nvb_aggregate_kernel<1>, dim3((unsigned)N, C / 64), dim3(256), 0, st, x, (const float*)rn,
                       (const float*)ds, centroids, dWp, (double*)nullptr, P);
    OIBL_LAUNCH_CHECK();
  }
  if (grad_feat) {
    OIBL_SET_MAX_LDS(nvb_dx_kernel, NVB_DX_LDS);
    hipLaunchKernelGGL(nvb_dx_kernel, pgrid, dim3(256), NVB_DX_LDS, st, x, (const float*)rn, (const float*)a,
                       (const float*)ds, (const float*)V, assign_w, grad_feat, P, normalize_input);
    OIBL_LAUNCH_CHECK();
  }
  if (grad_assign_w || grad_centroids) {
    hipLaunchKernelGGL(nvb_reduce_kernel, dim3(NVB_K * NVB_C / 256), dim3(256), 0, st, (const float*)dWp,
                       (const double*)dCp, grad_assign_w, grad_centroids, N);
    OIBL_LAUNCH_CHECK();
  }
  return OIBL_OK;
}

}  // extern "C"
