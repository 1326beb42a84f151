// Gradients of the SFRS region head on gfx950: the backward of oibl_region_vlad_forward and oibl_region_scores, i.e.
// of EmbedRegionNet._compute_region_sim (ibl/models/netvlad.py:123-186) as torch autograd differentiates it when
// SFRSTrainer._forward (ibl/trainers.py:235-259) trains through it.
//
// Notation of netvlad_backward.hip's header; q(p) the quarter of pixel p, S_r the quarters of region r in the order
// [0123, 01, 23, 02, 13, 0, 1, 2, 3], eps = 1e-12:
//   forward    V_q,k = sum_{p in q} a_pk xh_p - A_q,k c_k        A_q,k = sum_{p in q} a_pk
//              R_r = sum_{q in S_r} V_q,  t_r,k = max(|R_r,k|, eps),  U_r,k = R_r,k / t_r,k
//              g_r = max(|U_r|_F, eps),   Y_r = U_r / g_r                     (region_vlad[n][r], k-major)
//   backward   dU_r = (G_r - Y_r <Y_r, G_r>) / g_r
//              dR_r,k = (dU_r,k - U_r,k <U_r,k, dU_r,k>) / t_r,k
//              dV_q = sum_{r : q in S_r} dR_r                                 (4 regions per quarter)
//              dC_k = - sum_q A_q,k dV_q,k                                    summed over the images
//              da_pk = <dV_q(p),k, xh_p> - <dV_q(p),k, c_k>,  ds_pk = a_pk (da_pk - sum_j a_pj da_pj)
//              dW_k = sum_p ds_pk xh_p                                        summed over the images
//              dxh_p = sum_k (a_pk dV_q(p),k + ds_pk w_k),  dx_p = (dxh_p - xh_p <xh_p, dxh_p>) / r_p
//   scores     dY[t,0][a]   = sum_j sum_b grad_score[t][j][a][b] Y[t,1+j][b]  (anchor)
//              dY[t,1+j][b] = sum_a grad_score[t][j][a][b] Y[t,0][a]          (pair j)
//   where a max(., eps) is active its denominator is a constant: the projection term is dropped.
//
// Per pixel this is the plain head's backward with dV taken from the pixel's quarter, behind a 9-region
// normalisation backward.  The call is stateless like oibl_netvlad_backward: nothing of the reference's
// residual[N*4][K][C][P/4] exists.  The workspace orders an image's pixels QUARTER-MAJOR (index j = q Pq + i, i the
// row-major index inside quarter q of Pq = h/2 w/2 pixels); a chunk is 32 consecutive pixels of ONE quarter, so a
// chunk has one dV.  A pixel is 2 KB contiguous in the NHWC map, so the gather costs no coalescing.
//   rgb_assign_kernel        one workgroup per (quarter, chunk): |x_p| and the logits in fp64    -> r, a[j][64]
//   rgb_aggregate_kernel<0>  one workgroup per (quarter, 64 channels), the quarter's pixels in order on
//                            v_mfma_f32_32x32x2_f32; A in fp64                                   -> V_q[K][C], A_q[K]
//   rgb_rowstats_kernel      one wave per (image, cluster): the 9 region rows from the 4 quarter rows, per region
//                            t, |U_k|^2, <U_k, G_k>
//   rgb_dv_kernel            one wave per (image, cluster): per region g, <Y, G> and the two scalars that dR_r,k is
//                            in G_r,k and R_r,k; the four dV_q (over V_q), <dV_q,k, c_k> and the image's dC row —
//                            these two kernels in fp64 throughout
//   rgb_contract_kernel      the chunk against its quarter's dV on the matrix cores: da, ds      -> ds[j][64]
//   rgb_aggregate_kernel<1>  one workgroup per (image, 64 channels) over ALL the image's pixels (dW does not care
//                            for quarters), ds in the place of a                                 -> dW of the image
//   rgb_dx_kernel            dxh = [a | ds] . [dV_q ; w] per chunk, the projection, the division -> grad_feat
//   rgb_reduce_kernel        dW = sum_n dW_n (fp32), dC = sum_n dC_n (fp64, rounded once), in image order
//   rgb_scores_kernel        one thread per float4 of an image's 9 vectors, fp64 accumulators, fixed order
// No floating-point atomics; the decomposition depends on (h, w) alone, so results are bit-identical from run to run
// and an image's grad_feat rows do not depend on its batch mates.  V / dW, da and dxh are exact fp32 on the matrix
// cores; what feeds dC (logits, norms, both normalisations' backward, the per-image dC) is fp64 for the reason given
// in netvlad_backward.hip: the loss_soft and tuple-loss gradients sum to zero over a tuple, the images' dC cancel.
//
// The chunk kernels repeat netvlad_backward.hip's bodies instead of sharing them through a header: that file's
// outputs are pinned bit for bit, and the two differ in how a pixel index becomes an address, which dV a chunk
// contracts against and which grid axis carries the image (4 N quarters do not fit a grid's y).
#include "gemm_core.h"

namespace oibl {

constexpr int RGB_C = 512;
constexpr int RGB_K = 64;
constexpr int RGB_XP = 516;          // floats per LDS row of the chunk: 16-byte aligned, +4 banks per pixel
constexpr int RGB_LP = 65;           // pitch of the [32][64] partial tiles
constexpr int RGB_AP = 129;          // pitch of the [32][128] operand tile [a | ds]
constexpr int RGB_WP = 132;          // floats per LDS row of the weight slice
constexpr int RGB_ASSIGN_LDS = (32 * RGB_XP + RGB_K * RGB_WP + 32) * 4;
constexpr int RGB_CONTRACT_LDS = (32 * RGB_XP + 4 * 32 * RGB_LP + 32 + 32) * 4;
constexpr int RGB_DX_LDS = (32 * RGB_XP + 32 * RGB_AP + 4 * 32 + 32 + 32 + 32) * 4;
constexpr float RGB_EPS = 1e-12f;
// the quarters of the 9 regions as bit masks
__device__ constexpr int RGB_MEMBERS[9] = {0xF, 0x3, 0xC, 0x5, 0xA, 0x1, 0x2, 0x4, 0x8};

__device__ static inline double rgb_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the map pixel (row-major in the h x w map) of pixel i of quarter q
__device__ static inline int rgb_map_pixel(int q, int i, int hq, int wq) {
  const int row = i / wq, col = i - row * wq;
  return ((q >> 1) * hq + row) * (2 * wq) + (q & 1) * wq + col;
}

// pix_s[t] = map pixel of pixel p0 + t of quarter q, -1 beyond the quarter (threads 0..31; the caller synchronises)
__device__ static inline void rgb_chunk_pixels(int q, int p0, int hq, int wq, int* pix_s) {
  if (threadIdx.x < 32) {
    const int i = p0 + (int)threadIdx.x;
    pix_s[threadIdx.x] = i < hq * wq ? rgb_map_pixel(q, i, hq, wq) : -1;
  }
}

// the 32 pixels named by pix_s of one image -> x_s[32][RGB_XP]; pixels beyond the quarter read as zeros
__device__ static inline void rgb_load_chunk(const float* __restrict__ fimg, const int* pix_s, float* x_s) {
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int idx = (int)threadIdx.x + 256 * q;          // float4 index inside the chunk
    const int px = idx >> 7, c4 = (idx & 127) * 4;
    const int mp = pix_s[px];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mp >= 0) v = *reinterpret_cast<const float4*>(fimg + (size_t)mp * RGB_C + c4);
    *reinterpret_cast<float4*>(x_s + px * RGB_XP + c4) = v;
  }
}

// nvb_assign_kernel on one chunk of one quarter: rn[j] = |x_p| (1 without normalize), a[j][k] = softmax_k(w_k . xh_p),
// norm and logits accumulated in fp64 on the vector unit.  blockIdx.x = 4 n + q, blockIdx.y the chunk.
__global__ __launch_bounds__(256) void rgb_assign_kernel(const float* __restrict__ feat, const float* __restrict__ w,
                                                         float* __restrict__ rn, float* __restrict__ a, int hq, int wq,
                                                         int normalize) {
  constexpr int C = RGB_C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const x_s = reinterpret_cast<float*>(smem);             // [32][RGB_XP]
  float* const w_s = x_s + 32 * RGB_XP;                           // [64 clusters][RGB_WP]: 128 channels of a slice
  int* const pix_s = reinterpret_cast<int*>(w_s + RGB_K * RGB_WP);  // [32]
  const int Pq = hq * wq;
  const int m = blockIdx.x, p0 = blockIdx.y * 32;
  const int px = (int)threadIdx.x >> 3, sub = (int)threadIdx.x & 7;
  rgb_chunk_pixels(m & 3, p0, hq, wq, pix_s);
  __syncthreads();
  rgb_load_chunk(feat + (size_t)(m >> 2) * 4 * Pq * C, pix_s, x_s);
  double acc[8], ss = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.0;
  for (int c0 = 0; c0 < C; c0 += 128) {
    __syncthreads();                                              // the chunk is in LDS / the last slice is consumed
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = (int)threadIdx.x + 256 * q;
      const int c4 = idx & 31, k = idx >> 5;
      *reinterpret_cast<float4*>(w_s + k * RGB_WP + 4 * c4) =
          *reinterpret_cast<const float4*>(w + (size_t)k * C + c0 + 4 * c4);
    }
    __syncthreads();
    const float* xr = x_s + px * RGB_XP + c0;
    const float* wr = w_s + sub * RGB_WP;
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
        const float4 wv = *reinterpret_cast<const float4*>(wr + 8 * j * RGB_WP + c);
        acc[j] = fma(x0, (double)wv.x, acc[j]);
        acc[j] = fma(x1, (double)wv.y, acc[j]);
        acc[j] = fma(x2, (double)wv.z, acc[j]);
        acc[j] = fma(x3, (double)wv.w, acc[j]);
      }
    }
  }
  const double rd = normalize ? sqrt(ss) : 1.0;
  const double invd = 1.0 / fmax(rd, (double)RGB_EPS);
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
  if (p0 + px < Pq) {
    const size_t j = (size_t)m * Pq + p0 + px;
    float* dst = a + j * RGB_K + sub;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) dst[8 * jj] = l[jj] * is;
    if (sub == 0) rn[j] = (float)rd;
  }
}

// nvb_contract_kernel on one chunk of one quarter against that quarter's dV (B[m]): ds[j][k].  `out` may alias `a`.
__global__ __launch_bounds__(256) void rgb_contract_kernel(const float* __restrict__ feat, const float* __restrict__ B,
                                                           const float* __restrict__ dvc, const float* __restrict__ rn,
                                                           const float* a, float* out, int hq, int wq) {
  constexpr int C = RGB_C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const x_s = reinterpret_cast<float*>(smem);             // [32][RGB_XP]
  float* const lp_s = x_s + 32 * RGB_XP;                          // [4 waves][32][RGB_LP]
  float* const inv_s = lp_s + 4 * 32 * RGB_LP;                    // [32]
  int* const pix_s = reinterpret_cast<int*>(inv_s + 32);          // [32]
  const int Pq = hq * wq;
  const int m = blockIdx.x, p0 = blockIdx.y * 32;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l31 = lane & 31, kh = lane >> 5;
  B += (size_t)m * RGB_K * C;

  rgb_chunk_pixels(m & 3, p0, hq, wq, pix_s);
  if (threadIdx.x < 32) {
    const int p = p0 + (int)threadIdx.x;
    inv_s[threadIdx.x] = p < Pq ? 1.0f / fmaxf(rn[(size_t)m * Pq + p], RGB_EPS) : 0.f;
  }
  __syncthreads();
  rgb_load_chunk(feat + (size_t)(m >> 2) * 4 * Pq * C, pix_s, x_s);
  __syncthreads();
  {  // partial contraction over this wave's 128 channels: [32 pixels] x [64 rows of B]
    f32x16_t lg[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) lg[ct][r] = 0.f;
    const float* xa = x_s + l31 * RGB_XP + 128 * wave + 4 * kh;
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
    float* lw = lp_s + wave * 32 * RGB_LP;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) lw[acc_row(r, lane) * RGB_LP + 32 * ct + l31] = lg[ct][r];
  }
  __syncthreads();
  {  // eight threads per pixel, eight clusters each
    const int px = (int)threadIdx.x >> 3, sub = (int)threadIdx.x & 7;
    const float iv = inv_s[px];
    const bool live = p0 + px < Pq;
    float l[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int o = px * RGB_LP + sub * 8 + k;
      l[k] = (lp_s[o] + lp_s[32 * RGB_LP + o] + lp_s[2 * 32 * RGB_LP + o] + lp_s[3 * 32 * RGB_LP + o]) * iv;
    }
    const size_t off = ((size_t)m * Pq + p0 + px) * RGB_K + sub * 8;
    float av[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) av[k] = 0.f;
    if (live) {
      const float4 a0 = *reinterpret_cast<const float4*>(a + off), a1 = *reinterpret_cast<const float4*>(a + off + 4);
      av[0] = a0.x; av[1] = a0.y; av[2] = a0.z; av[3] = a0.w;
      av[4] = a1.x; av[5] = a1.y; av[6] = a1.z; av[7] = a1.w;
    }
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      l[k] -= dvc[(size_t)m * RGB_K + sub * 8 + k];
      dot = fmaf(av[k], l[k], dot);
    }
    dot += __shfl_xor(dot, 1, 64);
    dot += __shfl_xor(dot, 2, 64);
    dot += __shfl_xor(dot, 4, 64);
    if (live) {
      *reinterpret_cast<float4*>(out + off) = make_float4(av[0] * (l[0] - dot), av[1] * (l[1] - dot),
                                                          av[2] * (l[2] - dot), av[3] * (l[3] - dot));
      *reinterpret_cast<float4*>(out + off + 4) = make_float4(av[4] * (l[4] - dot), av[5] * (l[5] - dot),
                                                              av[6] * (l[6] - dot), av[7] * (l[7] - dot));
    }
  }
}

// out[s][k][c0..c0+63] = sum_p a[p][k] xh[p][c] over segment s of `seg_px` quarter-major pixels, in order; `segs`
// segments per image.  MODE 0 (segs 4, a segment is a quarter): minus A_k centroids[k][c], and A[s][k] = sum_p a[p][k]
// in fp64 (slice 0 writes it).  MODE 1 (segs 1, the whole image; a = ds): the plain sum, the image's dW.
// 4 waves as 2 (clusters) x 2 (channels), one 32x32 fp32 accumulator tile each.
template <int MODE>
__global__ __launch_bounds__(256) void rgb_aggregate_kernel(const float* __restrict__ feat,
                                                            const float* __restrict__ rn, const float* __restrict__ a,
                                                            const float* __restrict__ centroids,
                                                            float* __restrict__ out, double* __restrict__ A, int hq,
                                                            int wq, int segs, int seg_px) {
  constexpr int C = RGB_C;
  __shared__ __attribute__((aligned(16))) float a_s[32][64];
  __shared__ __attribute__((aligned(16))) float x_s[32][64];
  __shared__ float s_sum[64];
  const int Pq = hq * wq;
  const int s = blockIdx.x, c0 = blockIdx.y * 64;
  const int n = s / segs, j0 = (s - n * segs) * seg_px;         // first quarter-major pixel of the segment
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const float* fbase = feat + (size_t)n * 4 * Pq * C + c0;
  const float* abase = a + ((size_t)n * 4 * Pq + j0) * 64;
  const float* rbase = rn + (size_t)n * 4 * Pq + j0;

  f32x16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  double colsum = 0.0;  // threads 0..63: sum_p a[p][tid]

  const int xp = threadIdx.x >> 3, xc = (threadIdx.x & 7) * 8;
  float4 pa[2], px0, px1;
  float psc;
  auto prefetch = [&](int p0) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = threadIdx.x + q * 256;  // float4 index
      const int pr = idx >> 4, cq = (idx & 15) * 4;
      pa[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p0 + pr < seg_px) pa[q] = *reinterpret_cast<const float4*>(abase + (size_t)(p0 + pr) * 64 + cq);
    }
    px0 = make_float4(0.f, 0.f, 0.f, 0.f);
    px1 = px0;
    psc = 0.f;
    if (p0 + xp < seg_px) {
      const int j = j0 + p0 + xp, q = j / Pq;
      psc = 1.0f / fmaxf(rbase[p0 + xp], RGB_EPS);
      const float* src = fbase + (size_t)rgb_map_pixel(q, j - q * Pq, hq, wq) * C + xc;
      px0 = *reinterpret_cast<const float4*>(src);
      px1 = *reinterpret_cast<const float4*>(src + 4);
    }
  };
  prefetch(0);
  for (int p0 = 0; p0 < seg_px; p0 += 32) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int idx = threadIdx.x + q * 256;
      *reinterpret_cast<float4*>(&a_s[idx >> 4][(idx & 15) * 4]) = pa[q];
    }
    *reinterpret_cast<float4*>(&x_s[xp][xc]) = make_float4(px0.x * psc, px0.y * psc, px0.z * psc, px0.w * psc);
    *reinterpret_cast<float4*>(&x_s[xp][xc + 4]) = make_float4(px1.x * psc, px1.y * psc, px1.z * psc, px1.w * psc);
    __syncthreads();
    if (p0 + 32 < seg_px) prefetch(p0 + 32);
    if (MODE == 0 && threadIdx.x < 64) {
#pragma unroll
      for (int p = 0; p < 32; ++p) colsum += (double)a_s[p][threadIdx.x];
    }
#pragma unroll
    for (int st = 0; st < 16; ++st) {
      const int p = 2 * st + (lane >> 5);
      const float av = a_s[p][wm * 32 + (lane & 31)];
      const float bv = x_s[p][wn * 32 + (lane & 31)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  if (MODE == 0) {
    if (threadIdx.x < 64) {
      s_sum[threadIdx.x] = (float)colsum;
      if (blockIdx.y == 0) A[(size_t)s * 64 + threadIdx.x] = colsum;
    }
    __syncthreads();
  }
  const int ch = c0 + wn * 32 + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int k = wm * 32 + acc_row(r, lane);
    float v = acc[r];
    if (MODE == 0) v -= s_sum[k] * centroids[(size_t)k * C + ch];
    out[((size_t)s * 64 + k) * C + ch] = v;
  }
}

// one wave per (image, cluster): the region rows R_r,k = sum_{q in S_r} V_q,k in fp64 from the four fp32 quarter rows,
// st[(n 9 + r) K + k] = { |R_r,k| , |U_r,k|^2 , <U_r,k, G_r,k> }
__global__ __launch_bounds__(256) void rgb_rowstats_kernel(const float* __restrict__ V, const float* __restrict__ G,
                                                           double* __restrict__ st, long rows) {
  constexpr int C = RGB_C, K = RGB_K;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long n = row / K;
  const int k = (int)(row - n * K);
  float vq[4][8];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float* v = V + ((n * 4 + q) * K + k) * C;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float4 a = *reinterpret_cast<const float4*>(v + 256 * h + 4 * lane);
      vq[q][4 * h] = a.x; vq[q][4 * h + 1] = a.y; vq[q][4 * h + 2] = a.z; vq[q][4 * h + 3] = a.w;
    }
  }
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const long rrow = (n * 9 + r) * K + k;
    const float* g = G + rrow * C;
    double rr[8], gg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      rr[i] = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (RGB_MEMBERS[r] >> q & 1) rr[i] += (double)vq[q][i];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float4 b = *reinterpret_cast<const float4*>(g + 256 * h + 4 * lane);
      gg[4 * h] = b.x; gg[4 * h + 1] = b.y; gg[4 * h + 2] = b.z; gg[4 * h + 3] = b.w;
    }
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) ss += rr[i] * rr[i];
    ss = rgb_wave_sum_f64(ss);
    const double t = sqrt(ss);
    const double it = 1.0 / fmax(t, (double)RGB_EPS);
    double s2 = 0.0, ug = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double u = rr[i] * it;
      s2 += u * u;
      ug += u * gg[i];
    }
    s2 = rgb_wave_sum_f64(s2);
    ug = rgb_wave_sum_f64(ug);
    if (lane == 0) {
      st[3 * rrow] = t;
      st[3 * rrow + 1] = s2;
      st[3 * rrow + 2] = ug;
    }
  }
}

// one wave per (image, cluster): the 9 regions' dR_r,k, added into the four dV_q,k of their quarters (region order),
// V_q,k -> dV_q,k in place (fp32, the operand of the later contractions), dvc[(4 n + q) K + k] = <dV_q,k, c_k>, and,
// where dCp is given, the image's dC row -sum_q A_q,k dV_q,k in fp64.  Both normalisations' backward of a region row
// collapse to two scalars, dR_r,k = al_r G_r,k - be_r R_r,k: with u = R / t and the row's stats s2 = |U_r,k|^2,
// ug = <U_r,k, G_r,k>,
//   dU = G / g - u <Y, G> / g^2,  <u, dU> = (ug - s2 <Y, G> / g) / g,  dR = (dU - u <u, dU>) / t
// so the row is walked once, in two halves of 256 channels, with no cross-lane step inside.
__global__ __launch_bounds__(256) void rgb_dv_kernel(float* __restrict__ V, const float* __restrict__ G,
                                                     const double* __restrict__ st, const double* __restrict__ A,
                                                     const float* __restrict__ centroids, float* __restrict__ dvc,
                                                     double* __restrict__ dCp, long rows) {
  constexpr int C = RGB_C, K = RGB_K;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long n = row / K;
  const int k = (int)(row - n * K);
  double al[9], be[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const long vbase = (n * 9 + r) * K;                             // the region vector's first row
    // |U_r|_F^2 and <U_r, G_r>: lane j holds cluster j's, the same fixed-order sum in every wave of the image
    const double S2 = rgb_wave_sum_f64(st[3 * (vbase + lane) + 1]);
    const double UG = rgb_wave_sum_f64(st[3 * (vbase + lane) + 2]);
    const double gn = sqrt(S2);
    const double ig = 1.0 / fmax(gn, (double)RGB_EPS);
    const double yg = gn < (double)RGB_EPS ? 0.0 : UG * ig;         // <Y_r, G_r>; a clamped g is a constant
    const double t = st[3 * (vbase + k)], s2 = st[3 * (vbase + k) + 1], ug = st[3 * (vbase + k) + 2];
    const double it = 1.0 / fmax(t, (double)RGB_EPS);
    const double fd = t < (double)RGB_EPS ? 0.0 : (ug - s2 * ig * yg) * ig;   // <U_r,k, dU_r,k>; a clamped t likewise
    al[r] = ig * it;
    be[r] = (ig * ig * yg + fd) * it * it;
  }
  double na[4], dc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    na[q] = dCp != nullptr ? -A[(n * 4 + q) * K + k] : 0.0;
    dc[q] = 0.0;
  }
#pragma unroll 1
  for (int h = 0; h < 2; ++h) {
    const int co = 256 * h + 4 * lane;
    double vq[4][4], dvq[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(V + ((n * 4 + q) * K + k) * C + co);
      vq[q][0] = v.x; vq[q][1] = v.y; vq[q][2] = v.z; vq[q][3] = v.w;
#pragma unroll
      for (int i = 0; i < 4; ++i) dvq[q][i] = 0.0;
    }
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      const float4 b = *reinterpret_cast<const float4*>(G + ((n * 9 + r) * K + k) * C + co);
      const double gg[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double rr = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (RGB_MEMBERS[r] >> q & 1) rr += vq[q][i];
        const double dr = al[r] * gg[i] - be[r] * rr;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (RGB_MEMBERS[r] >> q & 1) dvq[q][i] += dr;
      }
    }
    const float4 cv = *reinterpret_cast<const float4*>(centroids + (size_t)k * C + co);
    const double cc[4] = {cv.x, cv.y, cv.z, cv.w};
    double dcr[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        dc[q] += dvq[q][i] * cc[i];
        dcr[i] += na[q] * dvq[q][i];
      }
      *reinterpret_cast<float4*>(V + ((n * 4 + q) * K + k) * C + co) =
          make_float4((float)dvq[q][0], (float)dvq[q][1], (float)dvq[q][2], (float)dvq[q][3]);
    }
    if (dCp != nullptr) {
      double* o = dCp + row * C + co;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = dcr[i];
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double s = rgb_wave_sum_f64(dc[q]);
    if (lane == 0) dvc[(n * 4 + q) * K + k] = (float)s;
  }
}

// nvb_dx_kernel on one chunk of one quarter: dxh[p][c] = sum_k a[p][k] dV_q[k][c] + sum_k ds[p][k] w[k][c], then
// dx_p = (dxh_p - xh_p <xh_p, dxh_p>) / r_p, written to the pixel's place in the map.
__global__ __launch_bounds__(256) void rgb_dx_kernel(const float* __restrict__ feat, const float* __restrict__ rn,
                                                     const float* __restrict__ a, const float* __restrict__ ds,
                                                     const float* __restrict__ dV, const float* __restrict__ w,
                                                     float* __restrict__ grad_feat, int hq, int wq, int normalize) {
  constexpr int C = RGB_C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const x_s = reinterpret_cast<float*>(smem);             // [32][RGB_XP]
  float* const ad_s = x_s + 32 * RGB_XP;                          // [32][RGB_AP]: a | ds
  float* const red_s = ad_s + 32 * RGB_AP;                        // [4 waves][32]
  float* const inv_s = red_s + 4 * 32;                            // [32]
  float* const dot_s = inv_s + 32;                                // [32]
  int* const pix_s = reinterpret_cast<int*>(dot_s + 32);          // [32]
  const int Pq = hq * wq;
  const int m = blockIdx.x, p0 = blockIdx.y * 32;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l31 = lane & 31, kh = lane >> 5;
  const size_t jbase = (size_t)m * Pq;
  dV += (size_t)m * RGB_K * C;

  rgb_chunk_pixels(m & 3, p0, hq, wq, pix_s);
  if (threadIdx.x < 32) {
    const int p = p0 + (int)threadIdx.x;
    inv_s[threadIdx.x] = p < Pq ? 1.0f / fmaxf(rn[jbase + p], RGB_EPS) : 0.f;
    // the projection is dropped where the input is not normalised or its norm sits on the clamp
    dot_s[threadIdx.x] = 0.f;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {                                   // 32 x 128 floats = 1024 float4
    const int idx = (int)threadIdx.x + 256 * q;
    const int px = idx >> 5, k4 = (idx & 31) * 4;                 // k4 < 64: a, else ds
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p0 + px < Pq) {
      const float* src = (k4 < 64 ? a : ds) + (jbase + p0 + px) * RGB_K + (k4 & 63);
      v = *reinterpret_cast<const float4*>(src);
    }
    float* d = ad_s + px * RGB_AP + k4;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  __syncthreads();
  rgb_load_chunk(feat + (size_t)(m >> 2) * 4 * Pq * C, pix_s, x_s);
  __syncthreads();

  f32x16_t acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
  const float* arow = ad_s + l31 * RGB_AP + kh;
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
      for (int ct = 0; ct < 4; ++ct) v = fmaf(acc[ct][r], x_s[px * RGB_XP + cb + 32 * ct], v);
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
      const bool clamped = p < Pq ? rn[jbase + p] < RGB_EPS : true;
      const float d = ((red_s[threadIdx.x] + red_s[32 + threadIdx.x]) + red_s[64 + threadIdx.x]) + red_s[96 + threadIdx.x];
      dot_s[threadIdx.x] = clamped ? 0.f : d * iv * iv;         // <xh_p, dxh_p> / r_p: it multiplies x_p below
    }
    __syncthreads();
  }
  float* gimg = grad_feat + (size_t)(m >> 2) * 4 * Pq * C;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int px = acc_row(r, lane);
    const int mp = pix_s[px];
    if (mp >= 0) {
      const float iv = inv_s[px], d = dot_s[px];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int ch = cb + 32 * ct;
        gimg[(size_t)mp * C + ch] = (acc[ct][r] - x_s[px * RGB_XP + ch] * d) * iv;
      }
    }
  }
}

// dW = sum_n dWp[n] (fp32), dC = sum_n dCp[n] (fp64, rounded once), both in image order; either output may be null
__global__ __launch_bounds__(256) void rgb_reduce_kernel(const float* __restrict__ dWp, const double* __restrict__ dCp,
                                                         float* __restrict__ dW, float* __restrict__ dC, int N) {
  constexpr int KC = RGB_K * RGB_C;
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

// The scores' backward: workgroup (float4 block of L, image i of the tuple, tuple t); a thread owns one float4 of
// each of the image's 9 gradient vectors.  Pair j = i - 1: dY[b] = sum_a gs[t][j][a][b] Y[t,0][a].  Anchor (i = 0):
// dY[a] = sum_j sum_b gs[t][j][a][b] Y[t,1+j][b], the pairs in order.  fp64 accumulators, rounded once; a pair's rows
// read the anchor's vectors and that pair's table only.
__global__ __launch_bounds__(256) void rgb_scores_kernel(const float* __restrict__ vec, int per, int L,
                                                         const float* __restrict__ gs, float* __restrict__ out) {
  __shared__ float g_s[81];
  const int i = blockIdx.y, t = blockIdx.z;
  const int l = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
  const int n = per - 1;
  const float* Yt = vec + (size_t)t * per * 9 * L;
  double acc[9][4];
#pragma unroll
  for (int o = 0; o < 9; ++o)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[o][e] = 0.0;
  const int j_lo = i == 0 ? 0 : i - 1, j_hi = i == 0 ? n : i;
  for (int j = j_lo; j < j_hi; ++j) {
    __syncthreads();
    if (threadIdx.x < 81) g_s[threadIdx.x] = gs[((size_t)t * n + j) * 81 + threadIdx.x];
    __syncthreads();
    if (l < L) {
      const float* src = Yt + (size_t)(i == 0 ? 1 + j : 0) * 9 * L + l;
#pragma unroll
      for (int s = 0; s < 9; ++s) {
        const float4 y = *reinterpret_cast<const float4*>(src + (size_t)s * L);
#pragma unroll
        for (int o = 0; o < 9; ++o) {
          // anchor: output region a = o, source region b = s; pair: output region b = o, source region a = s
          const double gv = (double)(i == 0 ? g_s[o * 9 + s] : g_s[s * 9 + o]);
          acc[o][0] = fma(gv, (double)y.x, acc[o][0]);
          acc[o][1] = fma(gv, (double)y.y, acc[o][1]);
          acc[o][2] = fma(gv, (double)y.z, acc[o][2]);
          acc[o][3] = fma(gv, (double)y.w, acc[o][3]);
        }
      }
    }
  }
  if (l < L) {
    float* dst = out + ((size_t)t * per + i) * 9 * L + l;
#pragma unroll
    for (int o = 0; o < 9; ++o)
      *reinterpret_cast<float4*>(dst + (size_t)o * L) =
          make_float4((float)acc[o][0], (float)acc[o][1], (float)acc[o][2], (float)acc[o][3]);
  }
}

}  // namespace oibl

using namespace oibl;

extern "C" {

// workspace, P = h w, M = 4 N quarters: r [N][P] | a [N][P][64] (quarter-major) | V_q -> dV_q [M][K][C] |
//            stats [N][9][K][3] fp64 | A [M][K] fp64 | dvc [M][K] | dW of every image [N][K][C] |
//            dC of every image [N][K][C] fp64 | ds [N][P][64] (only with grad_feat: without it ds overwrites a)
static size_t rgb_off_a(size_t N, size_t P) { return align_up(N * P * sizeof(float), 256); }
static size_t rgb_off_v(size_t N, size_t P) { return rgb_off_a(N, P) + align_up(N * P * 64 * sizeof(float), 256); }
static size_t rgb_off_st(size_t N, size_t P) {
  return rgb_off_v(N, P) + align_up(4 * N * RGB_K * RGB_C * sizeof(float), 256);
}
static size_t rgb_off_A(size_t N, size_t P) { return rgb_off_st(N, P) + align_up(N * 9 * RGB_K * 3 * sizeof(double), 256); }
static size_t rgb_off_dvc(size_t N, size_t P) { return rgb_off_A(N, P) + align_up(4 * N * RGB_K * sizeof(double), 256); }
static size_t rgb_off_dwp(size_t N, size_t P) { return rgb_off_dvc(N, P) + align_up(4 * N * RGB_K * sizeof(float), 256); }
static size_t rgb_off_dcp(size_t N, size_t P) {
  return rgb_off_dwp(N, P) + align_up(N * RGB_K * RGB_C * sizeof(float), 256);
}
static size_t rgb_off_ds(size_t N, size_t P) {
  return rgb_off_dcp(N, P) + align_up(N * RGB_K * RGB_C * sizeof(double), 256);
}
static bool rgb_shape_ok(int N, int h, int w, int K, int C) {
  return N > 0 && N <= 65535 && h >= 2 && w >= 2 && !(h & 1) && !(w & 1) && K == RGB_K && C == RGB_C &&
         (long)h * w <= (1L << 22);            // chunks per quarter are a grid's y; N h w stays far below 2^31 rows
}

size_t oibl_region_backward_workspace_bytes(int N, int h, int w, int K, int C, int want_grad_feat) {
  if (!rgb_shape_ok(N, h, w, K, C)) return 0;
  const size_t P = (size_t)h * w;
  return rgb_off_ds(N, P) + (want_grad_feat ? align_up((size_t)N * P * 64 * sizeof(float), 256) : 0);
}

int oibl_region_vlad_backward(const void* feat, int N, int h, int w, int K, int C, int precision,
                              const float* assign_w, const float* centroids, int normalize_input,
                              const float* grad_region_vlad, float* grad_assign_w, float* grad_centroids,
                              float* grad_feat, void* ws, size_t ws_bytes, void* stream) {
  OIBL_REQUIRE(feat && assign_w && centroids && grad_region_vlad && ws, "region_vlad_backward: null pointer");
  OIBL_REQUIRE(grad_assign_w || grad_centroids || grad_feat, "region_vlad_backward: no output requested");
  OIBL_REQUIRE(precision == OIBL_F32, "region_vlad_backward: the feature map must be fp32 (OIBL_F32), got precision %d",
               precision);
  OIBL_REQUIRE(K == RGB_K && C == RGB_C,
               "region_vlad_backward: kernels are built for num_clusters = 64, dim = 512 (got %d, %d)", K, C);
  OIBL_REQUIRE(N > 0 && h > 0 && w > 0, "region_vlad_backward: bad shape N=%d h=%d w=%d", N, h, w);
  OIBL_REQUIRE(!(h & 1) && !(w & 1), "region_vlad_backward: the map is %d x %d, both sides must be even to cut quarters",
               h, w);
  OIBL_REQUIRE(N <= 65535, "region_vlad_backward: at most 65535 images per call (got %d)", N);
  OIBL_REQUIRE(rgb_shape_ok(N, h, w, K, C), "region_vlad_backward: map %d x %d too large", h, w);
  OIBL_REQUIRE((uintptr_t)feat % 16 == 0 && (uintptr_t)assign_w % 16 == 0 && (uintptr_t)centroids % 16 == 0 &&
                   (uintptr_t)grad_region_vlad % 16 == 0 && (uintptr_t)grad_feat % 16 == 0,
               "region_vlad_backward: feat, assign_w, centroids, grad_region_vlad and grad_feat must be 16-byte aligned");
  const size_t need = oibl_region_backward_workspace_bytes(N, h, w, K, C, grad_feat != nullptr);
  if ((uintptr_t)ws % 256 != 0) {
    set_error("region_vlad_backward: workspace must be 256-byte aligned");
    return OIBL_E_WORKSPACE;
  }
  if (ws_bytes < need) {
    set_error("region_vlad_backward: workspace %zu < required %zu bytes", ws_bytes, need);
    return OIBL_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* wsb = (char*)ws;
  const float* x = (const float*)feat;
  const int hq = h / 2, wq = w / 2, Pq = hq * wq;
  const size_t P = (size_t)h * w;
  float* rn = (float*)wsb;
  float* a = (float*)(wsb + rgb_off_a(N, P));
  float* V = (float*)(wsb + rgb_off_v(N, P));
  double* stats = (double*)(wsb + rgb_off_st(N, P));
  double* A = (double*)(wsb + rgb_off_A(N, P));
  float* dvc = (float*)(wsb + rgb_off_dvc(N, P));
  float* dWp = (float*)(wsb + rgb_off_dwp(N, P));
  double* dCp = grad_centroids ? (double*)(wsb + rgb_off_dcp(N, P)) : nullptr;
  float* ds = grad_feat ? (float*)(wsb + rgb_off_ds(N, P)) : a;
  const dim3 pgrid((unsigned)(4 * N), (unsigned)((Pq + 31) / 32));
  const long vrows = (long)N * K;
  const unsigned rgrid = (unsigned)((vrows + 3) / 4);

  OIBL_SET_MAX_LDS(rgb_assign_kernel, RGB_ASSIGN_LDS);
  hipLaunchKernelGGL(rgb_assign_kernel, pgrid, dim3(256), RGB_ASSIGN_LDS, st, x, assign_w, rn, a, hq, wq,
                     normalize_input);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(rgb_aggregate_kernel<0>, dim3((unsigned)(4 * N), C / 64), dim3(256), 0, st, x, (const float*)rn,
                     (const float*)a, centroids, V, A, hq, wq, 4, Pq);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(rgb_rowstats_kernel, dim3(rgrid), dim3(256), 0, st, (const float*)V, grad_region_vlad, stats,
                     vrows);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(rgb_dv_kernel, dim3(rgrid), dim3(256), 0, st, V, grad_region_vlad, (const double*)stats,
                     (const double*)A, centroids, dvc, dCp, vrows);
  OIBL_LAUNCH_CHECK();
  if (grad_assign_w || grad_feat) {
    OIBL_SET_MAX_LDS(rgb_contract_kernel, RGB_CONTRACT_LDS);
    hipLaunchKernelGGL(rgb_contract_kernel, pgrid, dim3(256), RGB_CONTRACT_LDS, st, x, (const float*)V,
                       (const float*)dvc, (const float*)rn, (const float*)a, ds, hq, wq);
    OIBL_LAUNCH_CHECK();
  }
  if (grad_assign_w) {
    hipLaunchKernelGGL(rgb_aggregate_kernel<1>, dim3((unsigned)N, C / 64), dim3(256), 0, st, x, (const float*)rn,
                       (const float*)ds, centroids, dWp, (double*)nullptr, hq, wq, 1, 4 * Pq);
    OIBL_LAUNCH_CHECK();
  }
  if (grad_feat) {
    OIBL_SET_MAX_LDS(rgb_dx_kernel, RGB_DX_LDS);
    hipLaunchKernelGGL(rgb_dx_kernel, pgrid, dim3(256), RGB_DX_LDS, st, x, (const float*)rn, (const float*)a,
                       (const float*)ds, (const float*)V, assign_w, grad_feat, hq, wq, normalize_input);
    OIBL_LAUNCH_CHECK();
  }
  if (grad_assign_w || grad_centroids) {
    hipLaunchKernelGGL(rgb_reduce_kernel, dim3(RGB_K * RGB_C / 256), dim3(256), 0, st, (const float*)dWp,
                       (const double*)dCp, grad_assign_w, grad_centroids, N);
    OIBL_LAUNCH_CHECK();
  }
  return OIBL_OK;
}

int oibl_region_scores_backward(const float* region_vlad, int T, int per_tuple, int L, const float* grad_score,
                                float* grad_region_vlad, void* stream) {
  OIBL_REQUIRE(region_vlad && grad_score && grad_region_vlad, "region_scores_backward: null pointer");
  OIBL_REQUIRE(T > 0 && T <= 65535, "region_scores_backward: bad tuple count %d", T);
  OIBL_REQUIRE(per_tuple >= 2 && per_tuple <= 65535,
               "region_scores_backward: a tuple needs an anchor and at least one pair (got %d images per tuple)",
               per_tuple);
  OIBL_REQUIRE(L > 0 && L % 4 == 0, "region_scores_backward: vector length must be a multiple of 4 (got %d)", L);
  OIBL_REQUIRE((uintptr_t)region_vlad % 16 == 0 && (uintptr_t)grad_region_vlad % 16 == 0,
               "region_scores_backward: region_vlad and grad_region_vlad must be 16-byte aligned");
  hipLaunchKernelGGL(rgb_scores_kernel, dim3((unsigned)((L / 4 + 255) / 256), (unsigned)per_tuple, (unsigned)T),
                     dim3(256), 0, (hipStream_t)stream, region_vlad, per_tuple, L, grad_score, grad_region_vlad);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

}  // extern "C"
