// The K-general NetVLAD descriptor head on gfx950: forward and gradients for num_clusters = 16, 32, ..., 128
// (dim = 512, fp32 NHWC map).  The formulas are netvlad_backward.hip's header, the contract is that of netvlad.hip /
// netvlad_backward.hip: stateless, exact fp32 on v_mfma_f32_32x32x2_f32 for the matrix work, fp64 for
// what feeds grad_centroids, no floating-point atomics, every sum in a fixed order.  The tuned K = 64 kernels are not
// touched; these are slower per cluster (nothing is kept in registers across chunks, one accumulator tile at a time).
//
// K is a run-time argument.  KP = K rounded up to 32 is the pitch of the workspace rows a[.][KP] and ds[.][KP]; their
// columns K..KP-1 hold zeros, the padded weight / dV rows are fed to the matrix cores as zeros and never read from
// memory, and max, exp and sum of the softmax run over the K live columns only.  KT = KP / 32 column tiles.
// A CHUNK is 32 consecutive pixels of one image; workgroup b of a chunk kernel takes chunk b % chunks of image
// b / chunks, chunks = ceil(P / 32): the pixel decomposition depends on P alone — one kernel selection for every N —
// so an image's rows do not depend on its batch mates.
//   forward   nvk_assign_kernel        the chunk's 32 x 512 values in LDS, |x_p| in fp32, logits x . w^T on the matrix
//                                      cores (every wave its 128 channels, one column tile after the other, the four
//                                      partial [32 x KP] tiles added through LDS), masked softmax   -> r[P], a[P][KP]
//             nvk_aggregate_kernel<0>  one workgroup per (image, 64 channels), 4 waves as 2 (column tiles kt, kt + 2)
//                                      x 2 (channels), all pixels in order; A = sum_p a in fp64     -> V[K][C], A[KP]
//             nvk_rowstats_kernel, nvk_apply_kernel   intra-normalisation and L2 over K C, one wave per row
//   backward  nvk_assign64_kernel<KT>  as the forward's, |x_p| and the logits in fp64 on the vector unit
//             nvk_aggregate_kernel<0>, nvk_rowstats64_kernel, nvk_dv_kernel (fp64: g, <Y, G>, dU, dV, <dV_k, c_k>, the
//             image's dC), nvk_contract_kernel (da on the matrix cores, ds), nvk_aggregate_kernel<1> (dW of the image),
//             nvk_dx_kernel (dxh = [a | ds] . [dV ; w], the projection), nvk_reduce_kernel (image order)
#include "vlad_backward_core.h"

namespace oibl {

constexpr int NVK_KMAX = 128;
constexpr int NVK_AP = 132;          // pitch of the aggregation's [32][KP] tile: 16-byte aligned rows

__host__ __device__ static inline int nvk_kp(int K) { return (K + 31) / 32 * 32; }

// dynamic LDS (bytes)
static inline int nvk_assign_lds(int K) { return (32 * VLAD_XP + 4 * 32 * (nvk_kp(K) + 1) + 32) * 4; }
static inline int nvk_assign64_lds(int K) { return (32 * VLAD_XP + nvk_kp(K) * VLB_WP) * 4; }
static inline int nvk_dx_lds(int K) { return (32 * VLAD_XP + 32 * (2 * nvk_kp(K) + 1) + 4 * 32 + 32 + 32) * 4; }

// the chunk [p0, p0 + 32) of one image -> x_s[32][VLAD_XP]; pixels beyond the image read as zeros
__device__ __forceinline__ void nvk_load_chunk(const float* __restrict__ fimg, int p0, int P, float* x_s) {
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int idx = (int)threadIdx.x + 256 * q;          // float4 index inside the chunk
    const int px = idx >> 7, c4 = (idx & 127) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p0 + px < P) v = *reinterpret_cast<const float4*>(fimg + (size_t)(p0 + px) * VLAD_C + c4);
    *reinterpret_cast<float4*>(x_s + px * VLAD_XP + c4) = v;
  }
}

// lp_s[wave][pixel][k] = sum over this wave's 128 channels of x_s[pixel][c] B[k][c] for k < KP; the rows K..KP-1 of
// B do not exist and count as zeros
__device__ __forceinline__ void nvk_chunk_times_rows(const float* x_s, const float* __restrict__ B, int K, int KT,
                                                     float* lp_s, int LP, int wave, int lane) {
  const int l31 = lane & 31, kh = lane >> 5;
  const float* xa = x_s + l31 * VLAD_XP + 128 * wave + 4 * kh;
  float* lw = lp_s + wave * 32 * LP;
#pragma unroll 1
  for (int kt = 0; kt < KT; ++kt) {
    const int row = 32 * kt + l31;
    const bool live = row < K;
    const float* wb = B + (size_t)(live ? row : 0) * VLAD_C + 128 * wave + 4 * kh;
    f32x16_t lg;
#pragma unroll
    for (int r = 0; r < 16; ++r) lg[r] = 0.f;
#pragma unroll 4
    for (int j = 0; j < 16; ++j) {
      const float4 av = *reinterpret_cast<const float4*>(xa + 8 * j);
      float4 bv = *reinterpret_cast<const float4*>(wb + 8 * j);
      if (!live) bv = make_float4(0.f, 0.f, 0.f, 0.f);
      lg = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, lg, 0, 0, 0);
      lg = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, lg, 0, 0, 0);
      lg = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, lg, 0, 0, 0);
      lg = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, lg, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) lw[acc_row(r, lane) * LP + 32 * kt + l31] = lg[r];
  }
}

// softmax over the K live clusters of a pixel held by its eight threads, thread `sub` the clusters sub + 8 j;
// dst = a + row * KP + sub: the live columns get the assignment, the columns K..KP-1 zeros
template <int NJ>
__device__ __forceinline__ void nvk_softmax_store(float (&l)[NJ], int K, int KP, bool live, float* dst) {
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (8 * j < K) mx = fmaxf(mx, l[j]);
  mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
  float ssum = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (8 * j < K) {
      l[j] = expf(l[j] - mx);
      ssum += l[j];
    }
  ssum += __shfl_xor(ssum, 1, 64);
  ssum += __shfl_xor(ssum, 2, 64);
  ssum += __shfl_xor(ssum, 4, 64);
  const float is = 1.0f / ssum;
  if (live) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (8 * j < KP) dst[8 * j] = 8 * j < K ? l[j] * is : 0.f;
  }
}

// forward: rn[row] = |x_p| (1 without normalize), a[row][k] = softmax_k(w_k . x_p / max(r_p, eps)), fp32 on the MFMA
__global__ __launch_bounds__(256) void nvk_assign_kernel(const float* __restrict__ feat, const float* __restrict__ w,
                                                         float* __restrict__ rn, float* __restrict__ a, int P, int K,
                                                         int chunks, int normalize) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int KP = nvk_kp(K), KT = KP / 32, LP = KP + 1;
  float* const x_s = reinterpret_cast<float*>(smem);             // [32][VLAD_XP]
  float* const lp_s = x_s + 32 * VLAD_XP;                          // [4 waves][32][LP]
  float* const r_s = lp_s + 4 * 32 * LP;                           // [32]
  const int n = (int)blockIdx.x / chunks, p0 = ((int)blockIdx.x - n * chunks) * 32;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int px = (int)threadIdx.x >> 3, sub = (int)threadIdx.x & 7;
  nvk_load_chunk(feat + (size_t)n * P * VLAD_C, p0, P, x_s);
  __syncthreads();
  {
    float ss = 0.f;
    if (normalize) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(x_s + px * VLAD_XP + 4 * (sub + 8 * j));
        ss = fmaf(v.x, v.x, ss);
        ss = fmaf(v.y, v.y, ss);
        ss = fmaf(v.z, v.z, ss);
        ss = fmaf(v.w, v.w, ss);
      }
      ss += __shfl_xor(ss, 1, 64);
      ss += __shfl_xor(ss, 2, 64);
      ss += __shfl_xor(ss, 4, 64);
    }
    if (sub == 0) r_s[px] = normalize ? sqrtf(ss) : 1.0f;
  }
  nvk_chunk_times_rows(x_s, w, K, KT, lp_s, LP, wave, lane);
  __syncthreads();
  const float r = r_s[px];
  const float iv = 1.0f / fmaxf(r, VLAD_EPS);
  float l[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    l[j] = 0.f;
    if (8 * j < K) {
      const int o = px * LP + sub + 8 * j;
      l[j] = (lp_s[o] + lp_s[32 * LP + o] + lp_s[2 * 32 * LP + o] + lp_s[3 * 32 * LP + o]) * iv;
    }
  }
  const bool live = p0 + px < P;
  const size_t row = (size_t)n * P + p0 + px;
  nvk_softmax_store<16>(l, K, KP, live, a + row * KP + sub);
  if (live && sub == 0) rn[row] = r;
}

// backward: the same function from |x_p| and logits accumulated in fp64 on the vector unit (vlad_assign's reasons);
// thread `sub` of a pixel the clusters sub + 8 j, j < 4 KT; the weights pass through LDS in four slices of 128
// channels, rows K..KP-1 of the slice are zeros
template <int KT>
__global__ __launch_bounds__(256) void nvk_assign64_kernel(const float* __restrict__ feat, const float* __restrict__ w,
                                                           float* __restrict__ rn, float* __restrict__ a, int P,
                                                           int K, int chunks, int normalize) {
  constexpr int C = VLAD_C, KP = 32 * KT, NJ = 4 * KT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const x_s = reinterpret_cast<float*>(smem);             // [32][VLAD_XP]
  float* const w_s = x_s + 32 * VLAD_XP;                           // [KP clusters][VLB_WP]
  const int n = (int)blockIdx.x / chunks, p0 = ((int)blockIdx.x - n * chunks) * 32;
  const int px = (int)threadIdx.x >> 3, sub = (int)threadIdx.x & 7;
  nvk_load_chunk(feat + (size_t)n * P * C, p0, P, x_s);
  double acc[NJ], ss = 0.0;
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = 0.0;
  for (int c0 = 0; c0 < C; c0 += 128) {
    __syncthreads();                                              // the chunk is in LDS / the last slice is consumed
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
      const int idx = (int)threadIdx.x + 256 * q;
      const int c4 = idx & 31, k = idx >> 5;                      // k < KP
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < K) v = *reinterpret_cast<const float4*>(w + (size_t)k * C + c0 + 4 * c4);
      *reinterpret_cast<float4*>(w_s + k * VLB_WP + 4 * c4) = v;
    }
    __syncthreads();
    const float* xr = x_s + px * VLAD_XP + c0;
    const float* wr = w_s + sub * VLB_WP;
#pragma unroll 2
    for (int c = 0; c < 128; c += 4) {
      const float4 xv = *reinterpret_cast<const float4*>(xr + c);
      const double x0 = (double)xv.x, x1 = (double)xv.y, x2 = (double)xv.z, x3 = (double)xv.w;
      ss = fma(x0, x0, ss);
      ss = fma(x1, x1, ss);
      ss = fma(x2, x2, ss);
      ss = fma(x3, x3, ss);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float4 wv = *reinterpret_cast<const float4*>(wr + 8 * j * VLB_WP + c);
        acc[j] = fma(x0, (double)wv.x, acc[j]);
        acc[j] = fma(x1, (double)wv.y, acc[j]);
        acc[j] = fma(x2, (double)wv.z, acc[j]);
        acc[j] = fma(x3, (double)wv.w, acc[j]);
      }
    }
  }
  const double rd = normalize ? sqrt(ss) : 1.0;
  const double invd = 1.0 / fmax(rd, (double)VLAD_EPS);
  float l[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) l[j] = (float)(acc[j] * invd);
  const bool live = p0 + px < P;
  const size_t row = (size_t)n * P + p0 + px;
  nvk_softmax_store<NJ>(l, K, KP, live, a + row * KP + sub);
  if (live && sub == 0) rn[row] = (float)rd;
}

// out[n][k][c0..c0+63] = sum_p a[p][k] xh[p][c] over the image's pixels in order, c0 = 64 blockIdx.y.  MODE 0: minus
// A_k centroids[k][c], A_k = sum_p a[p][k] in fp64 (every slice the same sums in the same order; slice 0 writes them
// to A[n][KP] where A is given).  MODE 1 (a = ds): the plain sum, the image's dW.
// 4 waves as 2 (column tiles kt = wk and wk + 2) x 2 (channel tiles).
template <int MODE>
__global__ __launch_bounds__(256) void nvk_aggregate_kernel(const float* __restrict__ feat,
                                                            const float* __restrict__ rn, const float* __restrict__ a,
                                                            const float* __restrict__ centroids,
                                                            float* __restrict__ out, double* __restrict__ A, int P,
                                                            int K) {
  constexpr int C = VLAD_C;
  __shared__ __attribute__((aligned(16))) float a_s[32][NVK_AP];
  __shared__ __attribute__((aligned(16))) float x_s[32][64];
  __shared__ float s_sum[NVK_KMAX];
  const int KP = nvk_kp(K), KT = KP / 32, KQ = KP / 4;          // KQ float4 per row of a
  const int n = blockIdx.x, c0 = blockIdx.y * 64;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wk = wave >> 1, wn = wave & 1;
  const float* fbase = feat + (size_t)n * P * C + c0;
  const float* abase = a + (size_t)n * P * KP;
  const float* rbase = rn + (size_t)n * P;

  f32x16_t acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  double colsum = 0.0;  // threads 0..KP-1: sum_p a[p][tid]

  // staging: a chunk = 32 x KP floats = 8 KP float4 (KT per thread); x chunk = 32 pixels x 64 channels (8 threads
  // per pixel, 8 channels each).  The next chunk's loads are issued before the current chunk's MFMAs.
  const int xp = threadIdx.x >> 3, xc = (threadIdx.x & 7) * 8;
  float4 pa[4], px0, px1;
  float psc;
  auto prefetch = [&](int p0) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      pa[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q < KT) {
        const int idx = threadIdx.x + q * 256;  // float4 index, < 8 KP
        const int pr = idx / KQ, cq = (idx - pr * KQ) * 4;
        if (p0 + pr < P) pa[q] = *reinterpret_cast<const float4*>(abase + (size_t)(p0 + pr) * KP + cq);
      }
    }
    px0 = make_float4(0.f, 0.f, 0.f, 0.f);
    px1 = px0;
    psc = 0.f;
    if (p0 + xp < P) {
      psc = 1.0f / fmaxf(rbase[p0 + xp], VLAD_EPS);
      const float* src = fbase + (size_t)(p0 + xp) * C + xc;
      px0 = *reinterpret_cast<const float4*>(src);
      px1 = *reinterpret_cast<const float4*>(src + 4);
    }
  };
  prefetch(0);
  for (int p0 = 0; p0 < P; p0 += 32) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < KT) {
        const int idx = threadIdx.x + q * 256;
        const int pr = idx / KQ, cq = (idx - pr * KQ) * 4;
        *reinterpret_cast<float4*>(&a_s[pr][cq]) = pa[q];
      }
    *reinterpret_cast<float4*>(&x_s[xp][xc]) = make_float4(px0.x * psc, px0.y * psc, px0.z * psc, px0.w * psc);
    *reinterpret_cast<float4*>(&x_s[xp][xc + 4]) = make_float4(px1.x * psc, px1.y * psc, px1.z * psc, px1.w * psc);
    __syncthreads();
    if (p0 + 32 < P) prefetch(p0 + 32);
    if (MODE == 0 && (int)threadIdx.x < KP) {
#pragma unroll
      for (int p = 0; p < 32; ++p) colsum += (double)a_s[p][threadIdx.x];
    }
#pragma unroll
    for (int st = 0; st < 16; ++st) {
      const int p = 2 * st + (lane >> 5);
      const float bv = x_s[p][wn * 32 + (lane & 31)];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (wk + 2 * i < KT)
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_s[p][(wk + 2 * i) * 32 + (lane & 31)], bv, acc[i], 0, 0, 0);
    }
    __syncthreads();
  }
  if (MODE == 0) {
    if ((int)threadIdx.x < KP) {
      s_sum[threadIdx.x] = (float)colsum;
      if (blockIdx.y == 0 && A != nullptr) A[(size_t)n * KP + threadIdx.x] = colsum;
    }
    __syncthreads();
  }
  const int ch = c0 + wn * 32 + (lane & 31);
#pragma unroll
  for (int i = 0; i < 2; ++i)
    if (wk + 2 * i < KT) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = (wk + 2 * i) * 32 + acc_row(r, lane);
        if (k < K) {
          float v = acc[i][r];
          if (MODE == 0) v -= s_sum[k] * centroids[(size_t)k * C + ch];
          out[((size_t)n * K + k) * C + ch] = v;
        }
      }
    }
}

// forward normalisation, one wave per (image, cluster) row: iv = 1 / max(|r|, eps) and s2 = |r iv|^2 ...
__global__ __launch_bounds__(256) void nvk_rowstats_kernel(const float* __restrict__ raw, float* __restrict__ stats,
                                                           long rows) {
  constexpr int C = VLAD_C;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* r = raw + row * C;
  float s = 0.f;
  for (int i = lane; i < C; i += 64) s = fmaf(r[i], r[i], s);
  s = wave_sum(s);
  const float iv = 1.0f / fmaxf(sqrtf(s), VLAD_EPS);
  float s2 = 0.f;
  for (int i = lane; i < C; i += 64) {
    const float v = r[i] * iv;
    s2 = fmaf(v, v, s2);
  }
  s2 = wave_sum(s2);
  if (lane == 0) {
    stats[2 * row] = iv;
    stats[2 * row + 1] = s2;
  }
}

// ... then ginv = 1 / max(sqrt(sum_k s2[n][k]), eps) (fixed-order sum), out = r iv ginv
__global__ __launch_bounds__(256) void nvk_apply_kernel(const float* __restrict__ raw, const float* __restrict__ stats,
                                                        float* __restrict__ out, long rows, int K) {
  constexpr int C = VLAD_C;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long n = row / K;
  float t = 0.f;
  for (int k = lane; k < K; k += 64) t += stats[2 * (n * K + k) + 1];
  t = wave_sum(t);
  const float iv = stats[2 * row];
  const float ginv = 1.0f / fmaxf(sqrtf(t), VLAD_EPS);
  const float* r = raw + row * C;
  float* o = out + row * C;
  for (int i = lane * 4; i < C; i += 256) {
    const float4 v = *reinterpret_cast<const float4*>(r + i);
    *reinterpret_cast<float4*>(o + i) =
        make_float4(v.x * iv * ginv, v.y * iv * ginv, v.z * iv * ginv, v.w * iv * ginv);
  }
}

// backward, one wave per (image, cluster) row of V, fp64: st[row] = { |V_k| , |U_k|^2 , <U_k, G_k> }
__global__ __launch_bounds__(256) void nvk_rowstats64_kernel(const float* __restrict__ V, const float* __restrict__ G,
                                                             double* __restrict__ st, long rows) {
  constexpr int C = VLAD_C;
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
  const double it = 1.0 / fmax(t, (double)VLAD_EPS);
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
__global__ __launch_bounds__(256) void nvk_dv_kernel(float* __restrict__ V, const float* __restrict__ G,
                                                     const double* __restrict__ st, const double* __restrict__ A,
                                                     const float* __restrict__ centroids, float* __restrict__ dvc,
                                                     double* __restrict__ dCp, long rows, int K) {
  constexpr int C = VLAD_C;
  const int KP = nvk_kp(K);
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long n = row / K;
  const int k = (int)(row - n * K);
  // |U|_F^2 and <U, G> of the image: lane j holds clusters j and j + 64, the same fixed-order sum in every wave
  double s2 = 0.0, ug = 0.0;
  for (int kk = lane; kk < K; kk += 64) {
    s2 += st[3 * (n * K + kk) + 1];
    ug += st[3 * (n * K + kk) + 2];
  }
  const double S2 = wave_sum_f64(s2);
  const double UG = wave_sum_f64(ug);
  const double gn = sqrt(S2);
  const bool g_clamped = gn < (double)VLAD_EPS;
  const double ig = 1.0 / fmax(gn, (double)VLAD_EPS);
  const double yg = g_clamped ? 0.0 : UG * ig;                      // <Y, G>; a clamped g is a constant
  const double t = st[3 * row];
  const bool t_clamped = t < (double)VLAD_EPS;
  const double it = 1.0 / fmax(t, (double)VLAD_EPS);
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
    const double na = -A[n * KP + k];
    double* o = dCp + row * C;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 4; ++i) o[256 * h + 4 * lane + i] = na * dv[4 * h + i];
  }
  if (lane == 0) dvc[row] = (float)dc;
}

// ds[row][k] = a_pk (da_pk - sum_j a_pj da_pj), da_pk = dV_k . x_p / r_p - dvc_k, for one chunk against its image's
// dV; the columns K..KP-1 of ds get zeros.  `out` may alias `a` (every element is read and written by the same thread).
__global__ __launch_bounds__(256) void nvk_contract_kernel(const float* __restrict__ feat, const float* __restrict__ dV,
                                                           const float* __restrict__ dvc, const float* __restrict__ rn,
                                                           const float* a, float* out, int P, int K, int chunks) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int KP = nvk_kp(K), KT = KP / 32, LP = KP + 1;
  float* const x_s = reinterpret_cast<float*>(smem);             // [32][VLAD_XP]
  float* const lp_s = x_s + 32 * VLAD_XP;                          // [4 waves][32][LP]
  float* const inv_s = lp_s + 4 * 32 * LP;                         // [32]
  const int n = (int)blockIdx.x / chunks, p0 = ((int)blockIdx.x - n * chunks) * 32;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  nvk_load_chunk(feat + (size_t)n * P * VLAD_C, p0, P, x_s);
  if (threadIdx.x < 32) {
    const int p = p0 + (int)threadIdx.x;
    inv_s[threadIdx.x] = p < P ? 1.0f / fmaxf(rn[(size_t)n * P + p], VLAD_EPS) : 0.f;
  }
  __syncthreads();
  nvk_chunk_times_rows(x_s, dV + (size_t)n * K * VLAD_C, K, KT, lp_s, LP, wave, lane);
  __syncthreads();
  const int px = (int)threadIdx.x >> 3, sub = (int)threadIdx.x & 7;
  const float iv = inv_s[px];
  const bool live = p0 + px < P;
  const size_t off = ((size_t)n * P + p0 + px) * KP + sub;
  float l[16], av[16];
  float dot = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    l[j] = 0.f;
    av[j] = 0.f;
    if (8 * j < K) {
      const int o = px * LP + sub + 8 * j;
      l[j] = (lp_s[o] + lp_s[32 * LP + o] + lp_s[2 * 32 * LP + o] + lp_s[3 * 32 * LP + o]) * iv -
             dvc[(size_t)n * K + sub + 8 * j];
      if (live) av[j] = a[off + 8 * j];
      dot = fmaf(av[j], l[j], dot);
    }
  }
  dot += __shfl_xor(dot, 1, 64);
  dot += __shfl_xor(dot, 2, 64);
  dot += __shfl_xor(dot, 4, 64);
  if (live) {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (8 * j < KP) out[off + 8 * j] = 8 * j < K ? av[j] * (l[j] - dot) : 0.f;
  }
}

// grad_feat of one chunk: dxh[p][c] = sum_k a[p][k] dV[k][c] + sum_k ds[p][k] w[k][c] with the image's dV, every wave
// its 128 channels (4 accumulator tiles of 32 pixels x 32 channels, 2 KP / 2 contraction steps; the rows K..KP-1 of
// dV and w count as zeros), then dx_p = (dxh_p - xh_p <xh_p, dxh_p>) / r_p
__global__ __launch_bounds__(256) void nvk_dx_kernel(const float* __restrict__ feat, const float* __restrict__ rn,
                                                     const float* __restrict__ a, const float* __restrict__ ds,
                                                     const float* __restrict__ dV, const float* __restrict__ w,
                                                     float* __restrict__ grad_feat, int P, int K, int chunks,
                                                     int normalize) {
  constexpr int C = VLAD_C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int KP = nvk_kp(K), AP = 2 * KP + 1, KH = KP / 2;       // KH float4 per row of [a | ds]
  float* const x_s = reinterpret_cast<float*>(smem);             // [32][VLAD_XP]
  float* const ad_s = x_s + 32 * VLAD_XP;                          // [32][AP]: a | ds
  float* const red_s = ad_s + 32 * AP;                            // [4 waves][32]
  float* const inv_s = red_s + 4 * 32;                            // [32]
  float* const dot_s = inv_s + 32;                                // [32]
  const int n = (int)blockIdx.x / chunks, p0 = ((int)blockIdx.x - n * chunks) * 32;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l31 = lane & 31, kh = lane >> 5;
  const size_t row0 = (size_t)n * P;                              // the image's first workspace row
  dV += (size_t)n * K * C;

  nvk_load_chunk(feat + row0 * C, p0, P, x_s);
  for (int idx = (int)threadIdx.x; idx < 32 * KH; idx += 256) {   // 32 x 2 KP floats
    const int px = idx / KH, k4 = (idx - px * KH) * 4;            // k4 < KP: a, else ds
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p0 + px < P) {
      const float* src = (k4 < KP ? a + (row0 + p0 + px) * KP + k4 : ds + (row0 + p0 + px) * KP + (k4 - KP));
      v = *reinterpret_cast<const float4*>(src);
    }
    float* d = ad_s + px * AP + k4;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  if (threadIdx.x < 32) {
    const int p = p0 + (int)threadIdx.x;
    inv_s[threadIdx.x] = p < P ? 1.0f / fmaxf(rn[row0 + p], VLAD_EPS) : 0.f;
    // the projection is dropped where the input is not normalised or its norm sits on the clamp
    dot_s[threadIdx.x] = 0.f;
  }
  __syncthreads();

  f32x16_t acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
  const float* arow = ad_s + l31 * AP + kh;
  const int cb = 128 * wave + l31;
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    const float* Bm = (half == 0 ? dV : w) + cb;
    const float* ar = arow + KP * half;
#pragma unroll 4
    for (int s = 0; s < KH; ++s) {
      const int k = 2 * s + kh;
      const bool lv = k < K;
      const float av = ar[2 * s];
      const float* br = Bm + (size_t)(lv ? k : 0) * C;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const float bv = lv ? br[32 * ct] : 0.f;
        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[ct], 0, 0, 0);
      }
    }
  }
  if (normalize) {
    // <x_p, dxh_p>: this wave's 128 channels, then the four waves in wave order
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int px = acc_row(r, lane);
      float v = 0.f;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) v = fmaf(acc[ct][r], x_s[px * VLAD_XP + cb + 32 * ct], v);
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
      const bool clamped = p < P ? rn[row0 + p] < VLAD_EPS : true;
      const float d = ((red_s[threadIdx.x] + red_s[32 + threadIdx.x]) + red_s[64 + threadIdx.x]) + red_s[96 + threadIdx.x];
      dot_s[threadIdx.x] = clamped ? 0.f : d * iv * iv;         // <xh_p, dxh_p> / r_p: it multiplies x_p below
    }
    __syncthreads();
  }
  float* gimg = grad_feat + row0 * C;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int px = acc_row(r, lane);
    if (p0 + px < P) {
      const float iv = inv_s[px], d = dot_s[px];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int ch = cb + 32 * ct;
        gimg[(size_t)(p0 + px) * C + ch] = (acc[ct][r] - x_s[px * VLAD_XP + ch] * d) * iv;
      }
    }
  }
}

// dW = sum_n dWp[n] (fp32), dC = sum_n dCp[n] (fp64, rounded once), both in image order; either output may be null
__global__ __launch_bounds__(256) void nvk_reduce_kernel(const float* __restrict__ dWp, const double* __restrict__ dCp,
                                                         float* __restrict__ dW, float* __restrict__ dC, int N,
                                                         int KC) {
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

// Workspaces, every block 256-byte aligned.
//   forward : r [N][P] | a [N][P][KP] | raw [N][K][C] | stats [N][K][2]
//   backward: r [N][P] | a [N][P][KP] | V -> dV [N][K][C] | stats [N][K][3] fp64 | A [N][KP] fp64 | dvc [N][K] |
//             dW of every image [N][K][C] | dC of every image [N][K][C] fp64 |
//             ds [N][P][KP] (only with grad_feat: without it ds overwrites a)
struct NvkLayout {
  size_t a, v, stats, A, dvc, dwp, dcp, ds, total;               // byte offsets; r is at 0
};
static inline NvkLayout nvk_forward_layout(size_t N, size_t P, size_t K) {
  const size_t KP = nvk_kp((int)K), C = VLAD_C;
  NvkLayout o{};
  o.a = align_up(N * P * sizeof(float), 256);
  o.v = o.a + align_up(N * P * KP * sizeof(float), 256);
  o.stats = o.v + align_up(N * K * C * sizeof(float), 256);
  o.total = o.stats + align_up(N * K * 2 * sizeof(float), 256);
  return o;
}
static inline NvkLayout nvk_backward_layout(size_t N, size_t P, size_t K, int want_grad_feat) {
  const size_t KP = nvk_kp((int)K), C = VLAD_C;
  NvkLayout o{};
  o.a = align_up(N * P * sizeof(float), 256);
  o.v = o.a + align_up(N * P * KP * sizeof(float), 256);
  o.stats = o.v + align_up(N * K * C * sizeof(float), 256);
  o.A = o.stats + align_up(N * K * 3 * sizeof(double), 256);
  o.dvc = o.A + align_up(N * KP * sizeof(double), 256);
  o.dwp = o.dvc + align_up(N * K * sizeof(float), 256);
  o.dcp = o.dwp + align_up(N * K * C * sizeof(float), 256);
  o.ds = o.dcp + align_up(N * K * C * sizeof(double), 256);
  o.total = o.ds + (want_grad_feat ? align_up(N * P * KP * sizeof(float), 256) : 0);
  return o;
}

static inline bool nvk_k_ok(int K) { return K >= 16 && K <= NVK_KMAX && K % 16 == 0; }
static inline bool nvk_grid_ok(int N, int P) { return (long long)N * ((P + 31) / 32) <= 0x7fffffffLL; }

}  // namespace oibl

using namespace oibl;

// what the two entry points check in the same words
#define NVK_REQUIRE_SHAPE(what)                                                                                      \
  OIBL_REQUIRE(nvk_k_ok(K), what ": num_clusters must be a multiple of 16 in [16, 128] (got %d)", K);                \
  OIBL_REQUIRE(C == VLAD_C, what ": kernels are built for dim = 512 (got %d)", C);                                   \
  OIBL_REQUIRE(N > 0 && P > 0, what ": bad shape N=%d P=%d", N, P);                                                  \
  OIBL_REQUIRE(nvk_grid_ok(N, P), what ": N x ceil(P / 32) must fit a grid dimension (got N=%d P=%d)", N, P)

static int nvk_launch_assign64(int KT, dim3 grid, int lds, hipStream_t st, const float* x, const float* w, float* rn,
                               float* a, int P, int K, int chunks, int normalize) {
#define NVK_ASSIGN64_CASE(T)                                                                                         \
  case T:                                                                                                            \
    OIBL_SET_MAX_LDS(nvk_assign64_kernel<T>, (32 * VLAD_XP + 32 * T * VLB_WP) * 4);                                  \
    hipLaunchKernelGGL(nvk_assign64_kernel<T>, grid, dim3(256), lds, st, x, w, rn, a, P, K, chunks, normalize);     \
    break
  switch (KT) {
    NVK_ASSIGN64_CASE(1);
    NVK_ASSIGN64_CASE(2);
    NVK_ASSIGN64_CASE(3);
    NVK_ASSIGN64_CASE(4);
  }
#undef NVK_ASSIGN64_CASE
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

extern "C" {

size_t oibl_netvlad_k_workspace_bytes(int N, int P, int K, int C) {
  if (N <= 0 || P <= 0 || !nvk_k_ok(K) || C != VLAD_C) return 0;
  return nvk_forward_layout(N, P, K).total;
}

int oibl_netvlad_forward_k(const void* feat, int N, int P, int K, int C, const float* assign_w, const float* centroids,
                           int normalize_input, float* vlad_raw, float* vlad_norm, void* ws, size_t ws_bytes,
                           void* stream) {
  OIBL_REQUIRE(feat && assign_w && centroids && ws, "netvlad_k: null pointer");
  OIBL_REQUIRE(vlad_raw || vlad_norm, "netvlad_k: no output requested");
  NVK_REQUIRE_SHAPE("netvlad_k");
  OIBL_REQUIRE((uintptr_t)feat % 16 == 0 && (uintptr_t)assign_w % 16 == 0 && (uintptr_t)centroids % 16 == 0 &&
                   (uintptr_t)vlad_raw % 16 == 0 && (uintptr_t)vlad_norm % 16 == 0,
               "netvlad_k: feat, assign_w, centroids, vlad_raw and vlad_norm must be 16-byte aligned");
  const size_t need = oibl_netvlad_k_workspace_bytes(N, P, K, C);
  if ((uintptr_t)ws % 256 != 0) {
    set_error("netvlad_k: workspace must be 256-byte aligned");
    return OIBL_E_WORKSPACE;
  }
  if (ws_bytes < need) {
    set_error("netvlad_k: workspace %zu < required %zu bytes", ws_bytes, need);
    return OIBL_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* wsb = (char*)ws;
  const float* x = (const float*)feat;
  const NvkLayout lay = nvk_forward_layout(N, P, K);
  float* rn = (float*)wsb;
  float* a = (float*)(wsb + lay.a);
  float* raw = vlad_raw ? vlad_raw : (float*)(wsb + lay.v);
  float* stats = (float*)(wsb + lay.stats);
  const int chunks = (P + 31) / 32;
  const dim3 pgrid((unsigned)(N * chunks));

  OIBL_SET_MAX_LDS(nvk_assign_kernel, nvk_assign_lds(NVK_KMAX));
  hipLaunchKernelGGL(nvk_assign_kernel, pgrid, dim3(256), nvk_assign_lds(K), st, x, assign_w, rn, a, P, K, chunks,
                     normalize_input);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(nvk_aggregate_kernel<0>, dim3((unsigned)N, VLAD_C / 64), dim3(256), 0, st, x, (const float*)rn,
                     (const float*)a, centroids, raw, (double*)nullptr, P, K);
  OIBL_LAUNCH_CHECK();
  if (vlad_norm) {
    const long vrows = (long)N * K;
    const unsigned fgrid = (unsigned)((vrows + 3) / 4);
    hipLaunchKernelGGL(nvk_rowstats_kernel, dim3(fgrid), dim3(256), 0, st, (const float*)raw, stats, vrows);
    OIBL_LAUNCH_CHECK();
    hipLaunchKernelGGL(nvk_apply_kernel, dim3(fgrid), dim3(256), 0, st, (const float*)raw, (const float*)stats,
                       vlad_norm, vrows, K);
    OIBL_LAUNCH_CHECK();
  }
  return OIBL_OK;
}

size_t oibl_netvlad_k_backward_workspace_bytes(int N, int P, int K, int C, int want_grad_feat) {
  if (N <= 0 || P <= 0 || !nvk_k_ok(K) || C != VLAD_C) return 0;
  return nvk_backward_layout(N, P, K, want_grad_feat).total;
}

int oibl_netvlad_backward_k(const void* feat, int N, int P, int K, int C, const float* assign_w,
                            const float* centroids, int normalize_input, const float* grad_vlad_norm,
                            float* grad_assign_w, float* grad_centroids, float* grad_feat, void* ws, size_t ws_bytes,
                            void* stream) {
  OIBL_REQUIRE(feat && assign_w && centroids && grad_vlad_norm && ws, "netvlad_backward_k: null pointer");
  OIBL_REQUIRE(grad_assign_w || grad_centroids || grad_feat, "netvlad_backward_k: no output requested");
  NVK_REQUIRE_SHAPE("netvlad_backward_k");
  OIBL_REQUIRE((uintptr_t)feat % 16 == 0 && (uintptr_t)assign_w % 16 == 0 && (uintptr_t)centroids % 16 == 0 &&
                   (uintptr_t)grad_vlad_norm % 16 == 0 && (uintptr_t)grad_feat % 16 == 0,
               "netvlad_backward_k: feat, assign_w, centroids, grad_vlad_norm and grad_feat must be 16-byte aligned");
  const size_t need = oibl_netvlad_k_backward_workspace_bytes(N, P, K, C, grad_feat != nullptr);
  if ((uintptr_t)ws % 256 != 0) {
    set_error("netvlad_backward_k: workspace must be 256-byte aligned");
    return OIBL_E_WORKSPACE;
  }
  if (ws_bytes < need) {
    set_error("netvlad_backward_k: workspace %zu < required %zu bytes", ws_bytes, need);
    return OIBL_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  char* wsb = (char*)ws;
  const float* x = (const float*)feat;
  const NvkLayout lay = nvk_backward_layout(N, P, K, grad_feat != nullptr);
  float* rn = (float*)wsb;
  float* a = (float*)(wsb + lay.a);
  float* V = (float*)(wsb + lay.v);
  double* stats = (double*)(wsb + lay.stats);
  double* A = (double*)(wsb + lay.A);
  float* dvc = (float*)(wsb + lay.dvc);
  float* dWp = (float*)(wsb + lay.dwp);
  double* dCp = grad_centroids ? (double*)(wsb + lay.dcp) : nullptr;
  float* ds = grad_feat ? (float*)(wsb + lay.ds) : a;
  const int chunks = (P + 31) / 32;
  const dim3 pgrid((unsigned)(N * chunks));
  const long vrows = (long)N * K;
  const unsigned rgrid = (unsigned)((vrows + 3) / 4);

  if (int rc = nvk_launch_assign64(nvk_kp(K) / 32, pgrid, nvk_assign64_lds(K), st, x, assign_w, rn, a, P, K, chunks,
                                   normalize_input))
    return rc;
  hipLaunchKernelGGL(nvk_aggregate_kernel<0>, dim3((unsigned)N, VLAD_C / 64), dim3(256), 0, st, x, (const float*)rn,
                     (const float*)a, centroids, V, A, P, K);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(nvk_rowstats64_kernel, dim3(rgrid), dim3(256), 0, st, (const float*)V, grad_vlad_norm, stats,
                     vrows);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(nvk_dv_kernel, dim3(rgrid), dim3(256), 0, st, V, grad_vlad_norm, (const double*)stats,
                     (const double*)A, centroids, dvc, dCp, vrows, K);
  OIBL_LAUNCH_CHECK();
  if (grad_assign_w || grad_feat) {
    OIBL_SET_MAX_LDS(nvk_contract_kernel, nvk_assign_lds(NVK_KMAX));
    hipLaunchKernelGGL(nvk_contract_kernel, pgrid, dim3(256), nvk_assign_lds(K), st, x, (const float*)V,
                       (const float*)dvc, (const float*)rn, (const float*)a, ds, P, K, chunks);
    OIBL_LAUNCH_CHECK();
  }
  if (grad_assign_w) {
    hipLaunchKernelGGL(nvk_aggregate_kernel<1>, dim3((unsigned)N, VLAD_C / 64), dim3(256), 0, st, x, (const float*)rn,
                       (const float*)ds, centroids, dWp, (double*)nullptr, P, K);
    OIBL_LAUNCH_CHECK();
  }
  if (grad_feat) {
    OIBL_SET_MAX_LDS(nvk_dx_kernel, nvk_dx_lds(NVK_KMAX));
    hipLaunchKernelGGL(nvk_dx_kernel, pgrid, dim3(256), nvk_dx_lds(K), st, x, (const float*)rn, (const float*)a,
                       (const float*)ds, (const float*)V, assign_w, grad_feat, P, K, chunks, normalize_input);
    OIBL_LAUNCH_CHECK();
  }
  if (grad_assign_w || grad_centroids) {
    hipLaunchKernelGGL(nvk_reduce_kernel, dim3((unsigned)(K * VLAD_C / 256)), dim3(256), 0, st, (const float*)dWp,
                       (const double*)dCp, grad_assign_w, grad_centroids, N, K * VLAD_C);
    OIBL_LAUNCH_CHECK();
  }
  return OIBL_OK;
}

}  // extern "C"
