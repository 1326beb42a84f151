// What netvlad_backward.hip and region_backward.hip share: the chunk kernels of a NetVLAD head's backward (assign,
// contract, aggregate, dx), the reduction over the images, the chunk loader, the fp64 wave sum, the LDS pitches and
// the workspace layout.  Each exists once, here; the two units keep one-line __global__ wrappers with their own
// names and what is particular to them (their rowstats / dv pairs, the scores' backward, the entry points).
//
// The formulas are in netvlad_backward.hip's header.  A UNIT is what a chunk belongs to and what owns one dV: an
// image of the plain head, a quarter of an image of the region head.  A CHUNK is 32 consecutive pixels of one unit.
// The workspace rows r, a and ds are unit-major: row m Pu + i for pixel i of unit m, Pu the pixels of a unit.  The
// two heads differ in three things, and a pixel-map policy, passed by value, answers all three:
//   which grid axis carries the unit and which the chunk            unit(), chunk()
//   which map pixel (row of the image's NHWC map) pixel i of unit m is  prepare(), pixel(), image_pixel()
//   which image a unit belongs to, and how many pixels each has     image_row(), pixels(), image_pixels()
// A chunk pixel beyond the unit's end is not LIVE.  Where a body needs a pixel's place in the map it asks live() and,
// for a live t only, pixel() — two answers, because one answer with a sentinel costs the plain head 16 selects in its
// loader, and a table entry that was tested >= 0 needs no sign extension.  Workspace rows are tested p0 + t < pixels().
//   PlainMap{P}        grid (chunks, N); pixel p0 + t; no table in LDS, prepare() is empty and holds NO barrier
//   QuarterMap{hq, wq} grid (4 N, chunks) — 4 N quarters do not fit a grid's y; unit m is quarter m & 3 of image
//                      m >> 2; a 32-entry table of the chunk's map pixels in LDS behind the kernel's own arrays
//                      (TABLE_BYTES), filled by threads 0..31 in prepare(), which ends in a barrier
//   vlad_assign        one workgroup per chunk: the chunk's 32 x 512 values in LDS, |x_p| and the logits in fp64 on
//                      the vector unit, softmax                                                  -> r, a[.][64]
//   vlad_aggregate<0>  netvlad_aggregate_kernel's scheme on v_mfma_f32_32x32x2_f32, one workgroup per (segment, 64
//                      channels), the segment's pixels in order; A in fp64                       -> V[K][C], A[K]
//   vlad_contract      the chunk against its unit's dV on the matrix cores (every wave contracts its 128 channels, the
//                      four partial [32 x 64] tiles are added through LDS): da, ds              -> ds[.][64]
//   vlad_aggregate<1>  the aggregation over a whole image with ds in the place of a              -> dW of the image
//   vlad_dx            dxh = [a | ds] . [dV ; w] per chunk (32 x 512 over 128) on the same instruction, the
//                      projection, the division                                                  -> grad_feat
//   vlad_reduce        dW = sum_n dW_n (fp32), dC = sum_n dC_n (fp64, rounded once), both in image order
#pragma once

#include "vlad_common.h"

namespace oibl {

constexpr int VLB_AP = 129;         // pitch of the [32][128] operand tile [a | ds]
constexpr int VLB_WP = 132;          // floats per LDS row of the weight slice: 16-byte aligned, +4 banks per cluster
// dynamic LDS of the three chunk kernels without the map's table: a launch asks for these + Map::TABLE_BYTES
constexpr int VLB_ASSIGN_LDS = (32 * VLAD_XP + VLAD_K * VLB_WP) * 4;
constexpr int VLB_CONTRACT_LDS = (32 * VLAD_XP + 4 * 32 * VLAD_LP + 32) * 4;
constexpr int VLB_DX_LDS = (32 * VLAD_XP + 32 * VLB_AP + 4 * 32 + 32 + 32) * 4;

__device__ static inline double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// a unit is an image, a chunk's pixels are consecutive rows of its map
struct PlainMap {
  int P;
  static constexpr int TABLE_BYTES = 0;
  __device__ static int chunk() { return blockIdx.x; }
  __device__ static int unit() { return blockIdx.y; }
  __device__ int pixels() const { return P; }                           // of a unit
  __device__ int image_pixels() const { return P; }
  __device__ size_t image_row(int m) const { return (size_t)m * P; }    // first row of unit m's image in the map
  __device__ void prepare(int, int, int*) const {}
  __device__ bool live(int p0, int t, const int*) const { return p0 + t < P; }
  __device__ int pixel(int p0, int t, const int*) const { return p0 + t; }
  __device__ int image_pixel(int j) const { return j; }                 // of workspace row j of an image
};

// a unit is a quarter of an image of 2 hq x 2 wq pixels, row-major inside the quarter
struct QuarterMap {
  int hq, wq;
  static constexpr int TABLE_BYTES = 32 * 4;
  __device__ static int chunk() { return blockIdx.y; }
  __device__ static int unit() { return blockIdx.x; }
  __device__ int pixels() const { return hq * wq; }
  __device__ int image_pixels() const { return 4 * hq * wq; }
  __device__ size_t image_row(int m) const { return (size_t)(m >> 2) * 4 * (hq * wq); }
  __device__ int map_pixel(int q, int i) const { return quarter_map_pixel(q, i, hq, wq); }
  // tab[t] = map pixel of pixel p0 + t of unit m, -1 beyond the unit (threads 0..31), then the barrier that
  // publishes it
  __device__ void prepare(int m, int p0, int* tab) const {
    if (threadIdx.x < 32) {
      const int i = p0 + (int)threadIdx.x;
      tab[threadIdx.x] = i < hq * wq ? map_pixel(m & 3, i) : -1;
    }
    __syncthreads();
  }
  __device__ bool live(int, int t, const int* tab) const { return tab[t] >= 0; }
  __device__ int pixel(int, int t, const int* tab) const { return tab[t]; }
  __device__ int image_pixel(int j) const {
    const int q = j / (hq * wq);
    return map_pixel(q, j - q * (hq * wq));
  }
};

// the chunk [p0, p0 + 32) of one unit -> x_s[32][VLAD_XP]; pixels beyond the unit read as zeros
template <class Map>
__device__ __forceinline__ void vlad_load_chunk(const Map map, const float* __restrict__ fimg, int p0, const int* tab,
                                                float* x_s) {
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int idx = (int)threadIdx.x + 256 * q;          // float4 index inside the chunk
    const int px = idx >> 7, c4 = (idx & 127) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (map.live(p0, px, tab))
      v = *reinterpret_cast<const float4*>(fimg + (size_t)map.pixel(p0, px, tab) * VLAD_C + c4);
    *reinterpret_cast<float4*>(x_s + px * VLAD_XP + c4) = v;
  }
}

// rn[row] = |x_p| (1 without normalize) and a[row][k] = softmax_k(w_k . x_p / r_p) for one 32-pixel chunk of one unit.
// The logits and the norm are accumulated in fp64 on the vector unit, not on the fp32 matrix cores: a tuple loss makes
// the images' contributions to dC cancel (60-fold on near-identical maps), and the rounding of fp32 logits alone —
// 512-term sums whose terms are far larger than the sum — then costs 8e-7 to 3e-6 of dC.  This `a` is therefore NOT
// the forward kernels' `a` bit for bit (netvlad.hip forms its logits on the fp32 matrix cores): the backward
// differentiates the same function from a more accurate evaluation of it.  Eight threads per pixel, thread `sub`
// the clusters sub, sub + 8, ..., sub + 56; the weights pass through LDS in four slices of 128 channels, [cluster]
// [channel] as in memory (coalesced 512-byte row pieces in, the eight rows of a wave's reads on distinct banks).
template <class Map>
__device__ __forceinline__ void vlad_assign(const Map map, const float* __restrict__ feat, const float* __restrict__ w,
                                            float* __restrict__ rn, float* __restrict__ a, int normalize) {
  constexpr int C = VLAD_C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const x_s = reinterpret_cast<float*>(smem);             // [32][VLAD_XP]
  float* const w_s = x_s + 32 * VLAD_XP;                           // [64 clusters][VLB_WP]: 128 channels of a slice
  int* const tab = reinterpret_cast<int*>(smem + VLB_ASSIGN_LDS);  // the map's table
  const int Pu = map.pixels();
  const int m = map.unit(), p0 = map.chunk() * 32;
  const int px = (int)threadIdx.x >> 3, sub = (int)threadIdx.x & 7;
  map.prepare(m, p0, tab);
  vlad_load_chunk(map, feat + map.image_row(m) * C, p0, tab, x_s);
  double acc[8], ss = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.0;
  for (int c0 = 0; c0 < C; c0 += 128) {
    __syncthreads();                                              // the chunk is in LDS / the last slice is consumed
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = (int)threadIdx.x + 256 * q;
      const int c4 = idx & 31, k = idx >> 5;                      // k < 64; 32 lanes walk one row's 512 bytes
      *reinterpret_cast<float4*>(w_s + k * VLB_WP + 4 * c4) =
          *reinterpret_cast<const float4*>(w + (size_t)k * C + c0 + 4 * c4);
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
      for (int j = 0; j < 8; ++j) {
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
  if (p0 + px < Pu) {
    const size_t row = (size_t)m * Pu + p0 + px;
    float* dst = a + row * VLAD_K + sub;
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[8 * j] = l[j] * is;         // the eight threads of a pixel: 32 bytes per j
    if (sub == 0) rn[row] = (float)rd;
  }
}

// ds[row][k] = a_pk (da_pk - sum_j a_pj da_pj), da_pk = dV_k . x_p / r_p - dvc_k, for one 32-pixel chunk of one unit
// against that unit's dV (B[m]) and dvc: the chunk in LDS, every wave contracts its 128 channels on
// v_mfma_f32_32x32x2_f32, the four partial [32 x 64] tiles are added through LDS.  `out` may alias `a` (every element
// is read and written by the same thread).
template <class Map>
__device__ __forceinline__ void vlad_contract(const Map map, const float* __restrict__ feat,
                                              const float* __restrict__ B, const float* __restrict__ dvc,
                                              const float* __restrict__ rn, const float* a, float* out) {
  constexpr int C = VLAD_C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const x_s = reinterpret_cast<float*>(smem);             // [32][VLAD_XP]
  float* const lp_s = x_s + 32 * VLAD_XP;                          // [4 waves][32][VLAD_LP]
  float* const inv_s = lp_s + 4 * 32 * VLAD_LP;                    // [32]
  int* const tab = reinterpret_cast<int*>(smem + VLB_CONTRACT_LDS);  // the map's table
  const int Pu = map.pixels();
  const int m = map.unit(), p0 = map.chunk() * 32;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l31 = lane & 31, kh = lane >> 5;
  B += (size_t)m * VLAD_K * C;

  map.prepare(m, p0, tab);
  vlad_load_chunk(map, feat + map.image_row(m) * C, p0, tab, x_s);
  if (threadIdx.x < 32) {
    const int p = p0 + (int)threadIdx.x;
    inv_s[threadIdx.x] = p < Pu ? 1.0f / fmaxf(rn[(size_t)m * Pu + p], VLAD_EPS) : 0.f;
  }
  __syncthreads();
  {  // partial contraction over this wave's 128 channels: [32 pixels] x [64 rows of B]
    f32x16_t lg[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) lg[ct][r] = 0.f;
    const float* xa = x_s + l31 * VLAD_XP + 128 * wave + 4 * kh;
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
    float* lw = lp_s + wave * 32 * VLAD_LP;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) lw[acc_row(r, lane) * VLAD_LP + 32 * ct + l31] = lg[ct][r];
  }
  __syncthreads();
  {  // eight threads per pixel, eight clusters each
    const int px = (int)threadIdx.x >> 3, sub = (int)threadIdx.x & 7;
    const float iv = inv_s[px];
    const bool live = p0 + px < Pu;
    float l[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int o = px * VLAD_LP + sub * 8 + k;
      l[k] = (lp_s[o] + lp_s[32 * VLAD_LP + o] + lp_s[2 * 32 * VLAD_LP + o] + lp_s[3 * 32 * VLAD_LP + o]) * iv;
    }
    const size_t off = ((size_t)m * Pu + p0 + px) * VLAD_K + sub * 8;
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
      l[k] -= dvc[m * VLAD_K + sub * 8 + k];
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

// out[s][k][c0..c0+63] = sum_p a[p][k] xh[p][c] over segment s (blockIdx.x) of `seg_px` consecutive workspace rows, in
// order; `segs` segments per image, c0 = 64 blockIdx.y.  MODE 0 (a segment is a unit): minus A_k centroids[k][c], and
// A[s][k] = sum_p a[p][k] in fp64 (every slice computes the same sums in the same order; slice 0 writes them).
// MODE 1 (segs 1, the whole image; a = ds): the plain sum, the image's dW.
// 4 waves as 2 (clusters) x 2 (channels), one 32x32 fp32 accumulator tile each.
template <int MODE, class Map>
__device__ __forceinline__ void vlad_aggregate(const Map map, const float* __restrict__ feat,
                                               const float* __restrict__ rn, const float* __restrict__ a,
                                               const float* __restrict__ centroids, float* __restrict__ out,
                                               double* __restrict__ A, int segs, int seg_px) {
  constexpr int C = VLAD_C;
  __shared__ __attribute__((aligned(16))) float a_s[32][64];
  __shared__ __attribute__((aligned(16))) float x_s[32][64];
  __shared__ float s_sum[64];
  const int Pi = map.image_pixels();
  const int s = blockIdx.x, c0 = blockIdx.y * 64;
  const int n = s / segs, j0 = (s - n * segs) * seg_px;         // first workspace row of the segment in its image
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const float* fbase = feat + (size_t)n * Pi * C + c0;
  const float* abase = a + ((size_t)n * Pi + j0) * 64;
  const float* rbase = rn + (size_t)n * Pi + j0;

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
      if (p0 + pr < seg_px) pa[q] = *reinterpret_cast<const float4*>(abase + (size_t)(p0 + pr) * 64 + cq);
    }
    px0 = make_float4(0.f, 0.f, 0.f, 0.f);
    px1 = px0;
    psc = 0.f;
    if (p0 + xp < seg_px) {
      psc = 1.0f / fmaxf(rbase[p0 + xp], VLAD_EPS);
      const float* src = fbase + (size_t)map.image_pixel(j0 + p0 + xp) * C + xc;
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
      if (blockIdx.y == 0) A[s * 64 + threadIdx.x] = colsum;
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

// grad_feat of one 32-pixel chunk of one unit: dxh[p][c] = sum_k a[p][k] dV[k][c] + sum_k ds[p][k] w[k][c] with the
// unit's dV, every wave its 128 channels (4 accumulator tiles of 32 pixels x 32 channels, 128 contraction steps), then
// dx_p = (dxh_p - xh_p <xh_p, dxh_p>) / r_p, written to the pixel's place in the map.
template <class Map>
__device__ __forceinline__ void vlad_dx(const Map map, const float* __restrict__ feat, const float* __restrict__ rn,
                                        const float* __restrict__ a, const float* __restrict__ ds,
                                        const float* __restrict__ dV, const float* __restrict__ w,
                                        float* __restrict__ grad_feat, int normalize) {
  constexpr int C = VLAD_C;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const x_s = reinterpret_cast<float*>(smem);             // [32][VLAD_XP]
  float* const ad_s = x_s + 32 * VLAD_XP;                          // [32][VLB_AP]: a | ds
  float* const red_s = ad_s + 32 * VLB_AP;                        // [4 waves][32]
  float* const inv_s = red_s + 4 * 32;                            // [32]
  float* const dot_s = inv_s + 32;                                // [32]
  int* const tab = reinterpret_cast<int*>(smem + VLB_DX_LDS);    // the map's table
  const int Pu = map.pixels();
  const int m = map.unit(), p0 = map.chunk() * 32;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l31 = lane & 31, kh = lane >> 5;
  const size_t row0 = (size_t)m * Pu;                             // the unit's first workspace row
  dV += (size_t)m * VLAD_K * C;

  map.prepare(m, p0, tab);
  vlad_load_chunk(map, feat + map.image_row(m) * C, p0, tab, x_s);
#pragma unroll
  for (int q = 0; q < 4; ++q) {                                   // 32 x 128 floats = 1024 float4
    const int idx = (int)threadIdx.x + 256 * q;
    const int px = idx >> 5, k4 = (idx & 31) * 4;                 // k4 < 64: a, else ds
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p0 + px < Pu) {
      const float* src = (k4 < 64 ? a : ds) + (row0 + p0 + px) * VLAD_K + (k4 & 63);
      v = *reinterpret_cast<const float4*>(src);
    }
    float* d = ad_s + px * VLB_AP + k4;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  if (threadIdx.x < 32) {
    const int p = p0 + (int)threadIdx.x;
    inv_s[threadIdx.x] = p < Pu ? 1.0f / fmaxf(rn[row0 + p], VLAD_EPS) : 0.f;
    // the projection is dropped where the input is not normalised or its norm sits on the clamp
    dot_s[threadIdx.x] = 0.f;
  }
  __syncthreads();

  f32x16_t acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[ct][r] = 0.f;
  const float* arow = ad_s + l31 * VLB_AP + kh;
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
      const bool clamped = p < Pu ? rn[row0 + p] < VLAD_EPS : true;
      const float d = ((red_s[threadIdx.x] + red_s[32 + threadIdx.x]) + red_s[64 + threadIdx.x]) + red_s[96 + threadIdx.x];
      dot_s[threadIdx.x] = clamped ? 0.f : d * iv * iv;         // <xh_p, dxh_p> / r_p: it multiplies x_p below
    }
    __syncthreads();
  }
  float* gimg = grad_feat + map.image_row(m) * C;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int px = acc_row(r, lane);
    if (map.live(p0, px, tab)) {
      const float iv = inv_s[px], d = dot_s[px];
      const size_t mp = (size_t)map.pixel(p0, px, tab);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int ch = cb + 32 * ct;
        gimg[mp * C + ch] = (acc[ct][r] - x_s[px * VLAD_XP + ch] * d) * iv;
      }
    }
  }
}

// dW = sum_n dWp[n] (fp32), dC = sum_n dCp[n] (fp64, rounded once), both in image order; either output may be null
__device__ __forceinline__ void vlad_reduce(const float* __restrict__ dWp, const double* __restrict__ dCp,
                                            float* __restrict__ dW, float* __restrict__ dC, int N) {
  constexpr int KC = VLAD_K * VLAD_C;
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

// The workspace of a backward call over N images of P pixels, `units` units and `stat_rows` normalised vectors per
// image (1 and 1 for the plain head, 4 quarters and 9 regions for the region head); every block 256-byte aligned:
//   r [N][P] | a [N][P][64] | V -> dV [N units][K][C] | stats [N stat_rows][K][3] fp64 | A [N units][K] fp64 |
//   dvc [N units][K] | dW of every image [N][K][C] | dC of every image [N][K][C] fp64 |
//   ds [N][P][64] (only with grad_feat: without it ds overwrites a)
struct VladBackwardLayout {
  size_t a, v, stats, A, dvc, dwp, dcp, ds, total;               // byte offsets; r is at 0
};
static inline VladBackwardLayout vlad_backward_layout(size_t N, size_t P, size_t units, size_t stat_rows,
                                                      int want_grad_feat) {
  constexpr size_t K = VLAD_K, C = VLAD_C;
  VladBackwardLayout o;
  o.a = align_up(N * P * sizeof(float), 256);
  o.v = o.a + align_up(N * P * 64 * sizeof(float), 256);
  o.stats = o.v + align_up(N * units * K * C * sizeof(float), 256);
  o.A = o.stats + align_up(N * stat_rows * K * 3 * sizeof(double), 256);
  o.dvc = o.A + align_up(N * units * K * sizeof(double), 256);
  o.dwp = o.dvc + align_up(N * units * K * sizeof(float), 256);
  o.dcp = o.dwp + align_up(N * K * C * sizeof(float), 256);
  o.ds = o.dcp + align_up(N * K * C * sizeof(double), 256);
  o.total = o.ds + (want_grad_feat ? align_up(N * P * 64 * sizeof(float), 256) : 0);
  return o;
}

}  // namespace oibl
