// What netvlad.hip and region.hip share: the fused slab kernel of a NetVLAD head's forward, the counterpart of
// vlad_backward_core.h.  The body exists once, here; the two units keep one-line __global__ wrappers with their own
// names (netvlad_fused_kernel, region_aggregate_kernel).
//
// A UNIT is an image of the plain head, a quarter of an image of the region head; one workgroup takes one SLAB of a
// unit's pixels in CHUNKS of 32.  Per chunk: its 32 x 512 values go to LDS with coalesced 16-byte loads (64.5 KB, rows
// 4 floats apart in the banks); 1 / |x_p| from LDS; logits = x . w^T on v_mfma_f32_32x32x2_f32 — every wave contracts
// its 128 channels, the four partial [32 x 64] tiles are added through LDS — scaled by 1 / |x_p|; softmax over the 64
// clusters; aggregation sum_p a[p][k] / |x_p| * x[p][c] on the same instruction from the same LDS chunk, 64 clusters x
// 128 channels of accumulators per wave (128 VGPRs) kept across the slab; at the end acc - (sum_p a[p][k])
// centroids[k][c] goes to the slab's partial.  Exact fp32 throughout.
//
// The heads differ in how pixel i of the unit becomes an address (unit_base(), row()), where the unit ends (pixels())
// and where the partial goes (slab(), part()): a slab policy, passed by value, answers all three.
//   PlainSlabs    grid (N, slabs); pixel i is row i of the image's map; parts[slab][n][64][512]
//   QuarterSlabs  grid (N, 4 nslab), blockIdx.y = quarter * nslab + slab; pixel i is row quarter_map_pixel(q, i) of
//                 the image's map — a pixel is 2 KB contiguous in the NHWC map, so the gather costs no coalescing,
//                 and a whole slab passes through registers: no table in LDS; parts[n][q][slab][64][512]
#pragma once

#include "vlad_common.h"

namespace oibl {

// dynamic LDS of the slab kernel: the chunk, four partial logit tiles, a, a / |x|, 32 norms, 64 column sums
constexpr int VLF_LDS = (32 * VLAD_XP + 4 * 32 * VLAD_LP + 2 * 32 * VLAD_LP + 32 + 64) * 4;

// a unit is an image
struct PlainSlabs {
  int P, slab_px;
  __device__ static int slab() { return blockIdx.y; }
  __device__ int pixels() const { return P; }
  __device__ const float* unit_base(const float* feat) const { return feat + (size_t)blockIdx.x * P * VLAD_C; }
  __device__ static int row(int i) { return i; }
  __device__ static float* part(float* parts) {
    return parts + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * VLAD_K * VLAD_C;
  }
};

// a unit is a quarter of an image of 2 hq x 2 wq pixels, a slab lies inside ONE quarter; row() counts in the image
struct QuarterSlabs {
  int hq, wq, nslab, slab_px;
  __device__ int quarter() const { return (int)blockIdx.y / nslab; }
  __device__ int slab() const { return (int)blockIdx.y % nslab; }
  __device__ int pixels() const { return hq * wq; }
  __device__ const float* unit_base(const float* f) const { return f + (size_t)blockIdx.x * 4 * pixels() * VLAD_C; }
  __device__ int row(int i) const { return quarter_map_pixel(quarter(), i, hq, wq); }
  __device__ float* part(float* parts) const {
    return parts + (((size_t)blockIdx.x * 4 + quarter()) * nslab + slab()) * VLAD_K * VLAD_C;
  }
};

template <class Slabs>
__device__ __forceinline__ void vlad_fused_slab(const Slabs map, const float* __restrict__ feat,
                                                const float* __restrict__ w, const float* __restrict__ centroids,
                                                float* __restrict__ parts, int normalize) {
  constexpr int C = VLAD_C, XP = VLAD_XP, LP = VLAD_LP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const x_s = reinterpret_cast<float*>(smem);             // [32][XP]
  float* const lp_s = x_s + 32 * XP;                              // [4 waves][32][LP] partial logits
  float* const a_s = lp_s + 4 * 32 * LP;                          // [32][LP] a[p][k]
  float* const a2_s = a_s + 32 * LP;                              // [32][LP] a[p][k] / |x_p|
  float* const inv_s = a2_s + 32 * LP;                            // [32]
  float* const cs_s = inv_s + 32;                                 // [64] sum_p a[p][k] of the slab
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l31 = lane & 31, kh = lane >> 5;
  const int p_lo = map.slab() * map.slab_px;
  const int p_hi = min(p_lo + map.slab_px, map.pixels());
  const float* fimg = map.unit_base(feat);

  f32x16_t acc[2][4];          // [cluster tile][channel tile of this wave's 128 channels]
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[kt][ct][r] = 0.f;
  float colsum = 0.f;          // threads 0..63
  // the assignment weights of this wave's 128 channels stay in registers for the whole slab (128 VGPRs): lane
  // (cluster l31 / 32 + l31, k half kh) holds w[cluster][128 wave + 8 j + 4 kh ..+3]
  float4 wr[2][16];
  {
    const float* wb = w + (size_t)l31 * C + 128 * wave + 4 * kh;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      wr[0][j] = *reinterpret_cast<const float4*>(wb + 8 * j);
      wr[1][j] = *reinterpret_cast<const float4*>(wb + (size_t)32 * C + 8 * j);
    }
  }
  // register prefetch of the NEXT chunk (one workgroup per CU has nothing else to hide the load latency behind)
  float4 pf[16];
  auto prefetch = [&](int p0) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int idx = (int)threadIdx.x + 256 * q;          // float4 index inside the chunk
      const int i = p0 + (idx >> 7), c4 = (idx & 127) * 4;  // pixel of the unit, channel
      pf[q] = make_float4(0.f, 0.f, 0.f, 0.f);             // a pixel beyond the slab reads as zeros (a = 0 below)
      if (i < p_hi) pf[q] = *reinterpret_cast<const float4*>(fimg + (size_t)map.row(i) * C + c4);
    }
  };
  prefetch(p_lo);

  for (int p0 = p_lo; p0 < p_hi; p0 += 32) {
    // ---- the chunk -> LDS
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int idx = (int)threadIdx.x + 256 * q;
      *reinterpret_cast<float4*>(x_s + (idx >> 7) * XP + (idx & 127) * 4) = pf[q];
    }
    __syncthreads();
    if (p0 + 32 < p_hi) prefetch(p0 + 32);
    // ---- 1 / |x_p|: eight threads per pixel, interleaved float4s
    const int px = (int)threadIdx.x >> 3, sub = (int)threadIdx.x & 7;
    {
      float ss = 0.f;
      if (normalize) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float4 v = *reinterpret_cast<const float4*>(x_s + px * XP + 4 * (sub + 8 * j));
          ss = fmaf(v.x, v.x, ss);
          ss = fmaf(v.y, v.y, ss);
          ss = fmaf(v.z, v.z, ss);
          ss = fmaf(v.w, v.w, ss);
        }
        ss += __shfl_xor(ss, 1, 64);
        ss += __shfl_xor(ss, 2, 64);
        ss += __shfl_xor(ss, 4, 64);
      }
      if (sub == 0) inv_s[px] = normalize ? 1.0f / fmaxf(sqrtf(ss), VLAD_EPS) : 1.0f;
    }
    // ---- partial logits of this wave's 128 channels: [32 pixels] x [64 clusters]
    {
      f32x16_t lg[2];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) lg[ct][r] = 0.f;
      const float* xa = x_s + l31 * XP + 128 * wave + 4 * kh;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float4 a = *reinterpret_cast<const float4*>(xa + 8 * j);
        const float4 b0 = wr[0][j], b1 = wr[1][j];
        lg[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, lg[0], 0, 0, 0);
        lg[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, lg[1], 0, 0, 0);
        lg[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, lg[0], 0, 0, 0);
        lg[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, lg[1], 0, 0, 0);
        lg[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, lg[0], 0, 0, 0);
        lg[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, lg[1], 0, 0, 0);
        lg[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, lg[0], 0, 0, 0);
        lg[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, lg[1], 0, 0, 0);
      }
      float* lw = lp_s + wave * 32 * LP;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) lw[acc_row(r, lane) * LP + 32 * ct + l31] = lg[ct][r];
    }
    __syncthreads();
    // ---- softmax over the 64 clusters: eight threads per pixel, eight clusters each
    {
      const float iv = inv_s[px];
      float l[8], mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int o = px * LP + sub * 8 + k;
        l[k] = (lp_s[o] + lp_s[32 * LP + o] + lp_s[2 * 32 * LP + o] + lp_s[3 * 32 * LP + o]) * iv;
        mx = fmaxf(mx, l[k]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
      float ssum = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        l[k] = expf(l[k] - mx);
        ssum += l[k];
      }
      ssum += __shfl_xor(ssum, 1, 64);
      ssum += __shfl_xor(ssum, 2, 64);
      ssum += __shfl_xor(ssum, 4, 64);
      const float is = (p0 + px < p_hi) ? 1.0f / ssum : 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float a = l[k] * is;
        a_s[px * LP + sub * 8 + k] = a;
        a2_s[px * LP + sub * 8 + k] = a * iv;
      }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
#pragma unroll
      for (int p = 0; p < 32; ++p) colsum += a_s[p * LP + threadIdx.x];
    }
    // ---- aggregation: acc[k][c] += sum_p (a[p][k] / |x_p|) x[p][c]
#pragma unroll 2
    for (int s2 = 0; s2 < 16; ++s2) {
      const int p = 2 * s2 + kh;
      const float av0 = a2_s[p * LP + l31], av1 = a2_s[p * LP + 32 + l31];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const float bv = x_s[p * XP + 128 * wave + 32 * ct + l31];
        acc[0][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, bv, acc[0][ct], 0, 0, 0);
        acc[1][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, bv, acc[1][ct], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < 64) cs_s[threadIdx.x] = colsum;
  __syncthreads();
  float* out = map.part(parts);
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int ch = 128 * wave + 32 * ct + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = 32 * kt + acc_row(r, lane);
        out[(size_t)k * C + ch] = acc[kt][ct][r] - cs_s[k] * centroids[(size_t)k * C + ch];
      }
    }
}

}  // namespace oibl
