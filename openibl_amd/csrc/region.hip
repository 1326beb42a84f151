// SFRS region similarities on gfx950: the forward-only region head of EmbedRegionNet.
// Reference behaviour: EmbedRegionNet._compute_region_sim (ibl/models/netvlad.py:123-186), called on the frozen
// model under torch.no_grad() by SFRSTrainer._forward (ibl/trainers.py:243-244).
//
// The conv5_3 map [h][w] of an image is cut into four quarters (q0 top-left, q1 top-right, q2 bottom-left, q3
// bottom-right, h/2 x w/2 pixels each); NetVLAD is aggregated per quarter; 9 regions are sums of quarters
//   [q0+q1+q2+q3, q0+q1, q2+q3, q0+q2, q1+q3, q0, q1, q2, q3]
// each intra-normalised per cluster and L2-normalised over the K*C vector; the score of an (anchor, pair) couple is
// the 9 x 9 table of dots of their region vectors.  Three pieces, four launches, the map read ONCE:
//
//   region_aggregate_kernel  netvlad_fused_kernel's scheme (netvlad.hip: chunks of 32 pixels x 512 channels in LDS,
//                            1 / |x_p|, logits and aggregation on v_mfma_f32_32x32x2_f32, softmax over the 64
//                            clusters, accumulators kept across the slab) on slabs of pixels that lie inside ONE
//                            quarter: pixel i of quarter q is map pixel (q / 2 * h/2 + i / (w/2)) * w + q % 2 * w/2 +
//                            i % (w/2) — a pixel is 2 KB contiguous in the NHWC map, so the gather costs no
//                            coalescing.  Writes parts[n][q][slab][64][512] = acc - (sum_p a[p][k]) centroids[k][c].
//   region_rowstats_kernel   one wave per (image, cluster) row: the slabs of each quarter added in slab order, the
//                            quarters added in the order listed above, per region the intra-norm of the row — written
//                            to the output — and the row's share of the vector's squared norm;
//   region_apply_kernel      the L2 norm over the 32768-vector, in place;
//   region_score_kernel      one workgroup per (tuple, pair, pair region): 9 dots of length K*C against the anchor's
//                            regions (the anchor's 9 x 128 KB stay in L2 across the tuple's pairs), fixed-order sums.
//
// The aggregation kernel repeats netvlad_fused_kernel's body instead of sharing it: the eval head's code object is
// pinned (its descriptors are compared bit for bit across releases), and the two differ in how a pixel index becomes
// an address, where the slab ends and where the partial goes — a shared body would branch on its caller in all three.
//
// The slab decomposition is a function of the map size alone and nothing is accumulated with atomics: an image's
// region vectors and a pair's scores are bit-identical whatever batch they are computed in.  fp32 arithmetic throughout.
#include "gemm_core.h"

namespace oibl {

constexpr int RG_XP = 516;           // floats per LDS row of the chunk: 16-byte aligned, +4 banks per pixel
constexpr int RG_LP = 65;            // pitch of the [32][64] logit / assignment tiles
constexpr int RG_LDS = (32 * RG_XP + 4 * 32 * RG_LP + 2 * 32 * RG_LP + 32 + 64) * 4;
constexpr int RG_SLAB_TARGET = 64;   // pixels per slab, at most: two chunks

__global__ __launch_bounds__(256) void region_aggregate_kernel(const float* __restrict__ feat,
                                                               const float* __restrict__ w,
                                                               const float* __restrict__ centroids,
                                                               float* __restrict__ parts, int hq, int wq, int nslab,
                                                               int slab_px, int normalize) {
  constexpr int C = 512;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const x_s = reinterpret_cast<float*>(smem);             // [32][RG_XP]
  float* const lp_s = x_s + 32 * RG_XP;                           // [4 waves][32][RG_LP] partial logits
  float* const a_s = lp_s + 4 * 32 * RG_LP;                       // [32][RG_LP] a[p][k]
  float* const a2_s = a_s + 32 * RG_LP;                           // [32][RG_LP] a[p][k] / |x_p|
  float* const inv_s = a2_s + 32 * RG_LP;                         // [32]
  float* const cs_s = inv_s + 32;                                 // [64] sum_p a[p][k] of the slab
  const int n = blockIdx.x;
  const int quarter = (int)blockIdx.y / nslab, slab = (int)blockIdx.y % nslab;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l31 = lane & 31, kh = lane >> 5;
  const int Pq = hq * wq;                                         // pixels of a quarter
  const int p_lo = slab * slab_px;
  int p_hi = p_lo + slab_px;
  if (p_hi > Pq) p_hi = Pq;
  const int wfull = 2 * wq;
  // first pixel of this quarter in the image's map
  const float* fimg = feat + ((size_t)n * 4 * Pq + (size_t)(quarter >> 1) * hq * wfull + (size_t)(quarter & 1) * wq) * C;

  f32x16_t acc[2][4];          // [cluster tile][channel tile of this wave's 128 channels]
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[kt][ct][r] = 0.f;
  float colsum = 0.f;          // threads 0..63
  // the assignment weights of this wave's 128 channels stay in registers for the whole slab: lane (cluster l31 /
  // 32 + l31, k half kh) holds w[cluster][128 wave + 8 j + 4 kh ..+3]
  float4 wr[2][16];
  {
    const float* wb = w + (size_t)l31 * C + 128 * wave + 4 * kh;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      wr[0][j] = *reinterpret_cast<const float4*>(wb + 8 * j);
      wr[1][j] = *reinterpret_cast<const float4*>(wb + (size_t)32 * C + 8 * j);
    }
  }
  // register prefetch of the NEXT chunk
  float4 pf[16];
  auto prefetch = [&](int p0) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int idx = (int)threadIdx.x + 256 * q;          // float4 index inside the chunk
      const int i = p0 + (idx >> 7), c4 = (idx & 127) * 4;  // pixel of the quarter, channel
      pf[q] = make_float4(0.f, 0.f, 0.f, 0.f);             // a pixel beyond the slab reads as zeros (a = 0 below)
      if (i < p_hi) {
        const int row = i / wq, col = i - row * wq;
        pf[q] = *reinterpret_cast<const float4*>(fimg + ((size_t)row * wfull + col) * C + c4);
      }
    }
  };
  prefetch(p_lo);

  for (int p0 = p_lo; p0 < p_hi; p0 += 32) {
    // ---- the chunk -> LDS
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int idx = (int)threadIdx.x + 256 * q;
      *reinterpret_cast<float4*>(x_s + (idx >> 7) * RG_XP + (idx & 127) * 4) = pf[q];
    }
    __syncthreads();
    if (p0 + 32 < p_hi) prefetch(p0 + 32);
    // ---- 1 / |x_p|: eight threads per pixel, interleaved float4s
    {
      const int px = (int)threadIdx.x >> 3, sub = (int)threadIdx.x & 7;
      float ss = 0.f;
      if (normalize) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float4 v = *reinterpret_cast<const float4*>(x_s + px * RG_XP + 4 * (sub + 8 * j));
          ss = fmaf(v.x, v.x, ss);
          ss = fmaf(v.y, v.y, ss);
          ss = fmaf(v.z, v.z, ss);
          ss = fmaf(v.w, v.w, ss);
        }
        ss += __shfl_xor(ss, 1, 64);
        ss += __shfl_xor(ss, 2, 64);
        ss += __shfl_xor(ss, 4, 64);
      }
      if (sub == 0) inv_s[px] = normalize ? 1.0f / fmaxf(sqrtf(ss), 1e-12f) : 1.0f;
    }
    // ---- partial logits of this wave's 128 channels: [32 pixels] x [64 clusters]
    {
      f32x16_t lg[2];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) lg[ct][r] = 0.f;
      const float* xa = x_s + l31 * RG_XP + 128 * wave + 4 * kh;
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
      float* lw = lp_s + wave * 32 * RG_LP;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) lw[acc_row(r, lane) * RG_LP + 32 * ct + l31] = lg[ct][r];
    }
    __syncthreads();
    // ---- softmax over the 64 clusters: eight threads per pixel, eight clusters each
    {
      const int px = (int)threadIdx.x >> 3, sub = (int)threadIdx.x & 7;
      const float iv = inv_s[px];
      float l[8], mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int o = px * RG_LP + sub * 8 + k;
        l[k] = (lp_s[o] + lp_s[32 * RG_LP + o] + lp_s[2 * 32 * RG_LP + o] + lp_s[3 * 32 * RG_LP + o]) * iv;
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
        a_s[px * RG_LP + sub * 8 + k] = a;
        a2_s[px * RG_LP + sub * 8 + k] = a * iv;
      }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
#pragma unroll
      for (int p = 0; p < 32; ++p) colsum += a_s[p * RG_LP + threadIdx.x];
    }
    // ---- aggregation: acc[k][c] += sum_p (a[p][k] / |x_p|) x[p][c]
#pragma unroll 2
    for (int s2 = 0; s2 < 16; ++s2) {
      const int p = 2 * s2 + kh;
      const float av0 = a2_s[p * RG_LP + l31], av1 = a2_s[p * RG_LP + 32 + l31];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const float bv = x_s[p * RG_XP + 128 * wave + 32 * ct + l31];
        acc[0][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, bv, acc[0][ct], 0, 0, 0);
        acc[1][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, bv, acc[1][ct], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < 64) cs_s[threadIdx.x] = colsum;
  __syncthreads();
  float* out = parts + (((size_t)n * 4 + quarter) * nslab + slab) * 64 * C;
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

// One wave per (image, cluster) row; lane l holds channels 4 l .. 4 l + 3 and 256 + 4 l .. 256 + 4 l + 3 of the four
// quarter rows.  out[n][region][k][c] = row * iv (intra-normalised), stats[n][region][k] = |row * iv|^2.
__global__ __launch_bounds__(256) void region_rowstats_kernel(const float* __restrict__ parts, int nslab,
                                                              float* __restrict__ out, float* __restrict__ stats,
                                                              long rows) {
  constexpr int C = 512, K = 64;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long n = row / K;
  const int k = (int)(row - n * K);
  float4 q[4][2];
#pragma unroll
  for (int qi = 0; qi < 4; ++qi) {
    const float* src = parts + (((size_t)n * 4 + qi) * nslab * K + k) * C + 4 * lane;
    q[qi][0] = *reinterpret_cast<const float4*>(src);
    q[qi][1] = *reinterpret_cast<const float4*>(src + 256);
    for (int z = 1; z < nslab; ++z) {       // slab order
      const float4 u0 = *reinterpret_cast<const float4*>(src + (size_t)z * K * C);
      const float4 u1 = *reinterpret_cast<const float4*>(src + (size_t)z * K * C + 256);
      q[qi][0] = make_float4(q[qi][0].x + u0.x, q[qi][0].y + u0.y, q[qi][0].z + u0.z, q[qi][0].w + u0.w);
      q[qi][1] = make_float4(q[qi][1].x + u1.x, q[qi][1].y + u1.y, q[qi][1].z + u1.z, q[qi][1].w + u1.w);
    }
  }
  // members of the 9 regions as bit masks over the quarters, added in ascending quarter order
  constexpr int MEMBERS[9] = {0xF, 0x3, 0xC, 0x5, 0xA, 0x1, 0x2, 0x4, 0x8};
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    float v[8];
    bool first = true;
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
      if (!(MEMBERS[r] >> qi & 1)) continue;
      const float u[8] = {q[qi][0].x, q[qi][0].y, q[qi][0].z, q[qi][0].w, q[qi][1].x, q[qi][1].y, q[qi][1].z, q[qi][1].w};
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = first ? u[e] : v[e] + u[e];
      first = false;
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s = fmaf(v[e], v[e], s);
    s = wave_sum(s);
    const float iv = 1.0f / fmaxf(sqrtf(s), 1e-12f);
    float s2 = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v[e] *= iv;
      s2 = fmaf(v[e], v[e], s2);
    }
    s2 = wave_sum(s2);
    float* o = out + (((size_t)n * 9 + r) * K + k) * C + 4 * lane;
    *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(o + 256) = make_float4(v[4], v[5], v[6], v[7]);
    if (lane == 0) stats[((size_t)n * 9 + r) * K + k] = s2;
  }
}

// vec *= 1 / max(sqrt(sum_k stats[vector][k]), eps): one wave per (vector, cluster) row, fixed-order wave reduction.
__global__ __launch_bounds__(256) void region_apply_kernel(float* __restrict__ out, const float* __restrict__ stats,
                                                           long rows) {
  constexpr int C = 512, K = 64;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);   // (image * 9 + region) * K + k
  if (row >= rows) return;
  const float t = wave_sum(stats[(row / K) * K + lane]);
  const float ginv = 1.0f / fmaxf(sqrtf(t), 1e-12f);
  float* o = out + row * C + 4 * lane;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float4 v = *reinterpret_cast<const float4*>(o + 256 * h);
    *reinterpret_cast<float4*>(o + 256 * h) = make_float4(v.x * ginv, v.y * ginv, v.z * ginv, v.w * ginv);
  }
}

// score[t][j][a][b] = <vec[t * per][a], vec[t * per + 1 + j][b]>: workgroup (b, j, t), a = 0..8.
// Thread i walks float4 i, i + 256, ... in order; wave butterfly; the four waves are added in wave order.
__global__ __launch_bounds__(256) void region_score_kernel(const float* __restrict__ vec, int per, int L,
                                                           float* __restrict__ score) {
  __shared__ float red[4][9];
  const int b = blockIdx.x, j = blockIdx.y, t = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* A = vec + (size_t)t * per * 9 * L;
  const float* B = vec + (((size_t)t * per + 1 + j) * 9 + b) * L;
  float acc[9];
#pragma unroll
  for (int a = 0; a < 9; ++a) acc[a] = 0.f;
  for (int i = (int)threadIdx.x * 4; i < L; i += 1024) {
    const float4 bv = *reinterpret_cast<const float4*>(B + i);
#pragma unroll
    for (int a = 0; a < 9; ++a) {
      const float4 av = *reinterpret_cast<const float4*>(A + (size_t)a * L + i);
      acc[a] = fmaf(av.x, bv.x, acc[a]);
      acc[a] = fmaf(av.y, bv.y, acc[a]);
      acc[a] = fmaf(av.z, bv.z, acc[a]);
      acc[a] = fmaf(av.w, bv.w, acc[a]);
    }
  }
#pragma unroll
  for (int a = 0; a < 9; ++a) {
    const float s = wave_sum(acc[a]);
    if (lane == 0) red[wave][a] = s;
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    const int a = threadIdx.x;
    const float s = ((red[0][a] + red[1][a]) + red[2][a]) + red[3][a];
    score[((((size_t)t * gridDim.y + j) * 9) + a) * 9 + b] = s;
  }
}

}  // namespace oibl

using namespace oibl;

extern "C" {

// the slab decomposition of a quarter: a function of the map size alone
static int rg_nslab(int h, int w) { return ((h / 2) * (w / 2) + RG_SLAB_TARGET - 1) / RG_SLAB_TARGET; }
static int rg_slab_px(int h, int w) { return ((h / 2) * (w / 2) + rg_nslab(h, w) - 1) / rg_nslab(h, w); }
static size_t rg_off_stats(int N, int h, int w, int K, int C) {
  return align_up((size_t)N * 4 * rg_nslab(h, w) * K * C * sizeof(float), 256);
}

size_t oibl_region_workspace_bytes(int N, int h, int w, int K, int C) {
  if (N <= 0 || h < 2 || w < 2 || (h & 1) || (w & 1) || K <= 0 || C <= 0) return 0;
  return rg_off_stats(N, h, w, K, C) + align_up((size_t)N * 9 * K * sizeof(float), 256);
}

int oibl_region_vlad_forward(const void* feat, int N, int h, int w, int K, int C, int precision,
                             const float* assign_w, const float* centroids, int normalize_input,
                             float* region_vlad, void* ws, size_t ws_bytes, void* stream) {
  OIBL_REQUIRE(feat && assign_w && centroids && region_vlad && ws, "region_vlad: null pointer");
  OIBL_REQUIRE(precision == OIBL_F32, "region_vlad: the feature map must be fp32 (OIBL_F32), got precision %d",
               precision);
  OIBL_REQUIRE(K == 64 && C == 512, "region_vlad: kernels are built for num_clusters = 64, dim = 512 (got %d, %d)",
               K, C);
  OIBL_REQUIRE(N > 0 && h > 0 && w > 0, "region_vlad: bad shape N=%d h=%d w=%d", N, h, w);
  OIBL_REQUIRE(!(h & 1) && !(w & 1), "region_vlad: the map is %d x %d, both sides must be even to cut quarters", h, w);
  OIBL_REQUIRE(4 * rg_nslab(h, w) <= 65535, "region_vlad: map %d x %d too large", h, w);
  OIBL_REQUIRE((uintptr_t)ws % 256 == 0 && (uintptr_t)feat % 16 == 0 && (uintptr_t)assign_w % 16 == 0 &&
                   (uintptr_t)region_vlad % 16 == 0,
               "region_vlad: workspace must be 256-byte, feat / assign_w / region_vlad 16-byte aligned");
  const size_t need = oibl_region_workspace_bytes(N, h, w, K, C);
  if (ws_bytes < need) {
    set_error("region_vlad: workspace %zu < required %zu bytes", ws_bytes, need);
    return OIBL_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  float* parts = (float*)ws;
  float* stats = (float*)((char*)ws + rg_off_stats(N, h, w, K, C));
  const int nslab = rg_nslab(h, w);
  OIBL_SET_MAX_LDS(region_aggregate_kernel, RG_LDS);
  hipLaunchKernelGGL(region_aggregate_kernel, dim3((unsigned)N, (unsigned)(4 * nslab)), dim3(256), RG_LDS, st,
                     (const float*)feat, assign_w, centroids, parts, h / 2, w / 2, nslab, rg_slab_px(h, w),
                     normalize_input);
  OIBL_LAUNCH_CHECK();
  const long rows = (long)N * K;
  hipLaunchKernelGGL(region_rowstats_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (const float*)parts,
                     nslab, region_vlad, stats, rows);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(region_apply_kernel, dim3((unsigned)((rows * 9 + 3) / 4)), dim3(256), 0, st, region_vlad,
                     (const float*)stats, rows * 9);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

int oibl_region_scores(const float* region_vlad, int T, int per_tuple, int L, float* score, void* stream) {
  OIBL_REQUIRE(region_vlad && score, "region_scores: null pointer");
  OIBL_REQUIRE(T > 0 && T <= 65535, "region_scores: bad tuple count %d", T);
  OIBL_REQUIRE(per_tuple >= 2 && per_tuple - 1 <= 65535,
               "region_scores: a tuple needs an anchor and at least one pair (got %d images per tuple)", per_tuple);
  OIBL_REQUIRE(L > 0 && L % 4 == 0, "region_scores: vector length must be a multiple of 4 (got %d)", L);
  OIBL_REQUIRE((uintptr_t)region_vlad % 16 == 0, "region_scores: region_vlad must be 16-byte aligned");
  hipLaunchKernelGGL(region_score_kernel, dim3(9, (unsigned)(per_tuple - 1), (unsigned)T), dim3(256), 0,
                     (hipStream_t)stream, region_vlad, per_tuple, L, score);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

}  // extern "C"
