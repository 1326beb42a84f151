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
//   region_aggregate_kernel  netvlad_fused_kernel's body (vlad_fused_slab, vlad_forward_core.h) over QuarterSlabs:
//                            slabs of pixels that lie inside ONE quarter, a quarter's pixel placed in the map by
//                            quarter_map_pixel (vlad_common.h, shared with the backward).  Writes
//                            parts[n][q][slab][64][512] = acc - (sum_p a[p][k]) centroids[k][c].
//   region_rowstats_kernel   one wave per (image, cluster) row: the slabs of each quarter added in slab order, the
//                            quarters added in the order listed above, per region the intra-norm of the row — written
//                            to the output — and the row's share of the vector's squared norm;
//   region_apply_kernel      the L2 norm over the 32768-vector, in place;
//   region_score_kernel      one workgroup per (tuple, pair, pair region): 9 dots of length K*C against the anchor's
//                            regions (the anchor's 9 x 128 KB stay in L2 across the tuple's pairs), fixed-order sums.
//
// The slab decomposition is a function of the map size alone and nothing is accumulated with atomics: an image's
// region vectors and a pair's scores are bit-identical whatever batch they are computed in.  fp32 arithmetic throughout.
#include "vlad_forward_core.h"

namespace oibl {

constexpr int RG_SLAB_TARGET = 64;   // pixels per slab, at most: two chunks

__global__ __launch_bounds__(256) void region_aggregate_kernel(const float* __restrict__ feat,
                                                               const float* __restrict__ w,
                                                               const float* __restrict__ centroids,
                                                               float* __restrict__ parts, int hq, int wq, int nslab,
                                                               int slab_px, int normalize) {
  vlad_fused_slab(QuarterSlabs{hq, wq, nslab, slab_px}, feat, w, centroids, parts, normalize);
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
  OIBL_SET_MAX_LDS(region_aggregate_kernel, VLF_LDS);
  hipLaunchKernelGGL(region_aggregate_kernel, dim3((unsigned)N, (unsigned)(4 * nslab)), dim3(256), VLF_LDS, st,
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
