// NetVLAD initialisation without a checkpoint: the two device pieces of the reference's flow that sit around the
// k-means of cluster.hip.
//
//   oibl_local_descriptors   examples/cluster.py:93-104: F.normalize(conv5 map, dim = channels), then S sampled
//                            positions per image.  One wave per OUTPUT row: only the N*S sampled pixels are read (a
//                            pixel is C contiguous elements of the NHWC map: one coalesced line per 64 channels), the
//                            squared norm is accumulated in fp32 — lane l takes channels l, l + 64, ... in order, then
//                            the wave butterfly — and the row is divided by max(|x|, 1e-12) as F.normalize does.  The
//                            map is never transposed and never normalised as a whole (1200 pixels per 480x640 image,
//                            100 of them wanted).
//   oibl_assign_gap          NetVLAD._init_params (ibl/models/netvlad.py:34-42): clsts / |clsts|, the K dot products
//                            of every training descriptor with them, and the gap between the largest and the second
//                            largest — whose mean sets alpha.  Three launches:
//       assign_normalize_kernel   one wave per centre: clsts_assign[k][:] = clsts[k][:] / |clsts[k]| and its transposed
//                                 copy ct[c][k] (k padded with zeros to a multiple of 64) in the workspace;
//       assign_gap_kernel         a workgroup of 4 waves stages ct in chunks of 64 channels in LDS AS [c][k]: lane =
//                                 cluster (passes of 64 for K > 64), so the 64 lanes of a read sit on 64 consecutive
//                                 banks.  Every wave owns 8 descriptors; their values are wave-uniform and come
//                                 through scalar loads, one centre value read from LDS feeds 8 FMAs.  A dot product is
//                                 ONE fp32 FMA chain over c = 0 .. C-1 in order.  Top-2 over the clusters: per lane over
//                                 its passes, then across lanes with the LANE of the first maximum masked out (not its
//                                 value: duplicate centres give a gap of exactly 0).  Lanes 0..7 store the 8 gaps with
//                                 one vector store.  No [K][n] matrix exists anywhere.
//       assign_gap_sum_kernel     one workgroup: thread j adds gap[j], gap[j + 256], ... in fp64 in ascending index,
//                                 thread 0 adds the 256 partials in ascending j.
//
// Nothing is accumulated with atomics and every order of summation is a function of the indices alone: clsts_assign,
// gap[] and gap_sum are bit-identical from run to run and do not depend on the launch geometry.  All arithmetic is
// exact fp32 FMA (fp64 for the sum).  50 000 x 64 x 512 is 3.3 GFLOP: latency / HBM bound, nothing for the matrix
// cores.
#include "common.h"

namespace oibl {

constexpr int AG_CC = 64;      // channels per LDS chunk
constexpr int AG_D = 8;        // descriptors per wave
constexpr int AG_WAVES = 4;    // waves per workgroup

template <typename T>
__global__ __launch_bounds__(256) void local_descriptors_kernel(const T* __restrict__ feat, int P, int C,
                                                                const int32_t* __restrict__ positions, int S,
                                                                float* __restrict__ out, long rows) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);     // n * S + s
  if (row >= rows) return;
  const long n = row / S;
  const int pos = positions[row];
  float* o = out + row * C;
  if (pos < 0 || pos >= P) {      // never dereferenced (the host wrapper refuses such a call): the row reads as NaN
    for (int c = lane; c < C; c += 64) o[c] = __builtin_nanf("");
    return;
  }
  const T* src = feat + ((size_t)n * P + pos) * C;
  float ss = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float v = Elem<T>::load(src + c);
    ss = fmaf(v, v, ss);
  }
  ss = wave_sum(ss);
  const float nrm = fmaxf(sqrtf(ss), 1e-12f);
  for (int c = lane; c < C; c += 64) o[c] = Elem<T>::load(src + c) / nrm;     // second read: the line is in cache
}

// wave k < K: clsts_assign[k][:] = clsts[k][:] / |clsts[k]|, ct[c][k] the same; waves K .. Kp-1 zero their column of ct
__global__ __launch_bounds__(256) void assign_normalize_kernel(const float* __restrict__ clsts, int K, int Kp, int C,
                                                               float* __restrict__ clsts_assign,
                                                               float* __restrict__ ct) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= Kp) return;
  if (k >= K) {
    for (int c = lane; c < C; c += 64) ct[(size_t)c * Kp + k] = 0.f;
    return;
  }
  const float* src = clsts + (size_t)k * C;
  float ss = 0.f;
  for (int c = lane; c < C; c += 64) ss = fmaf(src[c], src[c], ss);
  const float nrm = sqrtf(wave_sum(ss));
  for (int c = lane; c < C; c += 64) {
    const float v = src[c] / nrm;
    clsts_assign[(size_t)k * C + c] = v;
    ct[(size_t)c * Kp + k] = v;
  }
}

template <int PASSES>
__global__ __launch_bounds__(256) void assign_gap_kernel(const float* __restrict__ descs, int n,
                                                         const float* __restrict__ ct, int K, int C,
                                                         float* __restrict__ gap) {
  constexpr int Kp = 64 * PASSES;
  __shared__ __attribute__((aligned(16))) float cs[AG_CC * Kp];      // [c of the chunk][k]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long d0 = ((long)blockIdx.x * AG_WAVES + wave) * AG_D;         // first descriptor of this wave
  // rows beyond n are clamped to the last one: read, never stored
  const float* drow[AG_D];
#pragma unroll
  for (int d = 0; d < AG_D; ++d) drow[d] = descs + (size_t)(d0 + d < n ? d0 + d : n - 1) * C;
  float acc[PASSES][AG_D];
#pragma unroll
  for (int p = 0; p < PASSES; ++p)
#pragma unroll
    for (int d = 0; d < AG_D; ++d) acc[p][d] = 0.f;

  for (int c0 = 0; c0 < C; c0 += AG_CC) {
    __syncthreads();       // the previous chunk has been consumed
    {
      const float4* src = reinterpret_cast<const float4*>(ct + (size_t)c0 * Kp);
      float4* dst = reinterpret_cast<float4*>(cs);
#pragma unroll
      for (int i = 0; i < AG_CC * Kp / 4 / 256; ++i) dst[threadIdx.x + 256 * i] = src[threadIdx.x + 256 * i];
    }
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < AG_CC; ++j) {
      float cv[PASSES];
#pragma unroll
      for (int p = 0; p < PASSES; ++p) cv[p] = cs[j * Kp + 64 * p + lane];
#pragma unroll
      for (int d = 0; d < AG_D; ++d) {
        const float x = drow[d][c0 + j];        // wave-uniform address: a scalar load
#pragma unroll
        for (int p = 0; p < PASSES; ++p) acc[p][d] = fmaf(cv[p], x, acc[p][d]);
      }
    }
  }

  float mine = 0.f;
#pragma unroll
  for (int d = 0; d < AG_D; ++d) {
    // this lane's best and second best over its passes, the pass of the best masked by index
    float m1 = -INFINITY, m2 = -INFINITY;
    int p1 = -1;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const float v = 64 * p + lane < K ? acc[p][d] : -INFINITY;
      if (v > m1) {
        m1 = v;
        p1 = p;
      }
    }
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const float v = 64 * p + lane < K ? acc[p][d] : -INFINITY;
      if (p != p1) m2 = fmaxf(m2, v);
    }
    const float best = wave_max(m1);
    const unsigned long long holders = __builtin_amdgcn_ballot_w64(m1 == best);
    const int owner = holders ? __builtin_ctzll(holders) : -1;        // the first lane that holds the maximum
    const float second = wave_max(lane == owner ? m2 : m1);
    if (lane == d) mine = best - second;
  }
  if (lane < AG_D && d0 + lane < n) gap[d0 + lane] = mine;
}

__global__ __launch_bounds__(256) void assign_gap_sum_kernel(const float* __restrict__ gap, int n,
                                                             double* __restrict__ gap_sum) {
  __shared__ double part[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)gap[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int j = 0; j < 256; ++j) t += part[j];
    *gap_sum = t;
  }
}

}  // namespace oibl

using namespace oibl;

extern "C" {

int oibl_local_descriptors(const void* feat, int N, int P, int C, int precision, const int32_t* positions, int S,
                           float* out, void* stream) {
  OIBL_REQUIRE(feat && positions && out, "local_descriptors: null pointer");
  OIBL_REQUIRE(precision == OIBL_BF16 || precision == OIBL_F32,
               "local_descriptors: the feature map must be bf16 or fp32 (got precision %d)", precision);
  OIBL_REQUIRE(N > 0 && P > 0 && S > 0, "local_descriptors: bad shape N=%d P=%d S=%d", N, P, S);
  OIBL_REQUIRE(C > 0 && C % 64 == 0, "local_descriptors: C must be a positive multiple of 64 (got %d)", C);
  OIBL_REQUIRE((uintptr_t)feat % 4 == 0 && (uintptr_t)positions % 4 == 0 && (uintptr_t)out % 4 == 0,
               "local_descriptors: feat / positions / out must be 4-byte aligned");
  const long rows = (long)N * S;
  OIBL_REQUIRE((rows + 3) / 4 <= 0x7fffffffL, "local_descriptors: %ld rows are too many", rows);
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (precision == OIBL_BF16)
    hipLaunchKernelGGL(local_descriptors_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)feat, P, C, positions, S, out, rows);
  else
    hipLaunchKernelGGL(local_descriptors_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)feat,
                       P, C, positions, S, out, rows);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

// the transposed, zero-padded normalised centres ct [C][Kp], Kp = K rounded up to 64
size_t oibl_assign_gap_workspace_bytes(int n, int K, int C) {
  if (n < 1 || K < 2 || K > 256 || C <= 0 || C % 64) return 0;
  return align_up((size_t)C * ((K + 63) / 64 * 64) * sizeof(float), 256);
}

int oibl_assign_gap(const float* descs, int n, const float* clsts, int K, int C, float* clsts_assign, float* gap,
                    double* gap_sum, void* ws, size_t ws_bytes, void* stream) {
  OIBL_REQUIRE(descs && clsts && clsts_assign && gap && gap_sum && ws, "assign_gap: null pointer");
  OIBL_REQUIRE(n >= 1, "assign_gap: at least one descriptor is needed (n = %d)", n);
  OIBL_REQUIRE(K >= 2 && K <= 256, "assign_gap: num_clusters must be in [2, 256] (got %d): a gap needs two clusters", K);
  OIBL_REQUIRE(C > 0 && C % 64 == 0, "assign_gap: C must be a positive multiple of 64 (got %d)", C);
  OIBL_REQUIRE((uintptr_t)ws % 256 == 0 && (uintptr_t)descs % 4 == 0 && (uintptr_t)clsts % 4 == 0 &&
                   (uintptr_t)clsts_assign % 4 == 0 && (uintptr_t)gap % 4 == 0 && (uintptr_t)gap_sum % 8 == 0,
               "assign_gap: workspace must be 256-byte, gap_sum 8-byte, the float arrays 4-byte aligned");
  const size_t need = oibl_assign_gap_workspace_bytes(n, K, C);
  if (ws_bytes < need) {
    set_error("assign_gap: workspace %zu < required %zu bytes", ws_bytes, need);
    return OIBL_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int passes = (K + 63) / 64, Kp = 64 * passes;
  float* ct = (float*)ws;
  hipLaunchKernelGGL(assign_normalize_kernel, dim3((unsigned)(Kp / 4)), dim3(256), 0, st, clsts, K, Kp, C,
                     clsts_assign, ct);
  OIBL_LAUNCH_CHECK();
  const long per_wg = AG_WAVES * AG_D;
  const dim3 grid((unsigned)((n + per_wg - 1) / per_wg));
  switch (passes) {
    case 1:
      hipLaunchKernelGGL(assign_gap_kernel<1>, grid, dim3(256), 0, st, descs, n, (const float*)ct, K, C, gap);
      break;
    case 2:
      hipLaunchKernelGGL(assign_gap_kernel<2>, grid, dim3(256), 0, st, descs, n, (const float*)ct, K, C, gap);
      break;
    case 3:
      hipLaunchKernelGGL(assign_gap_kernel<3>, grid, dim3(256), 0, st, descs, n, (const float*)ct, K, C, gap);
      break;
    default:
      hipLaunchKernelGGL(assign_gap_kernel<4>, grid, dim3(256), 0, st, descs, n, (const float*)ct, K, C, gap);
      break;
  }
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(assign_gap_sum_kernel, dim3(1), dim3(256), 0, st, (const float*)gap, n, gap_sum);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

}  // extern "C"
