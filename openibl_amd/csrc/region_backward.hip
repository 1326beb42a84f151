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
//
// The chunk kernels, the aggregation and the reduction are vlad_backward_core.h's bodies, the ones the plain head
// runs, instantiated with QuarterMap: a unit is a quarter (m = 4 n + q), the grid is (4 N, chunks), and a 32-entry
// table in LDS names the chunk's map pixels.
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
#include "vlad_backward_core.h"

namespace oibl {

constexpr int RGB_ASSIGN_LDS = VLB_ASSIGN_LDS + QuarterMap::TABLE_BYTES;
constexpr int RGB_CONTRACT_LDS = VLB_CONTRACT_LDS + QuarterMap::TABLE_BYTES;
constexpr int RGB_DX_LDS = VLB_DX_LDS + QuarterMap::TABLE_BYTES;

// the quarters of the 9 regions as bit masks
__device__ constexpr int RGB_MEMBERS[9] = {0xF, 0x3, 0xC, 0x5, 0xA, 0x1, 0x2, 0x4, 0x8};

// one workgroup per (quarter, chunk): blockIdx.x = 4 n + q, blockIdx.y the chunk
__global__ __launch_bounds__(256) void rgb_assign_kernel(const float* __restrict__ feat, const float* __restrict__ w,
                                                         float* __restrict__ rn, float* __restrict__ a, int hq, int wq,
                                                         int normalize) {
  vlad_assign(QuarterMap{hq, wq}, feat, w, rn, a, normalize);
}

__global__ __launch_bounds__(256) void rgb_contract_kernel(const float* __restrict__ feat, const float* __restrict__ B,
                                                           const float* __restrict__ dvc, const float* __restrict__ rn,
                                                           const float* a, float* out, int hq, int wq) {
  vlad_contract(QuarterMap{hq, wq}, feat, B, dvc, rn, a, out);
}

// MODE 0: segs 4, a segment is a quarter of seg_px = Pq pixels.  MODE 1: segs 1, the whole image, seg_px = 4 Pq.
template <int MODE>
__global__ __launch_bounds__(256) void rgb_aggregate_kernel(const float* __restrict__ feat,
                                                            const float* __restrict__ rn, const float* __restrict__ a,
                                                            const float* __restrict__ centroids,
                                                            float* __restrict__ out, double* __restrict__ A, int hq,
                                                            int wq, int segs, int seg_px) {
  vlad_aggregate<MODE>(QuarterMap{hq, wq}, feat, rn, a, centroids, out, A, segs, seg_px);
}

// one wave per (image, cluster): the region rows R_r,k = sum_{q in S_r} V_q,k in fp64 from the four fp32 quarter rows,
// st[(n 9 + r) K + k] = { |R_r,k| , |U_r,k|^2 , <U_r,k, G_r,k> }
__global__ __launch_bounds__(256) void rgb_rowstats_kernel(const float* __restrict__ V, const float* __restrict__ G,
                                                           double* __restrict__ st, long rows) {
  constexpr int C = VLAD_C, K = VLAD_K;
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
    ss = wave_sum_f64(ss);
    const double t = sqrt(ss);
    const double it = 1.0 / fmax(t, (double)VLAD_EPS);
    double s2 = 0.0, ug = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double u = rr[i] * it;
      s2 += u * u;
      ug += u * gg[i];
    }
    s2 = wave_sum_f64(s2);
    ug = wave_sum_f64(ug);
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
  constexpr int C = VLAD_C, K = VLAD_K;
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
    const double S2 = wave_sum_f64(st[3 * (vbase + lane) + 1]);
    const double UG = wave_sum_f64(st[3 * (vbase + lane) + 2]);
    const double gn = sqrt(S2);
    const double ig = 1.0 / fmax(gn, (double)VLAD_EPS);
    const double yg = gn < (double)VLAD_EPS ? 0.0 : UG * ig;         // <Y_r, G_r>; a clamped g is a constant
    const double t = st[3 * (vbase + k)], s2 = st[3 * (vbase + k) + 1], ug = st[3 * (vbase + k) + 2];
    const double it = 1.0 / fmax(t, (double)VLAD_EPS);
    const double fd = t < (double)VLAD_EPS ? 0.0 : (ug - s2 * ig * yg) * ig;   // <U_r,k, dU_r,k>; a clamped t likewise
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
    const double s = wave_sum_f64(dc[q]);
    if (lane == 0) dvc[(n * 4 + q) * K + k] = (float)s;
  }
}

__global__ __launch_bounds__(256) void rgb_dx_kernel(const float* __restrict__ feat, const float* __restrict__ rn,
                                                     const float* __restrict__ a, const float* __restrict__ ds,
                                                     const float* __restrict__ dV, const float* __restrict__ w,
                                                     float* __restrict__ grad_feat, int hq, int wq, int normalize) {
  vlad_dx(QuarterMap{hq, wq}, feat, rn, a, ds, dV, w, grad_feat, normalize);
}

__global__ __launch_bounds__(256) void rgb_reduce_kernel(const float* __restrict__ dWp, const double* __restrict__ dCp,
                                                         float* __restrict__ dW, float* __restrict__ dC, int N) {
  vlad_reduce(dWp, dCp, dW, dC, N);
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

// workspace: vlad_backward_layout with P = h w, four units (the quarters) and nine normalised vectors per image
static bool rgb_shape_ok(int N, int h, int w, int K, int C) {
  return N > 0 && N <= 65535 && h >= 2 && w >= 2 && !(h & 1) && !(w & 1) && K == VLAD_K && C == VLAD_C &&
         (long)h * w <= (1L << 22);            // chunks per quarter are a grid's y; N h w stays far below 2^31 rows
}

size_t oibl_region_backward_workspace_bytes(int N, int h, int w, int K, int C, int want_grad_feat) {
  if (!rgb_shape_ok(N, h, w, K, C)) return 0;
  const size_t P = (size_t)h * w;
  return vlad_backward_layout(N, P, 4, 9, want_grad_feat).total;
}

int oibl_region_vlad_backward(const void* feat, int N, int h, int w, int K, int C, int precision,
                              const float* assign_w, const float* centroids, int normalize_input,
                              const float* grad_region_vlad, float* grad_assign_w, float* grad_centroids,
                              float* grad_feat, void* ws, size_t ws_bytes, void* stream) {
  OIBL_REQUIRE(feat && assign_w && centroids && grad_region_vlad && ws, "region_vlad_backward: null pointer");
  OIBL_REQUIRE(grad_assign_w || grad_centroids || grad_feat, "region_vlad_backward: no output requested");
  OIBL_REQUIRE(precision == OIBL_F32, "region_vlad_backward: the feature map must be fp32 (OIBL_F32), got precision %d",
               precision);
  OIBL_REQUIRE(K == VLAD_K && C == VLAD_C,
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
  const VladBackwardLayout lay = vlad_backward_layout(N, P, 4, 9, grad_feat != nullptr);
  float* rn = (float*)wsb;
  float* a = (float*)(wsb + lay.a);
  float* V = (float*)(wsb + lay.v);
  double* stats = (double*)(wsb + lay.stats);
  double* A = (double*)(wsb + lay.A);
  float* dvc = (float*)(wsb + lay.dvc);
  float* dWp = (float*)(wsb + lay.dwp);
  double* dCp = grad_centroids ? (double*)(wsb + lay.dcp) : nullptr;
  float* ds = grad_feat ? (float*)(wsb + lay.ds) : a;
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
    hipLaunchKernelGGL(rgb_reduce_kernel, dim3(VLAD_K * VLAD_C / 256), dim3(256), 0, st, (const float*)dWp,
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
