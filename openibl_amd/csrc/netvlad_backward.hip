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
// here.  The call is stateless: it recomputes r, a and V from the map, then (the bodies of the chunk kernels, the
// aggregation and the reduction are vlad_backward_core.h's, instantiated with PlainMap: a unit is an image)
//   nvb_assign_kernel        one workgroup per (32-pixel chunk, image): the chunk's 32 x 512 values in LDS, |x_p| and
//                            the logits in fp64 on the vector unit (see vlad_assign: its a is a more accurate
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
#include "vlad_backward_core.h"

namespace oibl {

constexpr int NVB_ASSIGN_LDS = VLB_ASSIGN_LDS + PlainMap::TABLE_BYTES;
constexpr int NVB_CONTRACT_LDS = VLB_CONTRACT_LDS + PlainMap::TABLE_BYTES;
constexpr int NVB_DX_LDS = VLB_DX_LDS + PlainMap::TABLE_BYTES;

// one workgroup per (32-pixel chunk, image): grid (chunks, N)
__global__ __launch_bounds__(256) void nvb_assign_kernel(const float* __restrict__ feat, const float* __restrict__ w,
                                                         float* __restrict__ rn, float* __restrict__ a, int P,
                                                         int normalize) {
  vlad_assign(PlainMap{P}, feat, w, rn, a, normalize);
}

__global__ __launch_bounds__(256) void nvb_contract_kernel(const float* __restrict__ feat, const float* __restrict__ B,
                                                           const float* __restrict__ dvc, const float* __restrict__ rn,
                                                           const float* a, float* out, int P) {
  vlad_contract(PlainMap{P}, feat, B, dvc, rn, a, out);
}

// one workgroup per (image, 64 channels): one segment per image, all its P pixels
template <int MODE>
__global__ __launch_bounds__(256) void nvb_aggregate_kernel(const float* __restrict__ feat,
                                                            const float* __restrict__ rn, const float* __restrict__ a,
                                                            const float* __restrict__ centroids,
                                                            float* __restrict__ out, double* __restrict__ A, int P) {
  vlad_aggregate<MODE>(PlainMap{P}, feat, rn, a, centroids, out, A, 1, P);
}

// one wave per (image, cluster) row of V: st[row] = { |V_k| , |U_k|^2 , <U_k, G_k> }, U_k = V_k / max(|V_k|, eps).
// This kernel and the next evaluate the two normalisations' backward in fp64 from the fp32 rows: a tuple loss makes
// the images' dC contributions cancel (its dL/dY sum to zero over a tuple; 60-fold on near-identical maps), which
// multiplies every fp32 rounding of a contribution by that factor.
__global__ __launch_bounds__(256) void nvb_rowstats_kernel(const float* __restrict__ V, const float* __restrict__ G,
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
__global__ __launch_bounds__(256) void nvb_dv_kernel(float* __restrict__ V, const float* __restrict__ G,
                                                     const double* __restrict__ st, const double* __restrict__ A,
                                                     const float* __restrict__ centroids, float* __restrict__ dvc,
                                                     double* __restrict__ dCp, long rows) {
  constexpr int C = VLAD_C, K = VLAD_K;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long n = row / K;
  const int k = (int)(row - n * K);
  // |U|_F^2 and <U, G> of the image: lane j holds cluster j's, the same fixed-order sum in every wave of the image
  const double S2 = wave_sum_f64(st[3 * (n * K + lane) + 1]);
  const double UG = wave_sum_f64(st[3 * (n * K + lane) + 2]);
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
    const double na = -A[row];
    double* o = dCp + row * C;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 4; ++i) o[256 * h + 4 * lane + i] = na * dv[4 * h + i];
  }
  if (lane == 0) dvc[row] = (float)dc;
}

__global__ __launch_bounds__(256) void nvb_dx_kernel(const float* __restrict__ feat, const float* __restrict__ rn,
                                                     const float* __restrict__ a, const float* __restrict__ ds,
                                                     const float* __restrict__ dV, const float* __restrict__ w,
                                                     float* __restrict__ grad_feat, int P, int normalize) {
  vlad_dx(PlainMap{P}, feat, rn, a, ds, dV, w, grad_feat, normalize);
}

__global__ __launch_bounds__(256) void nvb_reduce_kernel(const float* __restrict__ dWp, const double* __restrict__ dCp,
                                                         float* __restrict__ dW, float* __restrict__ dC, int N) {
  vlad_reduce(dWp, dCp, dW, dC, N);
}

}  // namespace oibl

using namespace oibl;

extern "C" {

// workspace: vlad_backward_layout with one unit (the image) and one normalised vector per image
size_t oibl_netvlad_backward_workspace_bytes(int N, int P, int K, int C, int want_grad_feat) {
  if (N <= 0 || P <= 0 || K != VLAD_K || C != VLAD_C) return 0;
  return vlad_backward_layout(N, P, 1, 1, want_grad_feat).total;
}

int oibl_netvlad_backward(const void* feat, int N, int P, int K, int C, int precision, const float* assign_w,
                          const float* centroids, int normalize_input, const float* grad_vlad_norm,
                          float* grad_assign_w, float* grad_centroids, float* grad_feat, void* ws, size_t ws_bytes,
                          void* stream) {
  OIBL_REQUIRE(feat && assign_w && centroids && grad_vlad_norm && ws, "netvlad_backward: null pointer");
  OIBL_REQUIRE(grad_assign_w || grad_centroids || grad_feat, "netvlad_backward: no output requested");
  OIBL_REQUIRE(precision == OIBL_F32, "netvlad_backward: the feature map must be fp32 (got precision %d)", precision);
  OIBL_REQUIRE(K == VLAD_K, "netvlad_backward: kernels are built for num_clusters = 64 (got %d)", K);
  OIBL_REQUIRE(C == VLAD_C, "netvlad_backward: kernels are built for dim = 512 (got %d)", C);
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
  const VladBackwardLayout lay = vlad_backward_layout(N, P, 1, 1, grad_feat != nullptr);
  float* rn = (float*)wsb;
  float* a = (float*)(wsb + lay.a);
  float* V = (float*)(wsb + lay.v);
  double* stats = (double*)(wsb + lay.stats);
  double* A = (double*)(wsb + lay.A);
  float* dvc = (float*)(wsb + lay.dvc);
  float* dWp = (float*)(wsb + lay.dwp);
  double* dCp = grad_centroids ? (double*)(wsb + lay.dcp) : nullptr;
  float* ds = grad_feat ? (float*)(wsb + lay.ds) : a;
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
    hipLaunchKernelGGL(nvb_reduce_kernel, dim3(VLAD_K * VLAD_C / 256), dim3(256), 0, st, (const float*)dWp,
                       (const double*)dCp, grad_assign_w, grad_centroids, N);
    OIBL_LAUNCH_CHECK();
  }
  return OIBL_OK;
}

}  // extern "C"
