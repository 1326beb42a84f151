// The losses of an OpenIBL training step on gfx950, forward and backward, fused: what Trainer._get_loss
// (ibl/trainers.py:82-162), SFRSTrainer._get_loss / _get_hard_loss (:261-320) and the soft term of
// SFRSTrainer._forward (:256-257) compute as chains of elementwise and reduction launches under torch autograd.
//
// A tuple b is an anchor a, a positive x_0 = p and M negatives x_1 .. x_M, rows of L floats.  Per row i one scalar
//   sqdist   s_i = |a - x_i|^2          triplet   s_i = |a - x_i + 1e-6|^2  (torch's pairwise_distance)
//   dot      s_i = <a, x_i>
// is reduced over L; everything behind it is a function of the 1 + M scalars of a tuple:
//   triplet     loss = mean_{b,j} max(0, margin + sqrt(s_0) - sqrt(s_j))                          count = B M
//   sare_joint  z_i = -s_i (sqdist) | s_i / temp (dot);  loss = mean_b -log_softmax(z_0 .. z_M)[0]     count = B
//   sare_ind    loss = mean_{b,j} -log_softmax(z_0, z_j)[0] = mean softplus(z_j - z_0)            count = B M
// and the gradients are linear in the rows, with one coefficient u_i per row (the table the forward leaves):
//   sqdist, triplet   d_i = a - x_i (+ 1e-6):  dL/dx_i = u_i d_i,   dL/da = - sum_i u_i d_i
//   dot                                        dL/dx_i = u_i a,     dL/da =   sum_i u_i x_i
//   triplet     u_j = [hinge j active] / (count sqrt(s_j)),  u_0 = - (active hinges) / (count sqrt(s_0))
//   sare_joint  q = softmax(z):  w_j = q_j / count, w_0 = - sum_j w_j;   u = 2 w (sqdist) | w / temp (dot)
//   sare_ind    r_j = sigmoid(z_j - z_0):  w_j = r_j / count, w_0 = - sum_j w_j;   u as above
// The table holds 1 / count; the upstream gradient is read from the device by the backward.
//
//   tl_reduce_kernel   one workgroup per (chunk, row, tuple): TL_CHUNKS chunks of the row, the chunk's share of s_i
//                      accumulated in fp64, lanes then waves summed in a fixed order           -> partial[b][i][chunk]
//   tl_finish_kernel   one workgroup: the chunks of every row summed in chunk order, one thread per tuple for the
//                      hinge / softmax and the coefficients, the tuples' losses summed in a tree -> loss, table
//   tl_backward_kernel one thread per group of 4 columns of a tuple: the rows in order, fp64     -> the three gradients
//   sl_row_kernel      one workgroup per row of the soft-label loss: both softmaxes in fp64    -> row loss, table
//   sl_finish_kernel   the rows' losses summed in a tree, / B                                     -> loss
//   sl_backward_kernel table x upstream gradient                                                  -> grad_student
// A row is walked in groups of 4 consecutive floats whatever its alignment: a group is one 16-byte load where base
// and strides allow it and four (at the row's end fewer) 4-byte loads where they do not, summed in the same order —
// a strided view and its contiguous copy give the same bits.  No atomics anywhere; every decomposition depends on
// (B, M, L) alone, so results are bit-identical from run to run, and a tuple's coefficients depend on its batch
// mates through 1 / count only.
#include "common.h"

namespace oibl {

constexpr int TL_CHUNKS = 8;          // chunks per row of the L-reduction
constexpr int TL_MAX_NEG = 64;        // OIBL_TUPLE_LOSS_MAX_NEG
constexpr int SL_MAX_J = 4096;        // OIBL_SOFT_LABEL_MAX_J
constexpr double TL_PD_EPS = 1e-6;    // torch.nn.functional.pairwise_distance's eps

enum { TL_TRIPLET = 0, TL_SARE_JOINT = 1, TL_SARE_IND = 2 };
enum { TL_SQDIST = 0, TL_DOT = 1 };

struct TlRows {
  const float* a;       // [B] rows, stride sa
  const float* p;       // [B] rows, stride sp
  const float* n;       // [B][M] rows, strides snt (tuple), snr (row)
  long long sa, sp, snt, snr;
};

// the 4 floats of group g of a row of L floats (fewer at the row's end: the rest read as v[..] = 0, cnt says how many)
__device__ static inline int tl_load_group(const float* __restrict__ row, int g, int L, bool vec, float v[4]) {
  const long long e0 = 4LL * g;
  const int cnt = (long long)L - e0 >= 4 ? 4 : (int)((long long)L - e0);
  if (vec && cnt == 4) {
    const float4 t = *reinterpret_cast<const float4*>(row + e0);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = e < cnt ? row[e0 + e] : 0.f;
  }
  return cnt;
}

__device__ static inline void tl_store_group(float* __restrict__ row, int g, int cnt, bool vec, const double v[4]) {
  const long long e0 = 4LL * g;
  if (vec && cnt == 4) {
    *reinterpret_cast<float4*>(row + e0) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < cnt) row[e0 + e] = (float)v[e];
  }
}

__device__ static inline double tl_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the sum over the 256 threads of a workgroup, the same bits in every thread; red_s holds 4 doubles
__device__ static inline double tl_block_sum(double v, double* red_s) {
  v = tl_wave_sum(v);
  __syncthreads();                                   // red_s may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) red_s[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
}

__device__ static inline double tl_block_max(double v, double* red_s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red_s[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(red_s[0], red_s[1]), fmax(red_s[2], red_s[3]));
}

// blockIdx.x the chunk, blockIdx.y the row i (0 the positive, 1 + j negative j), blockIdx.z the tuple
__global__ __launch_bounds__(256) void tl_reduce_kernel(TlRows r, int L, int groups, int groups_per_chunk, int score,
                                                        double off, int vec, double* __restrict__ partial) {
  __shared__ double red_s[4];
  const int c = blockIdx.x, i = blockIdx.y, b = blockIdx.z;
  const int rows = gridDim.y;
  const float* ar = r.a + (long long)b * r.sa;
  const float* xr = i == 0 ? r.p + (long long)b * r.sp : r.n + (long long)b * r.snt + (long long)(i - 1) * r.snr;
  const int g_lo = c * groups_per_chunk;
  const int g_hi = min(groups, g_lo + groups_per_chunk);
  double acc = 0.0;
  for (int g = g_lo + (int)threadIdx.x; g < g_hi; g += 256) {
    float av[4], xv[4];
    const int cnt = tl_load_group(ar, g, L, vec != 0, av);
    tl_load_group(xr, g, L, vec != 0, xv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < cnt) {
        if (score == TL_DOT) {
          acc = fma((double)av[e], (double)xv[e], acc);
        } else {
          const double d = (double)av[e] - (double)xv[e] + off;
          acc = fma(d, d, acc);
        }
      }
    }
  }
  acc = tl_block_sum(acc, red_s);
  if (threadIdx.x == 0) partial[((size_t)b * rows + i) * TL_CHUNKS + c] = acc;
}

// one workgroup of 256 threads.  s [B][1 + M] is scratch, coef [B][1 + M] the table, loss one float.
__global__ __launch_bounds__(256) void tl_finish_kernel(const double* __restrict__ partial, double* __restrict__ s,
                                                        int B, int M, int mode, int score, double margin, double temp,
                                                        double* __restrict__ coef, float* __restrict__ loss) {
  __shared__ double red_s[4];
  const int rows = 1 + M;
  const long long total = (long long)B * rows;
  for (long long t = threadIdx.x; t < total; t += 256) {
    const double* src = partial + t * TL_CHUNKS;
    double v = src[0];
#pragma unroll
    for (int c = 1; c < TL_CHUNKS; ++c) v += src[c];
    s[t] = v;
  }
  __syncthreads();                                   // the workgroup's own global writes are visible behind it
  const double count = mode == TL_SARE_JOINT ? (double)B : (double)B * (double)M;
  const double inv_count = 1.0 / count;
  const double zscale = score == TL_DOT ? 1.0 / temp : -1.0;          // z_i = zscale s_i
  const double uscale = score == TL_DOT ? 1.0 / temp : 2.0;           // u_i = uscale w_i
  double lsum = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const double* sb = s + (size_t)b * rows;
    double* ub = coef + (size_t)b * rows;
    if (mode == TL_TRIPLET) {
      const double dp = sqrt(sb[0]);
      int active = 0;
      for (int j = 1; j <= M; ++j) {
        const double dn = sqrt(sb[j]);
        const double h = margin + dp - dn;
        const bool on = h >= 0.0;                    // clamp_min(., 0) passes the gradient at 0, as torch does
        if (on) lsum += h;
        active += on ? 1 : 0;
        ub[j] = on && dn > 0.0 ? inv_count / dn : 0.0;
      }
      ub[0] = active && dp > 0.0 ? -((double)active * inv_count) / dp : 0.0;
    } else if (mode == TL_SARE_JOINT) {
      const double z0 = zscale * sb[0];
      double mx = z0;
      for (int j = 1; j <= M; ++j) mx = fmax(mx, zscale * sb[j]);
      double Z = 0.0;
      for (int j = 0; j <= M; ++j) Z += exp(zscale * sb[j] - mx);
      lsum += log(Z) - (z0 - mx);
      double w0 = 0.0;
      for (int j = 1; j <= M; ++j) {
        const double w = exp(zscale * sb[j] - mx) / Z * inv_count;
        w0 -= w;
        ub[j] = uscale * w;
      }
      ub[0] = uscale * w0;
    } else {
      const double z0 = zscale * sb[0];
      double w0 = 0.0;
      for (int j = 1; j <= M; ++j) {
        const double z = zscale * sb[j] - z0;
        const double e = exp(-fabs(z));
        lsum += fmax(z, 0.0) + log1p(e);
        const double sig = z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
        const double w = sig * inv_count;
        w0 -= w;
        ub[j] = uscale * w;
      }
      ub[0] = uscale * w0;
    }
  }
  lsum = tl_block_sum(lsum, red_s);
  if (threadIdx.x == 0) *loss = (float)(lsum * inv_count);
}

// blockIdx.x * 128 + threadIdx.x the group of 4 columns, blockIdx.y the tuple.  A null gradient is not written.
__global__ __launch_bounds__(128) void tl_backward_kernel(TlRows r, int L, int groups, int M, int score, double off,
                                                          int vec_in, int vec_out, const double* __restrict__ coef,
                                                          const float* __restrict__ grad_loss, float* __restrict__ ga,
                                                          float* __restrict__ gp, float* __restrict__ gn) {
  __shared__ double u_s[1 + TL_MAX_NEG];
  const int b = blockIdx.y, rows = 1 + M;
  const double up = (double)*grad_loss;
  for (int i = threadIdx.x; i < rows; i += 128) u_s[i] = coef[(size_t)b * rows + i] * up;
  __syncthreads();
  const int g = (int)blockIdx.x * 128 + (int)threadIdx.x;
  if (g >= groups) return;
  float av[4], xv[4];
  const int cnt = tl_load_group(r.a + (long long)b * r.sa, g, L, vec_in != 0, av);
  double da[4] = {0.0, 0.0, 0.0, 0.0}, dx[4];
  for (int i = 0; i < rows; ++i) {
    const float* xr = i == 0 ? r.p + (long long)b * r.sp : r.n + (long long)b * r.snt + (long long)(i - 1) * r.snr;
    float* out = i == 0 ? (gp ? gp + (size_t)b * L : nullptr) : (gn ? gn + ((size_t)b * M + (i - 1)) * L : nullptr);
    const double u = u_s[i];
    if (score == TL_DOT) {
      if (ga) {
        tl_load_group(xr, g, L, vec_in != 0, xv);
#pragma unroll
        for (int e = 0; e < 4; ++e) da[e] = fma(u, (double)xv[e], da[e]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) dx[e] = u * (double)av[e];
    } else {
      tl_load_group(xr, g, L, vec_in != 0, xv);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        dx[e] = u * ((double)av[e] - (double)xv[e] + off);
        da[e] -= dx[e];
      }
    }
    if (out) tl_store_group(out, g, cnt, vec_out != 0, dx);
  }
  if (ga) tl_store_group(ga + (size_t)b * L, g, cnt, vec_out != 0, da);
}

// x / temp as ONE rounded product: the row maximum and the terms measured against it must be the same numbers.  The
// compiler contracts a product into the subtraction that follows it (an fma: the unrounded product) but not into the
// fmax, which leaves 1e-17 where an exact zero belongs; the empty asm makes the product opaque to that.
__device__ static inline double sl_scaled(float x, double inv_temp) {
  double v = (double)x * inv_temp;
  asm volatile("" : "+v"(v));
  return v;
}

// one workgroup per row: row_loss[b] = - sum_j softmax(t / tt)_j log_softmax(s / ts)_j,
// coef[b][j] = (softmax(s / ts)_j - softmax(t / tt)_j) / (B ts)
__global__ __launch_bounds__(256) void sl_row_kernel(const float* __restrict__ student, const float* __restrict__ teacher,
                                                     int B, int J, double ts, double tt, double* __restrict__ row_loss,
                                                     double* __restrict__ coef) {
  __shared__ double red_s[4];
  const int b = blockIdx.x;
  const float* sr = student + (size_t)b * J;
  const float* tr = teacher + (size_t)b * J;
  const double is = 1.0 / ts, it = 1.0 / tt;
  double ms = -INFINITY, mt = -INFINITY;
  for (int j = threadIdx.x; j < J; j += 256) {
    ms = fmax(ms, sl_scaled(sr[j], is));
    mt = fmax(mt, sl_scaled(tr[j], it));
  }
  ms = tl_block_max(ms, red_s);
  mt = tl_block_max(mt, red_s);
  double zs = 0.0, zt = 0.0;
  for (int j = threadIdx.x; j < J; j += 256) {
    zs += exp(sl_scaled(sr[j], is) - ms);
    zt += exp(sl_scaled(tr[j], it) - mt);
  }
  zs = tl_block_sum(zs, red_s);
  zt = tl_block_sum(zt, red_s);
  const double lzs = log(zs);
  const double cs = 1.0 / ((double)B * ts);
  double acc = 0.0;
  for (int j = threadIdx.x; j < J; j += 256) {
    const double ls = sl_scaled(sr[j], is) - ms;
    const double qt = exp(sl_scaled(tr[j], it) - mt) / zt;
    acc -= qt * (ls - lzs);
    coef[(size_t)b * J + j] = (exp(ls) / zs - qt) * cs;
  }
  acc = tl_block_sum(acc, red_s);
  if (threadIdx.x == 0) row_loss[b] = acc;
}

__global__ __launch_bounds__(256) void sl_finish_kernel(const double* __restrict__ row_loss, int B,
                                                        float* __restrict__ loss) {
  __shared__ double red_s[4];
  double acc = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) acc += row_loss[b];
  acc = tl_block_sum(acc, red_s);
  if (threadIdx.x == 0) *loss = (float)(acc / (double)B);
}

__global__ __launch_bounds__(256) void sl_backward_kernel(const double* __restrict__ coef, long long total,
                                                          const float* __restrict__ grad_loss,
                                                          float* __restrict__ grad_student) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < total) grad_student[t] = (float)(coef[t] * (double)*grad_loss);
}

}  // namespace oibl

using namespace oibl;

extern "C" {

// workspace: partial [B][1 + M][TL_CHUNKS] fp64 | s [B][1 + M] fp64
static size_t tl_off_s(size_t B, size_t M) { return align_up(B * (1 + M) * TL_CHUNKS * sizeof(double), 256); }

size_t oibl_tuple_loss_workspace_bytes(int B, int M) {
  if (B < 1 || B > 65535 || M < 1 || M > TL_MAX_NEG) return 0;
  return tl_off_s(B, M) + align_up((size_t)B * (1 + M) * sizeof(double), 256);
}

static bool tl_mode_ok(int mode, int score) {
  return mode >= TL_TRIPLET && mode <= TL_SARE_IND && (score == TL_SQDIST || score == TL_DOT);
}

// 16-byte loads need every row to start on a 16-byte boundary
static int tl_rows_vec(const TlRows& r) {
  return (uintptr_t)r.a % 16 == 0 && (uintptr_t)r.p % 16 == 0 && (uintptr_t)r.n % 16 == 0 && r.sa % 4 == 0 &&
         r.sp % 4 == 0 && r.snt % 4 == 0 && r.snr % 4 == 0;
}

#define TL_REQUIRE_SHAPE(what)                                                                                      \
  OIBL_REQUIRE(B >= 1 && B <= 65535, what ": 1 <= B <= 65535 tuples per call (got %d)", B);                        \
  OIBL_REQUIRE(M >= 1 && M <= TL_MAX_NEG, what ": 1 <= M <= %d negatives per tuple (got %d)", TL_MAX_NEG, M);      \
  OIBL_REQUIRE(L >= 1, what ": bad row length L=%d", L);                                                           \
  OIBL_REQUIRE(tl_mode_ok(mode, score), what ": unknown mode %d / score %d", mode, score);                         \
  OIBL_REQUIRE(stride_a >= 0 && stride_p >= 0 && stride_n_tuple >= 0 && stride_n_row >= 0,                         \
               what ": negative stride")

int oibl_tuple_loss_forward(const float* anchors, long long stride_a, const float* positives, long long stride_p,
                            const float* negatives, long long stride_n_tuple, long long stride_n_row, int B, int M,
                            int L, int mode, int score, double margin, double temp, float* loss, double* coef,
                            void* ws, size_t ws_bytes, void* stream) {
  OIBL_REQUIRE(anchors && positives && negatives && loss && coef && ws, "tuple_loss_forward: null pointer");
  TL_REQUIRE_SHAPE("tuple_loss_forward");
  OIBL_REQUIRE(mode == TL_TRIPLET || score == TL_SQDIST || temp > 0.0,
               "tuple_loss_forward: the temperature of the dot score must be positive (got %g)", temp);
  const size_t need = oibl_tuple_loss_workspace_bytes(B, M);
  if ((uintptr_t)ws % 256 != 0 || (uintptr_t)coef % 8 != 0) {
    set_error("tuple_loss_forward: workspace must be 256-byte aligned, the table 8-byte aligned");
    return OIBL_E_WORKSPACE;
  }
  if (ws_bytes < need) {
    set_error("tuple_loss_forward: workspace %zu < required %zu bytes", ws_bytes, need);
    return OIBL_E_WORKSPACE;
  }
  if (mode == TL_TRIPLET) score = TL_SQDIST;
  const TlRows r{anchors, positives, negatives, stride_a, stride_p, stride_n_tuple, stride_n_row};
  double* partial = (double*)ws;
  double* s = (double*)((char*)ws + tl_off_s(B, M));
  const int groups = (int)(((long long)L + 3) / 4);
  const int gpc = (groups + TL_CHUNKS - 1) / TL_CHUNKS;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tl_reduce_kernel, dim3(TL_CHUNKS, (unsigned)(1 + M), (unsigned)B), dim3(256), 0, st, r, L, groups,
                     gpc, score, mode == TL_TRIPLET ? TL_PD_EPS : 0.0, tl_rows_vec(r), partial);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(tl_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)partial, s, B, M, mode, score, margin,
                     temp, coef, loss);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

int oibl_tuple_loss_backward(const float* anchors, long long stride_a, const float* positives, long long stride_p,
                             const float* negatives, long long stride_n_tuple, long long stride_n_row, int B, int M,
                             int L, int mode, int score, const double* coef, const float* grad_loss,
                             float* grad_anchors, float* grad_positives, float* grad_negatives, void* stream) {
  OIBL_REQUIRE(anchors && positives && negatives && coef && grad_loss, "tuple_loss_backward: null pointer");
  OIBL_REQUIRE(grad_anchors || grad_positives || grad_negatives, "tuple_loss_backward: no output requested");
  TL_REQUIRE_SHAPE("tuple_loss_backward");
  OIBL_REQUIRE((uintptr_t)coef % 8 == 0, "tuple_loss_backward: the table must be 8-byte aligned");
  if (mode == TL_TRIPLET) score = TL_SQDIST;
  const TlRows r{anchors, positives, negatives, stride_a, stride_p, stride_n_tuple, stride_n_row};
  const int groups = (int)(((long long)L + 3) / 4);
  const int vec_out = L % 4 == 0 && (uintptr_t)grad_anchors % 16 == 0 && (uintptr_t)grad_positives % 16 == 0 &&
                      (uintptr_t)grad_negatives % 16 == 0;
  hipLaunchKernelGGL(tl_backward_kernel, dim3((unsigned)((groups + 127) / 128), (unsigned)B), dim3(128), 0,
                     (hipStream_t)stream, r, L, groups, M, score, mode == TL_TRIPLET ? TL_PD_EPS : 0.0, tl_rows_vec(r),
                     vec_out, coef, grad_loss, grad_anchors, grad_positives, grad_negatives);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

size_t oibl_soft_label_loss_workspace_bytes(int B, int J) {
  if (B < 1 || B > 65535 || J < 1 || J > SL_MAX_J) return 0;
  return align_up((size_t)B * sizeof(double), 256);
}

int oibl_soft_label_loss_forward(const float* student, const float* teacher, int B, int J, double temp_student,
                                 double temp_teacher, float* loss, double* coef, void* ws, size_t ws_bytes,
                                 void* stream) {
  OIBL_REQUIRE(student && teacher && loss && coef && ws, "soft_label_loss_forward: null pointer");
  OIBL_REQUIRE(B >= 1 && B <= 65535, "soft_label_loss_forward: 1 <= B <= 65535 rows per call (got %d)", B);
  OIBL_REQUIRE(J >= 1 && J <= SL_MAX_J, "soft_label_loss_forward: 1 <= J <= %d scores per row (got %d)", SL_MAX_J, J);
  OIBL_REQUIRE(temp_student > 0.0 && temp_teacher > 0.0,
               "soft_label_loss_forward: temperatures must be positive (got %g, %g)", temp_student, temp_teacher);
  if ((uintptr_t)ws % 256 != 0 || (uintptr_t)coef % 8 != 0) {
    set_error("soft_label_loss_forward: workspace must be 256-byte aligned, the table 8-byte aligned");
    return OIBL_E_WORKSPACE;
  }
  if (ws_bytes < oibl_soft_label_loss_workspace_bytes(B, J)) {
    set_error("soft_label_loss_forward: workspace %zu < required %zu bytes", ws_bytes,
              oibl_soft_label_loss_workspace_bytes(B, J));
    return OIBL_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sl_row_kernel, dim3((unsigned)B), dim3(256), 0, st, student, teacher, B, J, temp_student,
                     temp_teacher, (double*)ws, coef);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(sl_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, B, loss);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

int oibl_soft_label_loss_backward(const double* coef, int B, int J, const float* grad_loss, float* grad_student,
                                  void* stream) {
  OIBL_REQUIRE(coef && grad_loss && grad_student, "soft_label_loss_backward: null pointer");
  OIBL_REQUIRE(B >= 1 && B <= 65535, "soft_label_loss_backward: 1 <= B <= 65535 rows per call (got %d)", B);
  OIBL_REQUIRE(J >= 1 && J <= SL_MAX_J, "soft_label_loss_backward: 1 <= J <= %d scores per row (got %d)", SL_MAX_J, J);
  const long long total = (long long)B * J;
  hipLaunchKernelGGL(sl_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, coef,
                     total, grad_loss, grad_student);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

}  // extern "C"
