// k-reciprocal re-ranking (Zhong et al., CVPR 2017) from descriptor rows on gfx950, without the n x n matrix.
// Reference behaviour: re_ranking (ibl/utils/rerank.py:32-100), which Evaluator.evaluate(rerank=True) and the SFRS
// trainer's update_sampler(rerank=True) apply to dense (Q+G) x (Q+G) numpy arrays on the host.
//
// X = [queries; gallery] has n = Q + G rows, D[i][j] = (|x_i|^2 + |x_j|^2) - 2 x_i.x_j, O[i][j] = D[i][j]^2 / m_i with
// m_i = max_r D[r][i]^2.  Per item the algorithm needs its k1 + 1 nearest neighbours (the fused top-k kernels of
// match.hip produce them), m_i and a few dozen gathered distances; everything after that is sparse.  Stages:
//
//   rerank_sqnorm_kernel    |x_i|^2, one wave per row;
//   rerank_extremes_kernel  the fp32 contraction X.X^T on gemm_core.h (128 x 128 tiles, v_mfma_f32_32x32x2_f32) with
//                           the epilogue folded into a running max of |D| per row: a workgroup walks a range of
//                           column tiles for one row tile and writes ONE partial per row;
//   rerank_rowmax_kernel    m_i = (max |D|)^2 over the partials (= max(dmax^2, dmin^2): D can be slightly negative
//                           on the diagonal);
//   rerank_sets_kernel      one wave per item, integers only: the k1-reciprocal set, expanded by the
//                           round(k1/2)-reciprocal set of each member when 3 |sub & base| > 2 |sub|, sorted unique
//                           at a fixed stride with a count;
//   rerank_weights_kernel   one wave per item: a fp32 dot of length d per member (HBM-bound gathers),
//                           V[i][c] = exp(-O[i][c]) / sum, summed in member order;
//   rerank_expand_kernel    k2 > 1: V[i] <- mean of the k2 sparse rows V[R(i)[:k2]], a merge by binary search,
//                           summed in rank order;
//   rerank_colcount / rerank_scan / rerank_fill / rerank_colsort   the inverted index: integer counts, an exclusive
//                           scan, a fill and a per-column sort by row, so that the index does not depend on the
//                           order in which the fill ran;
//   rerank_jaccard_kernel   one workgroup per query row: the row's columns in ascending order, the rows of one
//                           column added by distinct threads, a barrier between columns; then
//                           (1 - lambda) (1 - s / (2 - s)) + lambda O over the row of q x g squared distances, in
//                           place.  Every product, quotient and sum of that blend is rounded on its own (no fused
//                           multiply-add): it repeats numpy's fp32 operations one by one.
//
// No floating-point atomics anywhere: the result is bit-identical from run to run.
#include "gemm_core.h"

// No contraction of a * b + c into a fused multiply-add in this file: the blend and the weights repeat numpy's
// separately rounded fp32 operations (the stage tests compare bit for bit); dot products call fmaf by name.  The
// arithmetic is written with plain operators for that reason: the __fmul_rn / __fadd_rn wrappers of the HIP headers
// are compiled under the headers' own contraction mode and fuse again once they are inlined.
#pragma clang fp contract(off)

namespace oibl {

constexpr int RR_MAX_K1 = 31;       // k1 + 1 neighbours are one lane each of half a wave's ballot
constexpr int RR_MAX_K2 = 8;
constexpr int RR_MAX_STRIDE = 576;   // (k1 + 1) (round(k1 / 2) + 2) at k1 = 31
constexpr int RR_JACCARD_BLOCKS = 1024;

using RrCfg = GemmCfg<float, 2, 2, 2, 2>;

__device__ static inline int rr_wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void rerank_sqnorm_kernel(const float* __restrict__ x, float* __restrict__ out, int rows, int d) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (size_t)row * d;
  float s = 0.f;
  for (int i = lane * 4; i < d; i += 256) {
    const float4 v = *reinterpret_cast<const float4*>(xr + i);
    s = fmaf(v.x, v.x, s);
    s = fmaf(v.y, v.y, s);
    s = fmaf(v.z, v.z, s);
    s = fmaf(v.w, v.w, s);
  }
  s = wave_sum(s);
  if (lane == 0) out[row] = s;
}

struct RrExtParams {
  const float* x;    // [n][d]
  const float* xn;   // [n]
  float* pmax;       // [chunks][n]: max |D| of the row over the chunk's columns
  int n, d, tiles, tiles_per_chunk;
};

// Row tile blockIdx.x against the column tiles of chunk blockIdx.y; the distances live in the accumulators only.
// max_r D^2 = (max_r |D|)^2 (D can be slightly negative on the diagonal), so one running max of |D| per row serves.
// It is kept in LDS behind the two stages of the main loop, not in registers: after every column tile the 32 rows a
// lane holds are reduced over its 32 columns and folded into the row's slot by the one lane that owns it — the
// kernel keeps the register budget of the plain distance kernel (two workgroups per CU).
constexpr int RR_EXT_LDS = RrCfg::MAIN_LDS_BYTES + RrCfg::WAVES_N * RrCfg::BM * (int)sizeof(float);

__global__ __launch_bounds__(RrCfg::NTHREADS, 2) void rerank_extremes_kernel(RrExtParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using Cfg = RrCfg;
  const WaveCoord c = wave_coord<Cfg>();
  const int l31 = c.lane & 31;
  const long m0 = (long)blockIdx.x * Cfg::BM;
  const int t_lo = (int)blockIdx.y * p.tiles_per_chunk;
  const int t_hi = t_lo + p.tiles_per_chunk < p.tiles ? t_lo + p.tiles_per_chunk : p.tiles;
  float* red = reinterpret_cast<float*>(smem + Cfg::MAIN_LDS_BYTES);   // [wn][BM]
  red[threadIdx.x] = 0.f;                                              // NTHREADS = WAVES_N * BM
  static_assert(Cfg::NTHREADS == Cfg::WAVES_N * Cfg::BM, "one slot per thread");

  for (int tn = t_lo; tn < t_hi; ++tn) {
    const long n0 = (long)tn * Cfg::BN;
    RowLoader<Cfg, Cfg::A_LOADS> la;
    RowLoader<Cfg, Cfg::B_LOADS> lb;
    la.init(c, p.x, m0, p.n, (long)p.d * 4);   // rows beyond n are clamped to the last row, their results masked
    lb.init(c, p.x, n0, p.n, (long)p.d * 4);
    f32x16_t acc[Cfg::TM][Cfg::TN];
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
      for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    gemm_nt_mainloop<Cfg, true>(acc, smem, c, la, lb, p.d / Cfg::BK);   // (begins and ends on a barrier)
    float yn[Cfg::TN];
    bool ok[Cfg::TN];
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j) {
      const long col = n0 + (c.wn * Cfg::TN + j) * 32 + l31;
      ok[j] = col < p.n;
      yn[j] = ok[j] ? p.xn[col] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (c.wm * Cfg::TM + i) * 32 + acc_row(r, c.lane);
        const long m = m0 + row < p.n ? m0 + row : p.n - 1;
        const float xn = p.xn[m];
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < Cfg::TN; ++j) {
          const float dd = fabsf(fmaf(-2.0f, acc[i][j][r], xn + yn[j]));
          a = ok[j] ? fmaxf(a, dd) : a;
        }
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
        if (l31 == 0) red[c.wn * Cfg::BM + row] = fmaxf(red[c.wn * Cfg::BM + row], a);
      }
  }
  __syncthreads();
  if ((int)threadIdx.x < Cfg::BM && m0 + threadIdx.x < p.n) {
    const int t = threadIdx.x;
    p.pmax[(size_t)blockIdx.y * p.n + m0 + t] = fmaxf(red[t], red[Cfg::BM + t]);
  }
}

__global__ void rerank_rowmax_kernel(const float* __restrict__ pmax, int chunks, int n, float* __restrict__ rowmax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float a = 0.f;
  for (int ch = 0; ch < chunks; ++ch) a = fmaxf(a, pmax[(size_t)ch * n + i]);
  rowmax[i] = a * a;
}

// One wave (= one workgroup) per item.  rank [n][ld] int32: the nearest neighbours of every item, nearest first,
// -1 = none.  idx [n][stride] <- the sorted unique members, cnt [n] <- their number.
__global__ __launch_bounds__(64) void rerank_sets_kernel(const int32_t* __restrict__ rank, int ld, int n, int k1,
                                                         int half, int32_t* __restrict__ idx,
                                                         int32_t* __restrict__ cnt, int stride) {
  __shared__ int32_t mem_s[RR_MAX_STRIDE];
  __shared__ int32_t first_s[RR_MAX_STRIDE];
  __shared__ int32_t base_s[RR_MAX_K1 + 1];
  const int lane = threadIdx.x;
  const int i = blockIdx.x;
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int32_t* ri = rank + (size_t)i * ld;
  // the k1-reciprocal set: j in R(i) with i in R(j), in rank order
  const int j = lane <= k1 ? ri[lane] : -1;
  bool rec = false;
  if (j >= 0 && j < n) {
    const int32_t* rj = rank + (size_t)j * ld;
    for (int t = 0; t <= k1; ++t) rec |= rj[t] == i;
  }
  const unsigned long long bm = __builtin_amdgcn_ballot_w64(rec);
  const int nb = __builtin_popcountll(bm);
  if (rec) {
    const int pos = __builtin_popcountll(bm & lt);
    base_s[pos] = j;
    mem_s[pos] = j;
  }
  int total = nb;
  __syncthreads();
  for (int b = 0; b < nb; ++b) {
    const int cand = base_s[b];
    const int32_t* rc = rank + (size_t)cand * ld;
    const int q = lane <= half ? rc[lane] : -1;
    bool in_sub = false;
    if (q >= 0 && q < n) {
      const int32_t* rq = rank + (size_t)q * ld;
      for (int t = 0; t <= half; ++t) in_sub |= rq[t] == cand;
    }
    bool in_base = false;
    if (in_sub)
      for (int t = 0; t < nb; ++t) in_base |= base_s[t] == q;
    const unsigned long long sm = __builtin_amdgcn_ballot_w64(in_sub);
    const int ns = __builtin_popcountll(sm);
    const int ni = __builtin_popcountll(__builtin_amdgcn_ballot_w64(in_base));
    if (3 * ni > 2 * ns) {            // len(intersect) > 2/3 len(sub), in integers
      if (in_sub) mem_s[total + __builtin_popcountll(sm & lt)] = q;
      total += ns;
    }
  }
  __syncthreads();
  // unique: the first occurrence of every value; its place is the number of smaller first occurrences
  for (int e = lane; e < total; e += 64) {
    const int v = mem_s[e];
    bool first = true;
    for (int t = 0; t < e; ++t) first &= mem_s[t] != v;
    first_s[e] = first;
  }
  __syncthreads();
  int mine = 0;
  for (int e = lane; e < total; e += 64) {
    if (!first_s[e]) continue;
    const int v = mem_s[e];
    int pos = 0;
    for (int t = 0; t < total; ++t) pos += (first_s[t] && mem_s[t] < v) ? 1 : 0;
    idx[(size_t)i * stride + pos] = v;
    ++mine;
  }
  mine = rr_wave_sum_int(mine);
  if (lane == 0) cnt[i] = mine;
}

// One wave per item: val[i][t] = exp(-O[i][idx[i][t]]) / sum_t, O[i][c] = D[i][c]^2 / rowmax[i].
__global__ __launch_bounds__(64) void rerank_weights_kernel(const float* __restrict__ x, const float* __restrict__ xn,
                                                            const float* __restrict__ rowmax, int d,
                                                            const int32_t* __restrict__ idx,
                                                            const int32_t* __restrict__ cnt, int stride,
                                                            float* __restrict__ val) {
  __shared__ float w_s[RR_MAX_STRIDE];
  __shared__ float sum_s;
  const int lane = threadIdx.x;
  const int i = blockIdx.x;
  const int ci = cnt[i];
  const float* xi = x + (size_t)i * d;
  const float ni = xn[i], mi = rowmax[i];
  for (int t = 0; t < ci; ++t) {
    const int c = idx[(size_t)i * stride + t];
    const float* xc = x + (size_t)c * d;
    float s = 0.f;
    for (int k = lane * 4; k < d; k += 256) {
      const float4 a = *reinterpret_cast<const float4*>(xi + k);
      const float4 b = *reinterpret_cast<const float4*>(xc + k);
      s = fmaf(a.x, b.x, s);
      s = fmaf(a.y, b.y, s);
      s = fmaf(a.z, b.z, s);
      s = fmaf(a.w, b.w, s);
    }
    s = wave_sum(s);
    if (lane == 0) {
      const float dd = fmaf(-2.0f, s, ni + xn[c]);
      w_s[t] = expf(-((dd * dd) / mi));
    }
  }
  __syncthreads();
  if (lane == 0) {
    float s = 0.f;
    for (int t = 0; t < ci; ++t) s += w_s[t];   // member order
    sum_s = s;
  }
  __syncthreads();
  const float s = sum_s;
  for (int t = lane; t < ci; t += 64) val[(size_t)i * stride + t] = w_s[t] / s;
}

// first position p of the sorted list a[0..len) with a[p] >= c
__device__ static inline int rr_lower_bound(const int32_t* a, int len, int c) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < c) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One wave per item: the merge of the sparse rows of its k2 nearest items (itself among them), each value the
// sum over those rows in rank order divided by their number (k2, or fewer when the rank list ends in -1).
// pre_s [k2][stride + 1]: per source row, the number of columns among its first t that no earlier source row holds.
__global__ __launch_bounds__(64) void rerank_expand_kernel(const int32_t* __restrict__ rank, int ld, int n, int k2,
                                                           const int32_t* __restrict__ idx,
                                                           const float* __restrict__ val,
                                                           const int32_t* __restrict__ cnt, int stride,
                                                           int32_t* __restrict__ idx2, float* __restrict__ val2,
                                                           int32_t* __restrict__ cnt2, int stride2) {
  extern __shared__ int32_t pre_s[];
  __shared__ int32_t row_s[RR_MAX_K2], len_s[RR_MAX_K2];
  const int lane = threadIdx.x;
  const int i = blockIdx.x;
  const int P = stride + 1;
  const int src = lane < k2 ? rank[(size_t)i * ld + lane] : -1;
  const bool ok = src >= 0 && src < n;
  if (lane < k2) {
    row_s[lane] = ok ? src : 0;
    len_s[lane] = ok ? cnt[src] : 0;
  }
  // the mean is taken over the items the list holds: n < k2 leaves -1 entries, which np.mean never sees
  const float fk2 = (float)__builtin_popcountll(__builtin_amdgcn_ballot_w64(ok));
  __syncthreads();
  for (int r = 0; r < k2; ++r) {
    const int32_t* a = idx + (size_t)row_s[r] * stride;
    for (int t = lane; t < len_s[r]; t += 64) {
      const int c = a[t];
      bool first = true;
      for (int r2 = 0; r2 < r; ++r2) {
        const int32_t* b = idx + (size_t)row_s[r2] * stride;
        const int p = rr_lower_bound(b, len_s[r2], c);
        if (p < len_s[r2] && b[p] == c) first = false;
      }
      pre_s[r * P + t + 1] = first ? 1 : 0;
    }
  }
  __syncthreads();
  if (lane < k2) {
    int32_t* pr = pre_s + lane * P;
    pr[0] = 0;
    for (int t = 0; t < len_s[lane]; ++t) pr[t + 1] += pr[t];
  }
  __syncthreads();
  for (int r = 0; r < k2; ++r) {
    const int32_t* a = idx + (size_t)row_s[r] * stride;
    for (int t = lane; t < len_s[r]; t += 64) {
      if (pre_s[r * P + t + 1] == pre_s[r * P + t]) continue;   // an earlier row holds this column
      const int c = a[t];
      int pos = 0;
      float s = 0.f;
      for (int r2 = 0; r2 < k2; ++r2) {
        const int32_t* b = idx + (size_t)row_s[r2] * stride;
        const int p = rr_lower_bound(b, len_s[r2], c);
        pos += pre_s[r2 * P + p];
        if (p < len_s[r2] && b[p] == c) s += val[(size_t)row_s[r2] * stride + p];
      }
      idx2[(size_t)i * stride2 + pos] = c;
      val2[(size_t)i * stride2 + pos] = s / fk2;
    }
  }
  if (lane == 0) {
    int total = 0;
    for (int r = 0; r < k2; ++r) total += pre_s[r * P + len_s[r]];
    cnt2[i] = total;
  }
}

// ---- inverted index: col_off [n + 1], the rows (ascending) and values of every column -------------------------
__global__ void rerank_colcount_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ cnt, int stride,
                                       int n, int32_t* __restrict__ colcnt) {
  const int i = blockIdx.x;
  for (int t = threadIdx.x; t < cnt[i]; t += blockDim.x) atomicAdd(&colcnt[idx[(size_t)i * stride + t]], 1);
}

// exclusive scan of colcnt [n] -> off [n + 1]; one workgroup of 1024 threads, a contiguous piece each
__global__ __launch_bounds__(1024) void rerank_scan_kernel(const int32_t* __restrict__ colcnt, int n,
                                                           int32_t* __restrict__ off) {
  __shared__ int32_t part_s[1024];
  const int t = threadIdx.x;
  const int per = (n + 1023) / 1024;
  const int lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
  int s = 0;
  for (int e = lo; e < hi; ++e) s += colcnt[e];
  part_s[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = t >= o ? part_s[t - o] : 0;
    __syncthreads();
    part_s[t] += v;
    __syncthreads();
  }
  int run = part_s[t] - s;
  for (int e = lo; e < hi; ++e) {
    off[e] = run;
    run += colcnt[e];
  }
  if (t == 1023) off[n] = part_s[1023];
}

__global__ void rerank_fill_kernel(const int32_t* __restrict__ idx, const float* __restrict__ val,
                                   const int32_t* __restrict__ cnt, int stride, const int32_t* __restrict__ off,
                                   int32_t* __restrict__ cursor, int32_t* __restrict__ tmp_row,
                                   float* __restrict__ tmp_val) {
  const int i = blockIdx.x;
  for (int t = threadIdx.x; t < cnt[i]; t += blockDim.x) {
    const int c = idx[(size_t)i * stride + t];
    const int p = off[c] + atomicAdd(&cursor[c], 1);
    tmp_row[p] = i;
    tmp_val[p] = val[(size_t)i * stride + t];
  }
}

// one wave per column: a row's place is the number of smaller rows of the column (rows are distinct)
__global__ __launch_bounds__(64) void rerank_colsort_kernel(const int32_t* __restrict__ off,
                                                            const int32_t* __restrict__ tmp_row,
                                                            const float* __restrict__ tmp_val,
                                                            int32_t* __restrict__ inv_row,
                                                            float* __restrict__ inv_val) {
  const int c = blockIdx.x;
  const int b = off[c], len = off[c + 1] - b;
  for (int e = threadIdx.x; e < len; e += 64) {
    const int r = tmp_row[b + e];
    int pos = 0;
    for (int t = 0; t < len; ++t) pos += tmp_row[b + t] < r ? 1 : 0;
    inv_row[b + pos] = r;
    inv_val[b + pos] = tmp_val[b + e];
  }
}

// Workgroup b serves query rows b, b + gridDim.x, ...; s = its G floats of scratch, zero on entry and on exit.
__global__ __launch_bounds__(256) void rerank_jaccard_kernel(const int32_t* __restrict__ idx,
                                                             const float* __restrict__ val,
                                                             const int32_t* __restrict__ cnt, int stride,
                                                             const int32_t* __restrict__ off,
                                                             const int32_t* __restrict__ inv_row,
                                                             const float* __restrict__ inv_val,
                                                             const float* __restrict__ rowmax, int Q, int G,
                                                             float one_minus_lambda, float lambda,
                                                             float* __restrict__ dist, size_t ldd,
                                                             float* __restrict__ scratch) {
  float* s = scratch + (size_t)blockIdx.x * G;
  for (int i = blockIdx.x; i < Q; i += gridDim.x) {
    const int ci = cnt[i];
    for (int t = 0; t < ci; ++t) {                       // columns of the row, ascending
      const int c = idx[(size_t)i * stride + t];
      const float v = val[(size_t)i * stride + t];
      const int e = off[c + 1];
      for (int p = off[c] + (int)threadIdx.x; p < e; p += 256) {
        const int j = inv_row[p] - Q;                    // distinct rows: distinct threads, distinct addresses
        if (j >= 0) s[j] = s[j] + fminf(v, inv_val[p]);
      }
      __syncthreads();
    }
    const float mi = rowmax[i];
    float* out = dist + (size_t)i * ldd;
    for (int j = threadIdx.x; j < G; j += 256) {
      const float sv = s[j];
      s[j] = 0.f;
      const float dd = out[j];
      const float o = (dd * dd) / mi;
      const float jac = 1.0f - sv / (2.0f - sv);
      out[j] = jac * one_minus_lambda + o * lambda;
    }
    __syncthreads();
  }
}

}  // namespace oibl

using namespace oibl;

extern "C" {

static int rr_tiles(int n) { return (n + RrCfg::BM - 1) / RrCfg::BM; }
// column tiles per workgroup: about 4096 workgroups in all, so that the partials stay a few floats per row
static int rr_tiles_per_chunk(int n) {
  const int tiles = rr_tiles(n);
  int chunks = (4096 + tiles - 1) / tiles;
  if (chunks > tiles) chunks = tiles;
  if (chunks > 65535) chunks = 65535;
  return (tiles + chunks - 1) / chunks;
}
static int rr_chunks(int n) { return (rr_tiles(n) + rr_tiles_per_chunk(n) - 1) / rr_tiles_per_chunk(n); }

int oibl_rerank_set_stride(int k1, int half) {
  if (k1 < 1 || k1 > RR_MAX_K1 || half < 0 || half > k1 || (k1 + 1) * (half + 2) > RR_MAX_STRIDE) return 0;
  return (k1 + 1) * (half + 2);
}

size_t oibl_rerank_row_extremes_workspace_bytes(int n, int d) {
  if (n <= 0 || d <= 0) return 0;
  return align_up((size_t)rr_chunks(n) * n * sizeof(float), 256);
}

int oibl_rerank_row_extremes(const float* x, int n, int d, float* norms, float* rowmax, void* ws, size_t ws_bytes,
                             void* stream) {
  OIBL_REQUIRE(x && norms && rowmax && ws, "rerank_row_extremes: null pointer");
  OIBL_REQUIRE(n > 0 && d > 0 && d % 32 == 0, "rerank_row_extremes: unsupported shape n=%d d=%d (d %% 32 == 0)", n, d);
  OIBL_REQUIRE((uintptr_t)ws % 256 == 0 && (uintptr_t)x % 16 == 0,
               "rerank_row_extremes: workspace must be 256-byte, x 16-byte aligned");
  OIBL_REQUIRE(rr_tiles(n) <= 0x7fffff, "rerank_row_extremes: n=%d too large", n);
  const size_t need = oibl_rerank_row_extremes_workspace_bytes(n, d);
  if (ws_bytes < need) {
    set_error("rerank_row_extremes: workspace %zu < required %zu bytes", ws_bytes, need);
    return OIBL_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rerank_sqnorm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, x, norms, n, d);
  OIBL_LAUNCH_CHECK();
  RrExtParams p;
  p.x = x;
  p.xn = norms;
  p.pmax = (float*)ws;
  p.n = n;
  p.d = d;
  p.tiles = rr_tiles(n);
  p.tiles_per_chunk = rr_tiles_per_chunk(n);
  const int chunks = rr_chunks(n);
  OIBL_SET_MAX_LDS(rerank_extremes_kernel, RR_EXT_LDS);
  hipLaunchKernelGGL(rerank_extremes_kernel, dim3((unsigned)p.tiles, (unsigned)chunks), dim3(RrCfg::NTHREADS),
                     RR_EXT_LDS, st, p);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(rerank_rowmax_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     (const float*)p.pmax, chunks, n, rowmax);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

int oibl_rerank_sets(const int32_t* rank, int ld, int n, int k1, int half, int32_t* idx, int32_t* cnt, int stride,
                     void* stream) {
  OIBL_REQUIRE(rank && idx && cnt, "rerank_sets: null pointer");
  OIBL_REQUIRE(k1 >= 1 && k1 <= RR_MAX_K1, "rerank_sets: k1 = %d outside 1..%d", k1, RR_MAX_K1);
  OIBL_REQUIRE(oibl_rerank_set_stride(k1, half) > 0, "rerank_sets: half = %d: (k1 + 1)(half + 2) must stay within %d",
               half, RR_MAX_STRIDE);
  OIBL_REQUIRE(n > 0 && ld >= k1 + 1, "rerank_sets: bad shape n=%d, %d ranks per item (needs k1 + 1 = %d)", n, ld,
               k1 + 1);
  OIBL_REQUIRE(stride >= oibl_rerank_set_stride(k1, half), "rerank_sets: stride %d below (k1 + 1)(half + 2) = %d",
               stride, oibl_rerank_set_stride(k1, half));
  hipLaunchKernelGGL(rerank_sets_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, rank, ld, n, k1, half,
                     idx, cnt, stride);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

int oibl_rerank_weights(const float* x, const float* norms, const float* rowmax, int n, int d, const int32_t* idx,
                        const int32_t* cnt, int stride, float* val, void* stream) {
  OIBL_REQUIRE(x && norms && rowmax && idx && cnt && val, "rerank_weights: null pointer");
  OIBL_REQUIRE(n > 0 && d > 0 && d % 4 == 0, "rerank_weights: unsupported shape n=%d d=%d", n, d);
  OIBL_REQUIRE(stride >= 1 && stride <= RR_MAX_STRIDE, "rerank_weights: stride %d outside 1..%d", stride,
               RR_MAX_STRIDE);
  OIBL_REQUIRE((uintptr_t)x % 16 == 0, "rerank_weights: x must be 16-byte aligned");
  hipLaunchKernelGGL(rerank_weights_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, x, norms, rowmax, d,
                     idx, cnt, stride, val);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

int oibl_rerank_expand(const int32_t* rank, int ld, int n, int k2, const int32_t* idx, const float* val,
                       const int32_t* cnt, int stride, int32_t* idx2, float* val2, int32_t* cnt2, int stride2,
                       void* stream) {
  OIBL_REQUIRE(rank && idx && val && cnt && idx2 && val2 && cnt2, "rerank_expand: null pointer");
  OIBL_REQUIRE(k2 >= 1 && k2 <= RR_MAX_K2, "rerank_expand: k2 = %d outside 1..%d", k2, RR_MAX_K2);
  OIBL_REQUIRE(n > 0 && ld >= k2, "rerank_expand: bad shape n=%d, %d ranks per item (needs k2 = %d)", n, ld, k2);
  OIBL_REQUIRE(stride >= 1 && stride <= RR_MAX_STRIDE, "rerank_expand: stride %d outside 1..%d", stride,
               RR_MAX_STRIDE);
  OIBL_REQUIRE((long)stride2 >= (long)k2 * stride, "rerank_expand: output stride %d below k2 * stride = %ld", stride2,
               (long)k2 * stride);
  const size_t lds = (size_t)k2 * (stride + 1) * sizeof(int32_t);
  hipLaunchKernelGGL(rerank_expand_kernel, dim3((unsigned)n), dim3(64), lds, (hipStream_t)stream, rank, ld, n, k2, idx,
                     val, cnt, stride, idx2, val2, cnt2, stride2);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

static size_t rr_inv_off_row(int n) { return align_up((size_t)n * sizeof(int32_t), 256); }
static size_t rr_inv_off_val(int n, size_t nnz) { return rr_inv_off_row(n) + align_up(nnz * sizeof(int32_t), 256); }

size_t oibl_rerank_invert_workspace_bytes(int n, size_t nnz) {
  if (n <= 0) return 0;
  return rr_inv_off_val(n, nnz) + align_up((size_t)nnz * sizeof(float), 256);
}

int oibl_rerank_invert(const int32_t* idx, const float* val, const int32_t* cnt, int stride, int n, size_t nnz,
                       int32_t* col_off, int32_t* inv_row, float* inv_val, void* ws, size_t ws_bytes, void* stream) {
  OIBL_REQUIRE(idx && val && cnt && col_off && inv_row && inv_val && ws, "rerank_invert: null pointer");
  OIBL_REQUIRE(n > 0 && stride >= 1 && nnz <= (size_t)0x7fffffff && nnz <= (size_t)n * stride,
               "rerank_invert: bad shape n=%d stride=%d nnz=%zu", n, stride, nnz);
  OIBL_REQUIRE((uintptr_t)ws % 256 == 0, "rerank_invert: workspace must be 256-byte aligned");
  const size_t need = oibl_rerank_invert_workspace_bytes(n, nnz);
  if (ws_bytes < need) {
    set_error("rerank_invert: workspace %zu < required %zu bytes", ws_bytes, need);
    return OIBL_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int32_t* cursor = (int32_t*)ws;
  int32_t* tmp_row = (int32_t*)((char*)ws + rr_inv_off_row(n));
  float* tmp_val = (float*)((char*)ws + rr_inv_off_val(n, nnz));
  OIBL_HIP_CHECK(hipMemsetAsync(cursor, 0, (size_t)n * sizeof(int32_t), st));
  hipLaunchKernelGGL(rerank_colcount_kernel, dim3((unsigned)n), dim3(64), 0, st, idx, cnt, stride, n, cursor);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(rerank_scan_kernel, dim3(1), dim3(1024), 0, st, (const int32_t*)cursor, n, col_off);
  OIBL_LAUNCH_CHECK();
  OIBL_HIP_CHECK(hipMemsetAsync(cursor, 0, (size_t)n * sizeof(int32_t), st));
  hipLaunchKernelGGL(rerank_fill_kernel, dim3((unsigned)n), dim3(64), 0, st, idx, val, cnt, stride,
                     (const int32_t*)col_off, cursor, tmp_row, tmp_val);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(rerank_colsort_kernel, dim3((unsigned)n), dim3(64), 0, st, (const int32_t*)col_off,
                     (const int32_t*)tmp_row, (const float*)tmp_val, inv_row, inv_val);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

static int rr_jaccard_blocks(int Q) { return Q < RR_JACCARD_BLOCKS ? Q : RR_JACCARD_BLOCKS; }

size_t oibl_rerank_jaccard_workspace_bytes(int Q, int G) {
  if (Q <= 0 || G <= 0) return 0;
  return align_up((size_t)rr_jaccard_blocks(Q) * G * sizeof(float), 256);
}

int oibl_rerank_jaccard(const int32_t* idx, const float* val, const int32_t* cnt, int stride, const int32_t* col_off,
                        const int32_t* inv_row, const float* inv_val, const float* rowmax, int Q, int G,
                        float one_minus_lambda, float lambda, float* dist, size_t ldd, void* ws, size_t ws_bytes,
                        void* stream) {
  OIBL_REQUIRE(idx && val && cnt && col_off && inv_row && inv_val && rowmax && dist && ws,
               "rerank_jaccard: null pointer");
  OIBL_REQUIRE(Q > 0 && G > 0 && (long)Q + G <= 0x7fffffffL && stride >= 1 && ldd >= (size_t)G,
               "rerank_jaccard: bad shape Q=%d G=%d stride=%d ldd=%zu", Q, G, stride, ldd);
  OIBL_REQUIRE((uintptr_t)ws % 256 == 0, "rerank_jaccard: workspace must be 256-byte aligned");
  const size_t need = oibl_rerank_jaccard_workspace_bytes(Q, G);
  if (ws_bytes < need) {
    set_error("rerank_jaccard: workspace %zu < required %zu bytes", ws_bytes, need);
    return OIBL_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  OIBL_HIP_CHECK(hipMemsetAsync(ws, 0, need, st));
  hipLaunchKernelGGL(rerank_jaccard_kernel, dim3((unsigned)rr_jaccard_blocks(Q)), dim3(256), 0, st, idx, val, cnt,
                     stride, col_off, inv_row, inv_val, rowmax, Q, G, one_minus_lambda, lambda, dist, ldd, (float*)ws);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

}  // extern "C"
