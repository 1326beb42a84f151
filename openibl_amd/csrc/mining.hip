// Hard-negative mining of the tuple samplers, per anchor row, on the device
// (ibl/utils/data/sampler.py: DistributedRandomTupleSampler.__iter__ and the SFRS sampler on top of it).
//
// The host loop asks three questions of every ranked row: which entries are outside the anchor's exclusion
// zone (the candidates for negatives), where in that candidate list last round's negatives sit, and which
// entries are positives, best-ranked first.  np.isin over the whole row answers each of them once per anchor
// and visit.  Here the row is ranked by the radix sort of oibl_row_argsort and walked ONCE:
//
//   one workgroup (4 waves) per anchor, the row in chunks of 256 ranks, one rank per lane;
//   membership by binary search in the anchor's sorted CSR rows — the exclusion list from LDS while it has at
//   most MINE_LDS_EXCL entries (16 KB), from global memory beyond, the positives from global memory (a few
//   dozen entries: they stay in the vector cache), the cache entries by a scan of the C <= 64 values in LDS;
//   the kept and the positive stream are compacted in rank order: a wave ballot gives the lane's place inside
//   its wave, the four wave counts cross through a double-buffered LDS slot (ONE barrier per chunk) and a
//   running base carries the place across chunks.
//
// Everything written is an integer position or index, or a copied float (pos_jac): no floating-point
// arithmetic, no atomics, the same bits on every run.  Latency / L2 bound (A x G x 4 bytes read once,
// at most as much written); nothing for the matrix cores.
#include "common.h"

namespace oibl {

constexpr int MINE_THREADS = 256;
constexpr int MINE_WAVES = MINE_THREADS / 64;
constexpr int MINE_LDS_EXCL = 4096;     // exclusion entries staged in LDS; longer lists are searched in global memory
constexpr int MINE_MAX_CACHE = 64;      // C
constexpr int MINE_MAX_POS_POOL = 1024; // pos_pool

struct MineParams {
  const int32_t* ranked;   // [A][G] rank order of every row
  const int32_t* csr_row;  // [A] or NULL: the CSR row of anchor a
  const int32_t* pos_off;
  const int32_t* pos_val;
  const int32_t* excl_off;
  const int32_t* excl_val;
  const int32_t* cache;    // [A][C] or NULL
  const float* jac;        // [A][jac_ld] or NULL
  size_t jac_ld;
  int G, C, pos_pool;
  int32_t* cand;           // [A][cand_ld]
  size_t cand_ld;
  int32_t* cand_len;       // [A]
  int32_t* cache_pos;      // [A][C]
  int32_t* pos_ranked;     // [A][pos_pool]
  float* pos_jac;          // [A][pos_pool]
};

// is g an element of the ascending list v[0..n)?
template <typename P>
__device__ __forceinline__ bool sorted_has(P v, int n, int g) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] < g) lo = mid + 1; else hi = mid;
  }
  return lo < n && v[lo] == g;
}

template <bool EXCL_IN_LDS>
__device__ __forceinline__ void mine_row(const MineParams& p, int a, int32_t* s_excl, int32_t* s_cache,
                                         int32_t* s_cpos, int (*s_cnt)[MINE_WAVES][2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = p.csr_row ? p.csr_row[a] : a;
  const int e0 = p.excl_off[row], ne = p.excl_off[row + 1] - e0;
  const int p0 = p.pos_off[row], np = p.pos_off[row + 1] - p0;
  const int32_t* excl = p.excl_val + e0;
  const int32_t* pos = p.pos_val + p0;
  const int32_t* ranked = p.ranked + (size_t)a * p.G;
  int32_t* cand = p.cand + (size_t)a * p.cand_ld;
  int32_t* pos_ranked = p.pos_ranked + (size_t)a * p.pos_pool;
  float* pos_jac = p.jac ? p.pos_jac + (size_t)a * p.pos_pool : nullptr;
  const float* jac = p.jac ? p.jac + (size_t)a * p.jac_ld : nullptr;

  if (EXCL_IN_LDS)
    for (int i = tid; i < ne; i += MINE_THREADS) s_excl[i] = excl[i];
  if (tid < p.C) {
    s_cache[tid] = p.cache[(size_t)a * p.C + tid];
    s_cpos[tid] = -1;
  }
  __syncthreads();

  int kept_base = 0, pos_base = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int c0 = 0, par = 0; c0 < p.G; c0 += MINE_THREADS, par ^= 1) {
    const int i = c0 + tid;
    const bool valid = i < p.G;
    const int g = valid ? ranked[i] : -1;
    bool keep = valid, is_pos = false;
    if (valid) {
      keep = EXCL_IN_LDS ? !sorted_has(s_excl, ne, g) : !sorted_has(excl, ne, g);
      is_pos = sorted_has(pos, np, g);
    }
    const unsigned long long mk = __ballot(keep), mp = __ballot(is_pos);
    if (lane == 0) {
      s_cnt[par][wave][0] = __popcll(mk);
      s_cnt[par][wave][1] = __popcll(mp);
    }
    __syncthreads();
    // (the slot of the other parity is written next: a wave still reading this one cannot be overtaken
    // by two barriers)
    int before_k = 0, before_p = 0, all_k = 0, all_p = 0;
#pragma unroll
    for (int w = 0; w < MINE_WAVES; ++w) {
      const int ck = s_cnt[par][w][0], cp = s_cnt[par][w][1];
      if (w < wave) {
        before_k += ck;
        before_p += cp;
      }
      all_k += ck;
      all_p += cp;
    }
    if (keep) {
      const int at = kept_base + before_k + __popcll(mk & below);
      cand[at] = g;
      for (int c = 0; c < p.C; ++c)
        if (s_cache[c] == g) s_cpos[c] = at;    // g occurs once in the row: one writer per slot
    }
    if (is_pos) {
      const int at = pos_base + before_p + __popcll(mp & below);
      if (at < p.pos_pool) {
        pos_ranked[at] = g;
        if (jac) pos_jac[at] = jac[g];
      }
    }
    kept_base += all_k;
    pos_base += all_p;
  }
  __syncthreads();
  for (size_t i = (size_t)kept_base + tid; i < p.cand_ld; i += MINE_THREADS) cand[i] = -1;
  for (int j = pos_base + tid; j < p.pos_pool; j += MINE_THREADS) {
    pos_ranked[j] = -1;
    if (jac) pos_jac[j] = __int_as_float(0x7fc00000);
  }
  if (tid < p.C) p.cache_pos[(size_t)a * p.C + tid] = s_cpos[tid];
  if (tid == 0) p.cand_len[a] = kept_base;
}

__global__ __launch_bounds__(MINE_THREADS) void mine_rows_kernel(MineParams p) {
  __shared__ int32_t s_excl[MINE_LDS_EXCL];
  __shared__ int32_t s_cache[MINE_MAX_CACHE];
  __shared__ int32_t s_cpos[MINE_MAX_CACHE];
  __shared__ int s_cnt[2][MINE_WAVES][2];
  const int a = blockIdx.x;
  const int row = p.csr_row ? p.csr_row[a] : a;
  const int ne = p.excl_off[row + 1] - p.excl_off[row];   // uniform: one branch per workgroup
  if (ne <= MINE_LDS_EXCL)
    mine_row<true>(p, a, s_excl, s_cache, s_cpos, s_cnt);
  else
    mine_row<false>(p, a, s_excl, s_cache, s_cpos, s_cnt);
}

}  // namespace oibl

using namespace oibl;

extern "C" {

size_t oibl_mine_rows_workspace_bytes(int A, int G) {
  if (A <= 0 || G <= 0) return 0;
  return align_up((size_t)A * G * 4, 256) + oibl_row_argsort_workspace_bytes(A, G);
}

int oibl_mine_rows(const float* dist, int A, int G, size_t ld, const int32_t* csr_row, const int32_t* pos_off,
                   const int32_t* pos_val, const int32_t* excl_off, const int32_t* excl_val, const int32_t* cache,
                   int C, const float* jac, size_t jac_ld, int pos_pool, int32_t* cand, size_t cand_ld,
                   int32_t* cand_len, int32_t* cache_pos, int32_t* pos_ranked, float* pos_jac, void* ws,
                   size_t ws_bytes, void* stream) {
  OIBL_REQUIRE(dist && pos_off && pos_val && excl_off && excl_val && cand && cand_len && pos_ranked && ws,
               "mine_rows: null pointer");
  OIBL_REQUIRE(A > 0 && G > 0 && ld >= (size_t)G, "mine_rows: bad shape A=%d G=%d ld=%zu", A, G, ld);
  OIBL_REQUIRE(cand_ld >= (size_t)G, "mine_rows: cand_ld=%zu < G=%d", cand_ld, G);
  OIBL_REQUIRE(C >= 0 && C <= MINE_MAX_CACHE, "mine_rows: C=%d outside [0, %d]", C, MINE_MAX_CACHE);
  OIBL_REQUIRE(C == 0 || (cache && cache_pos), "mine_rows: cache and cache_pos are required when C > 0");
  OIBL_REQUIRE(pos_pool >= 1 && pos_pool <= MINE_MAX_POS_POOL, "mine_rows: pos_pool=%d outside [1, %d]", pos_pool,
               MINE_MAX_POS_POOL);
  OIBL_REQUIRE(!jac || (pos_jac && jac_ld >= (size_t)G), "mine_rows: jac needs pos_jac and jac_ld=%zu >= G=%d",
               jac_ld, G);
  OIBL_REQUIRE((uintptr_t)ws % 256 == 0, "mine_rows: workspace must be 256-byte aligned");
  const size_t need = oibl_mine_rows_workspace_bytes(A, G);
  if (ws_bytes < need) {
    set_error("mine_rows: workspace %zu < required %zu bytes", ws_bytes, need);
    return OIBL_E_WORKSPACE;
  }
  const size_t part = align_up((size_t)A * G * 4, 256);
  int32_t* ranked = (int32_t*)ws;
  int rc = oibl_row_argsort(dist, A, G, ld, ranked, nullptr, (char*)ws + part, ws_bytes - part, stream);
  if (rc) return rc;
  MineParams p;
  p.ranked = ranked;
  p.csr_row = csr_row;
  p.pos_off = pos_off;
  p.pos_val = pos_val;
  p.excl_off = excl_off;
  p.excl_val = excl_val;
  p.cache = cache;
  p.jac = jac;
  p.jac_ld = jac_ld;
  p.G = G;
  p.C = C;
  p.pos_pool = pos_pool;
  p.cand = cand;
  p.cand_ld = cand_ld;
  p.cand_len = cand_len;
  p.cache_pos = cache_pos;
  p.pos_ranked = pos_ranked;
  p.pos_jac = pos_jac;
  hipLaunchKernelGGL(mine_rows_kernel, dim3((unsigned)A), dim3(MINE_THREADS), 0, (hipStream_t)stream, p);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

}  // extern "C"
