// One 256 x 256 squared-distance tile on the ring schedule (ring_core.h): the body of pairwise_ring_kernel (bf16,
// bf16x3 and f16mx rows, below) and of pairwise_f16r_kernel (fp16 rows, match_f16r.h).  A = queries, B = gallery,
// K = d.  Same K order and the same epilogue expression as pairwise_kernel (match.hip) -> identical matrices.
// Tile order: the hardware deals block b to XCD b % 8; every XCD gets a contiguous range of tile
// ids, and ids walk groups of 8 query tiles x all gallery tiles with the query tile fastest, so the
// 32 workgroups resident on an XCD form an 8 x 4 block of tiles that shares 8 query panels and 4
// gallery panels through that XCD's L2 (12 panel streams for 32 tiles instead of 33-64).
//   FILTER = false: write dist[m][ldd].
//   FILTER = true : fused top-k front end.  thr[row] is an upper bound of the row's k-th smallest
//     distance (k-th smallest over a strided sample of the gallery, computed with this same kernel,
//     so the sample's own distances reappear bit for bit); every distance the policy keeps against
//     thr[row] is appended to the row's candidate list (value, global index).  The matrix is never
//     written: for 8192 x 81920 the candidates are ~1 % of its 2.7 GB.  Lists that outgrow `cap` are
//     counted, not stored (the caller sees cnt > cap and falls back to the exact path).
// A policy (PairRingPolicy below, F16rPolicy in match_f16r.h) supplies what the two kernels do not share:
//   P, ES          operand code of ring_mainloop and bytes per operand element
//   LIST_OFF       LDS byte offset of the survivor lists: behind everything the policy stages
//   stage_row      thread t < 256 holds row r (clamped) of the tile: stages the policy's own per-row scalars and
//                  returns the row's widened threshold (FILTER; the body stores it in th_s)
//   stage_col      the same for column c; `once` is true in exactly one tile per column of the launch (the
//                  policy's atomicMax bookkeeping over the launch's columns)
//   col            the per-column values of one accumulator column tile, read once per j
//   dist, keep     the distance of an accumulator element and the FILTER predicate
// The policy's callbacks get the LDS base and a row / column of the tile, nothing they would have to derive again.
// The parameters come BY VALUE: the body is optimised before it is inlined into a kernel, and behind a reference
// every store of the filter block might have written them (the list addresses were then formed again at each of
// the 128 elements: several hundred instructions more in the FILTER kernels).
#pragma once

#include "ring_core.h"

namespace oibl {

// what both kernels are launched with
struct RingDistParams {
  const void* x;  // [m][d] operand rows
  const void* y;  // [n rows at y_row_bytes][d]
  const float* xn;
  const float* yn;  // yn[col * y_stride] (and every other per-column array of a policy)
  float* dist;      // !FILTER: [m][ldd]
  size_t ldd;
  unsigned x_bytes, y_bytes;
  long y_row_bytes;
  int y_stride;
  int m, n, d, tiles_m, tiles_n;
  const float* thr;  // FILTER: thr[row * thr_stride]
  int thr_stride;
  float* cand_val;
  int32_t* cand_idx;
  int* cand_cnt;
  int cap, index_base;  // global index of column c = index_base + c
  int group_m;          // query tiles per ordering group (see above)
  // 2-way split-K (threshold sample only, gridDim.y = 2): block (., h) contracts K-half h and writes
  // dist + h * part_stride; the norms enter half 0 only, so the two halves ADD UP to the distances
  // (in another summation order than the one-pass kernel: see thr_slack).
  size_t part_stride;
};

// LDS behind the main loop, in floats from the base: norms of the tile's rows / columns and the rows' thresholds
constexpr int RING_XN_S = 0, RING_YN_S = 256, RING_TH_S = 512;

template <bool FILTER, typename Pol>
__device__ __forceinline__ void ring_dist_tile(const typename Pol::Params p) {
  using G = RingGeo<2>;
  constexpr int P = Pol::P;
  constexpr int KSHIFT = Pol::ES == 4 ? 5 : 6;  // 4-byte operand elements: 32 K per K-tile (bf16x3 and f16mx)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / G::WN, wn = wave % G::WN;
  const unsigned id = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned gm = (unsigned)p.group_m;
  const unsigned width = gm * (unsigned)p.tiles_n;
  const unsigned grp = id / width, in_grp = id - grp * width;
  const unsigned first_m = grp * gm;
  const unsigned gsz = (unsigned)p.tiles_m - first_m < gm ? (unsigned)p.tiles_m - first_m : gm;
  const int tm = (int)(first_m + in_grp % gsz), tn = (int)(in_grp / gsz);
  const int m0 = tm * G::BM, n0 = tn * G::BN;

  const int piece = ring_piece(wave, lane);
  int rows_a[4], rows_b[4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      rows_a[2 * h + i] = ring_a_row<2>(wave, lane, h, i);
      rows_b[2 * h + i] = ring_b_row<2>(wave, lane, h, i);
    }
  // split-K: this block's K-half starts kh * d/2 elements into every row
  const int ksplit = (int)gridDim.y, kh = (int)blockIdx.y;
  const int d_part = p.d / ksplit;
  const unsigned koff = (unsigned)kh * (unsigned)d_part * (unsigned)Pol::ES;
  RingRowLoader<2> la, lb;
  la.init(static_cast<const char*>(p.x) + koff, p.x_bytes - koff, m0, p.m, (long)p.d * Pol::ES, rows_a, piece);
  lb.init(static_cast<const char*>(p.y) + koff, p.y_bytes - koff, n0, p.n, p.y_row_bytes, rows_b,
          P >= RING_MX ? ring_piece_mxb(wave, lane) : piece);

  f32x16_t acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // one copy of the loop per stagger group (ring_core.h)
  if ((wave >> 2) == 0) ring_mainloop<2, false, false, P, 0>(acc, smem, wave, lane, la, lb, d_part >> KSHIFT);
  else ring_mainloop<2, false, false, P, 1>(acc, smem, wave, lane, la, lb, d_part >> KSHIFT);

  // norms (and thresholds, and what the policy adds) of the tile's rows / columns -> LDS; out-of-range
  // rows/columns are clamped here and masked at the store
  float* const s = reinterpret_cast<float*>(smem);
  if (threadIdx.x < 256) {
    const unsigned t = threadIdx.x;
    int r = m0 + (int)t;
    if (r > p.m - 1) r = p.m - 1;
    const float xn = p.xn[r];
    s[RING_XN_S + t] = kh == 0 ? xn : 0.f;
    float th = 0.f;
    if (FILTER) th = p.thr[(long)r * p.thr_stride];
    th = Pol::template stage_row<FILTER>(p, s, t, r, xn, th);
    if (FILTER) s[RING_TH_S + t] = th;
  } else {
    const unsigned t = threadIdx.x - 256;
    int c = n0 + (int)t;
    if (c > p.n - 1) c = p.n - 1;
    const long ci = (long)c * p.y_stride;
    const float yn = p.yn[ci];
    s[RING_YN_S + t] = kh == 0 ? yn : 0.f;
    // (kh == 0 && tm == 0: one column of tiles covers every column of the launch once)
    Pol::template stage_col<FILTER>(p, s, t, ci, yn, kh == 0 && tm == 0, lane);
  }
  __syncthreads();
  // lane geometry: column col0 + 32 j, rows row0 + 32 i + (r & 3) + 8 (r >> 2)
  const int col0 = wn * 64 + (lane & 31), row0 = wm * 128 + 4 * (lane >> 5);
  if constexpr (!FILTER) {
    // stores go through buffer descriptors based at the first element of each 32-row accumulator tile of
    // the wave: one 32-bit lane offset, everything else is scalar (offsets inside a tile stay below
    // 31 * ldd * 4 bytes: the host guarantees ldd <= 2^24)
    const float* const dbase = p.dist + (size_t)kh * p.part_stride + ((size_t)m0 + wm * 128) * p.ldd + n0;
    const unsigned ldd4 = (unsigned)p.ldd * 4u;
    const unsigned voff = (unsigned)(4 * (lane >> 5)) * ldd4 + (unsigned)col0 * 4u;
    const int rows_left = p.m - m0 - row0;  // row r of this lane is valid iff its offset < rows_left
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(dbase + (size_t)(32 * i) * p.ldd), 0, 0x7fffffff, 0x00020000);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bool nok = n0 + col0 + 32 * j < p.n;
        const typename Pol::Col cv = Pol::col(s, col0 + 32 * j);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rt = (r & 3) + 8 * (r >> 2), ro = 32 * i + rt;
          const float dv = Pol::dist(acc[i][j][r], s, row0 + ro, cv);
          if (nok && ro < rows_left)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, dv), rs_d, (int)voff,
                                                  (int)((unsigned)rt * ldd4 + 128u * j), 0);
          // keep the scalar row offsets from being computed (and spilled) for all 128 stores at once
          if ((r & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  } else {
    // Survivors are rare (about 1 % of the distances, ~1.3 per lane and tile) but a wave sees one
    // in every second accumulator register, so nothing with a memory round trip may sit in this
    // loop: each lane first collects its own survivors in a private LDS list (count in a
    // register), then all lanes claim their slots with back-to-back atomics — one round trip per
    // tile instead of one per register.  List layout [entry][thread]: conflict-free.
    constexpr int LCAP = 8;
    float* const l_val = reinterpret_cast<float*>(smem + Pol::LIST_OFF);
    int* const l_idx = reinterpret_cast<int*>(smem + Pol::LIST_OFF + LCAP * 512 * 4);
    int* const l_row = reinterpret_cast<int*>(smem + Pol::LIST_OFF + 2 * LCAP * 512 * 4);
    const int rows_left = p.m - m0 - row0;
    // (the list arguments as values: the stores below do not make the compiler read them again)
    float* const cand_val = p.cand_val;
    int32_t* const cand_idx = p.cand_idx;
    int* const cand_cnt = p.cand_cnt;
    const int cap = p.cap, index_base = p.index_base;
    int nl = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + col0 + 32 * j;
      const bool nok = n < p.n;
      const typename Pol::Col cv = Pol::col(s, col0 + 32 * j);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ro = 32 * i + (r & 3) + 8 * (r >> 2);
          const float dv = Pol::dist(acc[i][j][r], s, row0 + ro, cv);
          // (the predicate in front of the range test, not behind its &&: one branch per element instead of two —
          //  two cost pairwise_f16r_kernel 1.3 %)
          const bool kp = Pol::keep(dv, s, row0 + ro, cv);
          if (nok && ro < rows_left && kp) {
            const int m = m0 + row0 + ro;
            if (nl < LCAP) {
              l_val[nl * 512 + threadIdx.x] = dv;
              l_idx[nl * 512 + threadIdx.x] = index_base + n;
              l_row[nl * 512 + threadIdx.x] = m;
              ++nl;
            } else {  // list full (practically never): claim the slot right away
              const int pos = atomicAdd(cand_cnt + m, 1);
              if (pos < cap) {
                cand_val[(size_t)m * cap + pos] = dv;
                cand_idx[(size_t)m * cap + pos] = index_base + n;
              }
            }
          }
        }
    }
    int e_row[LCAP], e_pos[LCAP];
#pragma unroll
    for (int e = 0; e < LCAP; ++e) {
      e_row[e] = e < nl ? l_row[e * 512 + threadIdx.x] : 0;
      e_pos[e] = cap;
    }
#pragma unroll
    for (int e = 0; e < LCAP; ++e)
      if (e < nl) e_pos[e] = atomicAdd(cand_cnt + e_row[e], 1);
#pragma unroll
    for (int e = 0; e < LCAP; ++e)
      if (e < nl && e_pos[e] < cap) {
        cand_val[(size_t)e_row[e] * cap + e_pos[e]] = l_val[e * 512 + threadIdx.x];
        cand_idx[(size_t)e_row[e] * cap + e_pos[e]] = l_idx[e * 512 + threadIdx.x];
      }
  }
}

// ---- bf16 / bf16x3 / f16mx rows: dist = (xn + yn) - 2 x.y, kept iff <= the row's threshold --------------------
struct PairRingParams : RingDistParams {
  // !FILTER: optional, max over the launch's columns of yn (bit pattern of a non-negative float,
  // atomicMax).  FILTER: optional, read back — the threshold of row i is widened by
  // thr_slack * (xn[i] + *yn_max) / 2, a bound on what the other summation order can move a distance.
  unsigned* yn_max;
  float thr_slack;
};

template <int P_>
struct PairRingPolicy {
  using Params = PairRingParams;
  static constexpr int P = P_, ES = P_ != RING_BF16 ? 4 : 2, LIST_OFF = 4096;
  struct Col {
    float yn;
  };
  template <bool FILTER>
  __device__ static __forceinline__ float stage_row(const Params& p, float*, unsigned, int, float xn, float th) {
    if (FILTER && p.yn_max) th += p.thr_slack * 0.5f * (xn + __uint_as_float(*p.yn_max));
    return th;
  }
  template <bool FILTER>
  __device__ static __forceinline__ void stage_col(const Params& p, float*, unsigned, long, float yn, bool once,
                                                   int lane) {
    if (!FILTER && p.yn_max && once) {
      const float mx = wave_max(yn);  // (norms are >= 0: their bit patterns order as integers)
      if (lane == 0) atomicMax(p.yn_max, __float_as_uint(mx));
    }
  }
  __device__ static __forceinline__ Col col(const float* s, int c) { return {s[RING_YN_S + c]}; }
  __device__ static __forceinline__ float dist(float acc, const float* s, int row, const Col& c) {
    return fmaf(-2.0f, acc, s[RING_XN_S + row] + c.yn);
  }
  __device__ static __forceinline__ bool keep(float dv, const float* s, int row, const Col&) {
    return dv <= s[RING_TH_S + row];
  }
};

template <bool FILTER, int P = RING_BF16>
__global__ __launch_bounds__(512) void pairwise_ring_kernel(PairRingParams p) {
  ring_dist_tile<FILTER, PairRingPolicy<P>>(p);
}

}  // namespace oibl
