// 3x3 convolutions on gfx950: NHWC activations, implicit GEMM on the shared MFMA core (gemm_core.h) and on
// the ring / halo schedules (conv_ring.h, conv_halo.h, conv_halo4.h), bias + ReLU + 2x2 max-pool fused into
// the epilogue.  The Cin = 3 / Cin = 64 front of the backbone is stem.hip, the VGG16 forward vgg.hip.
// Reference behaviour: ibl/models/vgg.py:40-42 (layer list), :61-70 (forward).
#include "conv_halo.h"
#include "conv_halo4.h"
#include "conv_ring.h"
#include "gemm_core.h"
#include "conv_internal.h"

namespace oibl {

// ---------------------------------------------------------------------------------------------
// weight re-pack: [Cout][Cin][3][3] fp32 -> [tap][Cout][Cin] T
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void pack_conv3x3_kernel(const float* __restrict__ w, T* __restrict__ packed, int cout,
                                    int cin) {
  const size_t total = (size_t)9 * cout * cin;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int ci = (int)(i % cin);
    const size_t t = i / cin;
    const int co = (int)(t % cout);
    const int tap = (int)(t / cout);
    const float v = w[((size_t)co * cin + ci) * 9 + tap];
    if constexpr (std::is_same<T, bf16x3_t>::value)
      x3_store(reinterpret_cast<char*>(packed) + (i - ci) * 4, ci, v);  // row (tap, co): cin x 4 bytes
    else
      Elem<T>::store(packed + i, v);
  }
}

// fp32 rows <-> bf16x3 rows (groups of [32 hi | 32 lo]); C % 32 == 0
__global__ void x3_split_rows_kernel(const float* __restrict__ src, char* __restrict__ dst, size_t n,
                                     int C) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / C, c = i - row * C;
    x3_store(dst + row * C * 4, c, src[i]);
  }
}
__global__ void x3_join_rows_kernel(const char* __restrict__ src, float* __restrict__ dst, size_t n,
                                    int C) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / C, c = i - row * C;
    dst[i] = x3_load(src + row * C * 4, c);
  }
}

// ---- f16mx (common.h) ------------------------------------------------------------------------
// weights: one thread per (tap, cout, 32-channel group) line of the packed tensor [tap][Cout][Cin]
__global__ void pack_conv3x3_mx_kernel(const float* __restrict__ w, char* __restrict__ packed, int cout,
                                       int cin) {
  const int groups = cin >> 5;
  const size_t total = (size_t)9 * cout * groups;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int g = (int)(i % groups);
    const size_t t = i / groups;
    const int co = (int)(t % cout);
    const int tap = (int)(t / cout);
    float v[32];
#pragma unroll
    for (int e = 0; e < 32; ++e) v[e] = w[((size_t)co * cin + g * 32 + e) * 9 + tap];
    uint4 line[8];
    mx_pack_line(v, line);
    uint4* dst = reinterpret_cast<uint4*>(packed + i * 128);
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[k] = line[k];
  }
}
// rows: SRC = 0 fp32 rows [rows][C] -> f16mx lines; SRC = 1 bf16x3 lines -> f16mx lines (may be in
// place: a thread reads its whole line before it writes it).  One thread per line.
template <int SRC>
__global__ void mx_pack_rows_kernel(const char* __restrict__ src, char* __restrict__ dst, size_t lines,
                                    unsigned* range_flag) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < lines;
       i += (size_t)gridDim.x * blockDim.x) {
    float v[32];
    const uint4* sp = reinterpret_cast<const uint4*>(src + i * 128);
    if constexpr (SRC == 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint4 t = sp[k];
        v[4 * k] = __builtin_bit_cast(float, t.x);
        v[4 * k + 1] = __builtin_bit_cast(float, t.y);
        v[4 * k + 2] = __builtin_bit_cast(float, t.z);
        v[4 * k + 3] = __builtin_bit_cast(float, t.w);
      }
    } else {
      uint4 hi[4], lo[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        hi[k] = sp[k];
        lo[k] = sp[4 + k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned h[4] = {hi[k].x, hi[k].y, hi[k].z, hi[k].w}, l[4] = {lo[k].x, lo[k].y, lo[k].z, lo[k].w};
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          v[8 * k + 2 * d] = __builtin_bit_cast(float, h[d] << 16) + __builtin_bit_cast(float, l[d] << 16);
          v[8 * k + 2 * d + 1] = __builtin_bit_cast(float, h[d] & 0xffff0000u) + __builtin_bit_cast(float, l[d] & 0xffff0000u);
        }
      }
    }
    uint4 line[8];
    mx_pack_line(v, line, range_flag);
    uint4* dp = reinterpret_cast<uint4*>(dst + i * 128);
#pragma unroll
    for (int k = 0; k < 8; ++k) dp[k] = line[k];
  }
}
// f16mx lines -> fp32 rows as the kernels see the values: WHICH = 0 hi + q6(lo) (the stored value to
// ~2^-15), 1 hi alone, 2 q6(hi), 3 q6(lo)   (tests)
// (mul: a power of two that undoes the backbone's storage scale, 1 elsewhere)
__global__ void mx_join_rows_kernel(const char* __restrict__ src, float* __restrict__ dst, size_t n, int which,
                                    float mul = 1.f) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    float hi, hi6, lo6;
    mx_line_decode(src + (i >> 5) * 128, (int)(i & 31), hi, hi6, lo6);
    dst[i] = (which == 0 ? hi + lo6 : which == 1 ? hi : which == 2 ? hi6 : lo6) * mul;
  }
}

// ---------------------------------------------------------------------------------------------
// implicit-GEMM 3x3 convolution
//   M = output pixels, N = Cout, K = 9 * Cin ordered (tap, cin).  A K-step is one tap x one
//   128-byte run of input channels of each pixel, fetched straight from the NHWC tensor (or from a
//   zero line when the tap falls outside the image).
//   POOL: pixels are enumerated quad-major (m = 4*quad + 2*dy + dx over the floor(H/2) x floor(W/2)
//   pooled grid), so that the four members of a 2x2 window are 4 consecutive GEMM rows = registers
//   4g..4g+3 of one lane in the 32x32 accumulator layout: the pool is an in-register max and the
//   kernel writes the pooled NHWC tensor directly.
// ---------------------------------------------------------------------------------------------
struct ConvParams {
  const void* in;
  const void* w;
  const float* bias;
  void* out;
  const void* zero;
  int N, H, W, cin, cout;
  long m_total;   // GEMM rows (pixels enumerated, 4 per pooled output when POOL)
  long out_rows;  // rows of the output tensor ( = m_total or m_total / 4)
  int tiles_n;
  int relu;
  int ablate;  // timing experiments only (wrong results): 1 = A loads only at tap 0, 2 = B loads
               // only at the first step, 3 = both
  int out_f32;  // bf16x3 only: the output is written as plain fp32 NHWC (the layer feeding the head)
  int korder;   // K order of the implicit GEMM (test hook, see ConvRingALoader::begin_tile)
  // split-K (layers with too few tiles to fill the chip, e.g. conv5 of a single image: 40 tiles):
  // gridDim.y = ksplit workgroups share a tile, each contracts steps/ksplit K-steps from zero and
  // dumps its fp32 accumulators to partial[ks][m_total][cout]; conv_splitk_reduce_kernel adds them in
  // a fixed order, then bias / ReLU / pool / store.
  int ksplit;
  float* partial;
  unsigned* range_flag;  // f16mx: the pass's range flag (common.h, mx_raise_range_flag); may be null
  float bias_mul = 1.f, out_mul = 1.f;   // f16mx backbone: activation scale (g_mx_act_shift; conv_ring.h, RingParams)
};

// one output element into the staged tile row (row-major [BN] of T; bf16x3: (hi, lo) groups or fp32)
template <typename T>
__device__ static inline void conv_stage_store(char* row, int col, float v, int out_f32) {
  if constexpr (std::is_same<T, bf16x3_t>::value) {
    if (out_f32)
      reinterpret_cast<float*>(row)[col] = v;
    else
      x3_store(row, col, v);
  } else {
    Elem<T>::store(reinterpret_cast<T*>(row) + col, v);
  }
}

template <typename Cfg, bool POOL>
struct ConvALoader {
  const char* base[Cfg::A_LOADS];
  unsigned mask[Cfg::A_LOADS];
  const char* zero;
  long tap_off;
  int tap, cc, cchunks, W, ablate, korder;
  long pix_bytes;

  // step0: first K-step of this workgroup (split-K), in the loop's own order
  __device__ inline void init(const WaveCoord& c, const ConvParams& p, long m0, int step0) {
    using T = typename Cfg::T;
    const int piece = load_piece_bytes<Cfg>(c);
    pix_bytes = (long)p.cin * sizeof(T);
    W = p.W;
    ablate = p.ablate;
    korder = p.korder;
    cchunks = p.cin / Cfg::BK;
    zero = reinterpret_cast<const char*>(p.zero) + (c.lane & 7) * 16;
    const int Hq = POOL ? (p.H >> 1) : p.H, Wq = POOL ? (p.W >> 1) : p.W;
#pragma unroll
    for (int j = 0; j < Cfg::A_LOADS; ++j) {
      // 32-bit index math (the host checks m_total < 2^31): 64-bit divides cost hundreds of cycles
      const unsigned m = (unsigned)m0 + (unsigned)load_row<Cfg>(c, j);
      unsigned mk = 0;
      long off = 0;
      if (m < (unsigned)p.m_total) {
        const unsigned q = POOL ? (m >> 2) : m;
        const unsigned sub = POOL ? (m & 3u) : 0u;
        const unsigned hw = (unsigned)Hq * (unsigned)Wq;
        const unsigned n = q / hw;
        const unsigned rem = q - n * hw;
        unsigned yq = rem / (unsigned)Wq;
        int y = (int)yq, x = (int)(rem - yq * (unsigned)Wq);
        if (POOL) {
          y = 2 * y + (int)(sub >> 1);
          x = 2 * x + (int)(sub & 1);
        }
        const bool y0 = y > 0, y2 = y + 1 < p.H, x0 = x > 0, x2 = x + 1 < p.W;
        mk = (y0 && x0 ? 1u : 0u) | (y0 ? 2u : 0u) | (y0 && x2 ? 4u : 0u) | (x0 ? 8u : 0u) | 16u |
             (x2 ? 32u : 0u) | (y2 && x0 ? 64u : 0u) | (y2 ? 128u : 0u) | (y2 && x2 ? 256u : 0u);
        off = (((long)n * p.H + y) * p.W + x) * pix_bytes;
      }
      mask[j] = mk;
      base[j] = reinterpret_cast<const char*>(p.in) + off + piece;
    }
    tap = korder ? step0 % 9 : step0 / cchunks;
    cc = korder ? step0 / 9 : step0 % cchunks;
    tap_off = (long)((tap / 3 - 1) * W + (tap % 3 - 1)) * pix_bytes;
  }
  __device__ inline const char* src(int j) const {
    return ((mask[j] >> tap) & 1u) ? base[j] + tap_off + cc * 128 : zero;
  }
  __device__ inline bool active() const { return !((ablate & 1) && tap != 0); }
  // K order as in ConvRingALoader::begin_tile: 0 = (tap, chunk), 1 = (chunk, tap; test hook)
  __device__ inline void next() {
    if (korder == 0) {
      if (++cc == cchunks) {
        cc = 0;
        ++tap;
        tap_off = (long)((tap / 3 - 1) * W + (tap % 3 - 1)) * pix_bytes;
      }
    } else {
      if (++tap == 9) {
        tap = 0;
        ++cc;
      }
      tap_off = (long)((tap / 3 - 1) * W + (tap % 3 - 1)) * pix_bytes;
    }
  }
};

template <typename Cfg>
struct ConvBLoader {
  const char* p0[Cfg::B_LOADS];  // row pointers at (tap 0, channel chunk 0)
  long tap_stride, off;
  int tap, cc, cchunks, ablate, step, korder;
  __device__ inline bool active() const { return !((ablate & 2) && step != 0); }
  __device__ inline void init(const WaveCoord& c, const ConvParams& prm, long n0, int step0) {
    using T = typename Cfg::T;
    const int piece = load_piece_bytes<Cfg>(c);
    cchunks = prm.cin / Cfg::BK;
    ablate = prm.ablate;
    korder = prm.korder;
    tap = korder ? step0 % 9 : step0 / cchunks;
    cc = korder ? step0 / 9 : step0 % cchunks;
    step = 0;
    tap_stride = (long)prm.cin * sizeof(T) * prm.cout;
    off = tap * tap_stride + cc * 128;
#pragma unroll
    for (int j = 0; j < Cfg::B_LOADS; ++j) {
      const long n = n0 + load_row<Cfg>(c, j);
      p0[j] = reinterpret_cast<const char*>(prm.w) + n * prm.cin * (long)sizeof(T) + piece;
    }
  }
  __device__ inline const char* src(int j) const { return p0[j] + off; }
  __device__ inline void next() {
    ++step;
    if (korder == 0) {
      if (++cc == cchunks) {
        cc = 0;
        ++tap;
      }
    } else if (++tap == 9) {
      tap = 0;
      ++cc;
    }
    off = tap * tap_stride + cc * 128;
  }
};

template <typename Cfg, bool POOL>
constexpr int conv_lds_bytes() {
  constexpr int rows = POOL ? Cfg::BM / 4 : Cfg::BM;
  constexpr int epi = rows * (Cfg::BN * (int)sizeof(typename Cfg::T) + 16);
  return epi > Cfg::MAIN_LDS_BYTES ? epi : Cfg::MAIN_LDS_BYTES;
}

template <typename Cfg, bool POOL, bool GLDS, bool SPLITK = false>
__global__ __launch_bounds__(Cfg::NTHREADS) void conv3x3_igemm_kernel(ConvParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using T = typename Cfg::T;
  constexpr int TM = Cfg::TM, TN = Cfg::TN;
  const WaveCoord c = wave_coord<Cfg>();
  const unsigned tile = xcd_remap(blockIdx.x, gridDim.x);
  const int tn = tile % p.tiles_n, tm = tile / p.tiles_n;
  const long m0 = (long)tm * Cfg::BM, n0 = (long)tn * Cfg::BN;
  const int steps_all = 9 * (p.cin / Cfg::BK);
  const int nsteps = SPLITK ? steps_all / p.ksplit : steps_all;
  const int step0 = SPLITK ? (int)blockIdx.y * nsteps : 0;

  ConvALoader<Cfg, POOL> la;
  ConvBLoader<Cfg> lb;
  la.init(c, p, m0, step0);
  lb.init(c, p, n0, step0);

  // accumulators start at the bias (every kernel of this file orders the sum that way, so that
  // all variants of a layer produce identical bits); split-K parts start at zero, the bias is the
  // first term of the reduction
  f32x16_t acc[TM][TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    float b = SPLITK ? 0.f : p.bias[n0 + (c.wn * TN + j) * 32 + (c.lane & 31)];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        asm volatile("" : "+v"(b));  // distinct registers, not aliases of one value
        acc[i][j][r] = b;
      }
  }

  gemm_nt_mainloop<Cfg, GLDS>(acc, smem, c, la, lb, nsteps);
  // (the main loop ends on a workgroup barrier: the staging LDS is free for the epilogue)

  if constexpr (SPLITK) {
    float* part = p.partial + (size_t)blockIdx.y * (size_t)p.m_total * p.cout;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const long n = n0 + (c.wn * TN + j) * 32 + (c.lane & 31);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const long m = m0 + (c.wm * TM + i) * 32 + acc_row(r, c.lane);
          if (m < p.m_total) part[m * p.cout + n] = acc[i][j][r];
        }
    }
    return;
  }

  constexpr int PITCH = Cfg::BN * (int)sizeof(T) + 16;
  constexpr int OUT_ROWS = POOL ? Cfg::BM / 4 : Cfg::BM;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = (c.wn * TN + j) * 32 + (c.lane & 31);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      if constexpr (POOL) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float v = fmaxf(fmaxf(acc[i][j][4 * g], acc[i][j][4 * g + 1]),
                          fmaxf(acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]));
          if (p.relu) v = fmaxf(v, 0.f);
          const int row = (c.wm * TM + i) * 8 + 2 * g + (c.lane >> 5);
          conv_stage_store<T>(smem + row * PITCH, col, v, p.out_f32);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = acc[i][j][r];
          if (p.relu) v = fmaxf(v, 0.f);
          const int row = (c.wm * TM + i) * 32 + acc_row(r, c.lane);
          conv_stage_store<T>(smem + row * PITCH, col, v, p.out_f32);
        }
      }
    }
  }
  __syncthreads();
  // coalesced copy-out: every output row is BN * sizeof(T) contiguous bytes of the NHWC tensor
  constexpr int CPR = Cfg::BN * (int)sizeof(T) / 16;  // 16-byte chunks per row
  const long row0 = POOL ? (m0 >> 2) : m0;
  char* obase = reinterpret_cast<char*>(p.out) + n0 * (long)sizeof(T);
  const long orow_bytes = (long)p.cout * sizeof(T);
  for (int idx = threadIdx.x; idx < OUT_ROWS * CPR; idx += Cfg::NTHREADS) {
    const int row = idx / CPR, ch = idx - row * CPR;
    const long grow = row0 + row;
    if (grow < p.out_rows)
      *reinterpret_cast<uint4*>(obase + grow * orow_bytes + ch * 16) =
          *reinterpret_cast<const uint4*>(smem + row * PITCH + ch * 16);
  }
}

// out[row][ch] = act(bias[ch] + sum_ks partial[ks][m][ch])  (POOL: max over the 4 GEMM rows of a quad
// first) — the bias leads the sum like in the one-pass kernels, parts are added in ks order.
template <typename T, bool POOL>
__global__ void conv_splitk_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ bias,
                                          char* __restrict__ out, long out_rows, long m_total, int cout,
                                          int ksplit, int relu, int out_f32) {
  const long total = out_rows * cout;
  const size_t part = (size_t)m_total * cout;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / cout;
    const int ch = (int)(i - row * cout);
    float v = -INFINITY;
#pragma unroll
    for (int q = 0; q < (POOL ? 4 : 1); ++q) {
      const size_t m = POOL ? (size_t)row * 4 + q : (size_t)row;
      float a = bias[ch];
      for (int ks = 0; ks < ksplit; ++ks) a += partial[ks * part + m * cout + ch];
      v = fmaxf(v, a);
    }
    if (relu) v = fmaxf(v, 0.f);
    conv_stage_store<T>(out + (size_t)row * cout * sizeof(T), ch, v, out_f32);
  }
}

// split factor for a layer whose tiling leaves most CUs idle (0 = none); shared by the launch and
// by the workspace query.  128-row tiles; parts of >= 6 K-steps; up to 512 workgroups.
static int conv_splitk_factor(long m_total, int cout, int steps) {
  const long tiles = ((m_total + 127) / 128) * (cout / (cout % 128 == 0 ? 128 : 64));
  if (tiles > 192 || steps < 12) return 0;
  const int cands[] = {8, 6, 4, 3, 2};
  for (int s : cands)
    if (steps % s == 0 && steps / s >= 6 && tiles * s <= 512) return s;
  return 0;
}

template <typename Cfg, bool POOL, bool GLDS>
static int launch_conv_kernel(const ConvParams& q, long grid, hipStream_t st) {
  constexpr int lds = conv_lds_bytes<Cfg, POOL>();
  auto kern = conv3x3_igemm_kernel<Cfg, POOL, GLDS>;
  if (lds > 64 * 1024) OIBL_SET_MAX_LDS(kern, lds);  // opt in to more than 64 KiB of dynamic LDS
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(Cfg::NTHREADS), lds, st, q);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

template <typename Cfg, bool POOL>
static int launch_conv_cfg(const ConvParams& p, hipStream_t st) {
  ConvParams q = p;
  q.tiles_n = p.cout / Cfg::BN;
  const long tiles_m = (p.m_total + Cfg::BM - 1) / Cfg::BM;
  const long grid = tiles_m * q.tiles_n;
  if (grid <= 0 || grid > 0x7fffffffL) {
    set_error("conv3x3: grid %ld out of range", grid);
    return OIBL_E_INVALID;
  }
  return g_regstage ? launch_conv_kernel<Cfg, POOL, false>(q, grid, st)
                    : launch_conv_kernel<Cfg, POOL, true>(q, grid, st);
}

// split-K launch: the partial pass of Cfg (128-row tiles) + the reduction
template <typename Cfg, bool POOL>
static int launch_conv_splitk(const ConvParams& p, hipStream_t st) {
  using T = typename Cfg::T;
  ConvParams q = p;
  q.tiles_n = p.cout / Cfg::BN;
  const long grid = ((p.m_total + Cfg::BM - 1) / Cfg::BM) * q.tiles_n;
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)grid, (unsigned)p.ksplit), dim3(Cfg::NTHREADS),
                       Cfg::MAIN_LDS_BYTES, st, q);
  };
  if (g_regstage)
    launch(conv3x3_igemm_kernel<Cfg, POOL, false, true>);
  else
    launch(conv3x3_igemm_kernel<Cfg, POOL, true, true>);
  OIBL_LAUNCH_CHECK();
  const long total = p.out_rows * p.cout;
  unsigned blocks = (unsigned)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL((conv_splitk_reduce_kernel<T, POOL>), dim3(blocks), dim3(256), 0, st, p.partial, p.bias,
                     (char*)p.out, p.out_rows, p.m_total, p.cout, p.ksplit, p.relu, p.out_f32);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

OIBL_HOOK(int, g_ring_raster, 0);                     // test hook: xcd_tile() mode of the ring kernels
// K order of the implicit-GEMM convolutions: 0 = (tap, channel chunk), 1 = (channel chunk, tap), -1 = per
// layer (default).  Order 1 cuts the fetched bytes 3-8x and is slower on every layer except
// the one whose re-fetches run at HBM-class bandwidth: bf16x3 conv2_2 (128 -> 128 at 240 x 320: 11.3 GB
// fetched per launch at 6.6 TB/s in order 0; 1.66 -> 1.54 ms in order 1).  The hook forces one order.
OIBL_HOOK(int, g_conv_korder, -1);
static int conv_korder_for(int precision, int cin, int cout) {
  if (g_conv_korder >= 0) return g_conv_korder;
  return (precision == OIBL_BF16X3 || precision == OIBL_F16MX) && cin == 128 && cout == 128 ? 1 : 0;
}
#ifdef OIBL_DEBUG_HOOKS   // hooks that stem.hip / vgg.hip read too (conv_internal.h)
unsigned long long* g_prof_buf = nullptr;  // test hook: phase profile of block 0
int g_conv_tile = 0;                       // test hook: tile selection (launch_conv)
int g_conv_ablate = 0;
#endif
OIBL_HOOK(int, g_ring_ablate, 0);                     // test hook: see RingParams::ablate

// ring-schedule kernel (conv_ring.h): bf16, Cin % 64 == 0; WM = 2: 256 x 256 tile (Cout % 256 == 0),
// WM = 4: 512 x 128 tile (Cout % 128 == 0)
// a launch over a row sub-range and / or a K split of the layer (conv_ring.h, RingParams; f16mx split-K)
struct RingSub {
  int tiles_m;       // M tiles of this launch, starting at GEMM row m_base
  long m_base;
  int parts;         // 0: one pass; else gridDim.y = parts split-K workgroups per tile
  int nsteps_part, outer_step;
  void* out;         // parts: the partial tensor [parts][out_rows][cout] fp32
  long out_rows;
  size_t part_stride;
};
template <int WM, bool POOL, bool ODD, int P = RING_BF16, bool OUTMX = (P >= RING_MX)>
static int launch_conv_ring_impl(const ConvParams& p, hipStream_t st, const RingSub* sub = nullptr) {
  using G = RingGeo<WM>;
  constexpr bool X3 = P != RING_BF16;  // 4-byte elements
  RingParams q;
  q.in = p.in;
  q.w = p.w;
  q.bias = p.bias;
  q.out = p.out;
  q.in_bytes = (unsigned)((size_t)p.N * p.H * p.W * p.cin * (X3 ? 4 : 2));
  q.w_bytes = (unsigned)((size_t)9 * p.cout * p.cin * (X3 ? 4 : 2));
  q.out_f32 = X3 ? p.out_f32 : 0;
  q.N = p.N;
  q.H = p.H;
  q.W = p.W;
  q.cin = p.cin;
  q.cout = p.cout;
  q.m_total = (int)p.m_total;
  q.out_rows = (int)p.out_rows;
  q.tiles_n = p.cout / G::BN;
  q.relu = p.relu;
  q.prof = g_prof_buf;
  q.ablate = g_ring_ablate;
  {
    const unsigned hq = POOL ? p.H >> 1 : p.H, wq = POOL ? p.W >> 1 : p.W;
    ring_magic_u31(hq * wq ? hq * wq : 1u, &q.hw_mul, &q.hw_sh);
    ring_magic_u31(wq ? wq : 1u, &q.w_mul, &q.w_sh);
  }
  long tiles_m = (p.m_total + G::BM - 1) / G::BM;
  q.m_base = 0;
  q.nsteps_part = q.k_outer_step = 0;
  q.part_stride = 0;
  unsigned parts = 1;
  if (sub) {
    tiles_m = sub->tiles_m;
    q.m_base = (int)sub->m_base;
    if (sub->parts) {   // split-K: raw fp32 accumulators into the partial tensor
      parts = (unsigned)sub->parts;
      q.nsteps_part = sub->nsteps_part;
      q.k_outer_step = sub->outer_step;
      q.part_stride = sub->part_stride;
      q.out = sub->out;
      q.out_rows = (int)sub->out_rows;
      q.out_f32 = 1;
      q.relu = 0;
    }
  }
  const long grid = tiles_m * q.tiles_n;
  q.tiles_m = (int)tiles_m;
  q.raster = g_ring_raster;
  q.korder = p.korder;
  q.range_flag = p.range_flag;
  q.bias_mul = p.bias_mul;
  q.out_mul = (sub && sub->parts) ? 1.f : p.out_mul;   // (split-K partials are raw sums: the reduction scales)
  q.stagger = 0;   // (unread: conv_ring.h)
  constexpr int lds = ring_lds_bytes<WM, POOL, P, OUTMX>();
  auto kern = conv3x3_ring_kernel<WM, POOL, ODD, P, OUTMX>;
  OIBL_SET_MAX_LDS(kern, lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid, parts), dim3(512), lds, st, q);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

template <int WM, bool POOL, int P = RING_BF16>
static int launch_conv_ring(const ConvParams& p, hipStream_t st, const RingSub* sub = nullptr) {
  // an odd number of K-tiles happens only for Cin = 64 in bf16 (the 4-byte element types have twice
  // the K-tiles), which only the 512 x 128 variant serves
  if constexpr (WM == 4 && P == RING_BF16) {
    if ((9 * (p.cin / 64)) & 1) return launch_conv_ring_impl<WM, POOL, true>(p, st);
  }
  return launch_conv_ring_impl<WM, POOL, false, P>(p, st, sub);
}

// 0 = not eligible, else the wave-row count of the instantiation to use (es = bytes per element)
static int ring_variant(const ConvParams& p, int es = 2) {
  if (p.cin % 64 != 0 || (size_t)p.N * p.H * p.W * p.cin * es >= (size_t)0xE0000000u ||
      p.m_total >= 0x7fffff00L)
    return 0;
  if (p.cout % 256 == 0 && p.cin % 128 == 0) return 2;
  if (p.cout % 128 == 0) return 4;
  return 0;
}

// Tile selection.  The implicit GEMM is bound by L2 -> LDS traffic before it is bound by the
// matrix cores: a 128 x 128 x 64 step needs 32 KB per 2.1 MFLOP (64 flop/B, i.e. ~64 B/clk/CU at
// the bf16 MFMA peak), a 256 x 256 step half of that.  So the largest tile that still gives every
// CU a couple of workgroups wins; small problems (conv5 at small batch) fall back to 128-row tiles.
// g_conv_tile (test hook): 0 = auto, 1 = 128x{128,64}, 2 = 256x{128,64}, 3 = 256x256 where legal,
// 4 = ring schedule where legal.  Auto prefers the ring kernel whenever its 256x256 tiling gives
// every CU at least one workgroup.
OIBL_HOOK(long, g_ring_min_tiles, 256);

template <typename T>
static int launch_conv(const ConvParams& p, int pool, hipStream_t st) {
  using C128x128 = GemmCfg<T, 2, 2, 2, 2>;
  using C128x64 = GemmCfg<T, 2, 2, 2, 1>;
#define OIBL_CONV_DISPATCH(CFG) \
  return pool ? launch_conv_cfg<CFG, true>(p, st) : launch_conv_cfg<CFG, false>(p, st)
  if (p.ksplit > 1 && p.partial && !p.ablate && g_conv_tile == 0) {
    if (p.cout % 128 == 0)
      return pool ? launch_conv_splitk<C128x128, true>(p, st) : launch_conv_splitk<C128x128, false>(p, st);
    return pool ? launch_conv_splitk<C128x64, true>(p, st) : launch_conv_splitk<C128x64, false>(p, st);
  }
  if constexpr (std::is_same<T, bf16x3_t>::value) {
    // ring kernels as in bf16 (pooled layers never write fp32); generic tiles whose staged output
    // (4 bytes per element) fits next to nothing else in LDS: 256 x {128, 64}, 128 x {128, 64}
    using C256x128 = GemmCfg<T, 4, 2, 2, 2>;
    using C256x64 = GemmCfg<T, 4, 2, 2, 1>;
    using C512x64 = GemmCfg<T, 8, 1, 2, 2>;  // Cout = 64 (conv1_2): 64 x 64 per wave instead of 64 x 32
    using C256x64w4 = GemmCfg<T, 4, 1, 2, 2>;  // the same wave tile with 4 waves: 80 KB, two workgroups per CU
    const int rv = (g_regstage || p.ablate || (pool && p.out_f32)) ? 0 : ring_variant(p, 4);
    const long t256 = (p.m_total + 255) / 256;
    const long ring_tiles = rv == 2 ? t256 * (p.cout / 256) : ((p.m_total + 511) / 512) * (p.cout / 128);
    int mode = g_conv_tile;
    if (rv && (mode == 4 || (mode == 0 && ring_tiles >= g_ring_min_tiles))) {
      if (rv == 2)
        return pool ? launch_conv_ring<2, true, RING_X3>(p, st) : launch_conv_ring<2, false, RING_X3>(p, st);
      return pool ? launch_conv_ring<4, true, RING_X3>(p, st) : launch_conv_ring<4, false, RING_X3>(p, st);
    }
    if (mode == 4) mode = 0;
    // (the 512 x 64 tile — 64 x 64 per wave — is kept behind the hook: 2.73 ms vs 2.48 ms for the
    //  256 x 64 tile on conv1_2 at batch 32)
    if (mode == 0) mode = t256 * (p.cout / (p.cout % 128 == 0 ? 128 : 64)) >= 512 ? 2 : 1;
    if (mode == 3 && p.cout % 128 != 0) { OIBL_CONV_DISPATCH(C512x64); }
    if (mode == 5 && p.cout % 128 != 0) { OIBL_CONV_DISPATCH(C256x64w4); }
    if (mode == 5) mode = 2;
    if (mode >= 2) {
      if (p.cout % 128 == 0) { OIBL_CONV_DISPATCH(C256x128); }
      OIBL_CONV_DISPATCH(C256x64);
    }
  } else if constexpr (sizeof(T) == 2) {
    using C256x256 = GemmCfg<T, 2, 4, 4, 2>;
    using C256x128 = GemmCfg<T, 4, 2, 2, 2>;
    using C256x64 = GemmCfg<T, 4, 2, 2, 1>;
    const long t256 = (p.m_total + 255) / 256;
    int mode = g_conv_tile;
    const int rv = (g_regstage || p.ablate) ? 0 : ring_variant(p);
    const long ring_tiles = rv == 2 ? t256 * (p.cout / 256) : ((p.m_total + 511) / 512) * (p.cout / 128);
    if (rv && (mode == 4 || (mode == 0 && ring_tiles >= g_ring_min_tiles))) {
      if (rv == 2) return pool ? launch_conv_ring<2, true>(p, st) : launch_conv_ring<2, false>(p, st);
      return pool ? launch_conv_ring<4, true>(p, st) : launch_conv_ring<4, false>(p, st);
    }
    if (mode == 4) mode = 0;
    if (mode == 0) {
      if (p.cout % 256 == 0 && t256 * (p.cout / 256) >= 512) mode = 3;
      else if (t256 * (p.cout / (p.cout % 128 == 0 ? 128 : 64)) >= 512) mode = 2;
      else mode = 1;
    }
    if (mode == 3 && p.cout % 256 == 0) { OIBL_CONV_DISPATCH(C256x256); }
    if (mode >= 2) {
      if (p.cout % 128 == 0) { OIBL_CONV_DISPATCH(C256x128); }
      OIBL_CONV_DISPATCH(C256x64);
    }
  }
  if (p.cout % 128 == 0) { OIBL_CONV_DISPATCH(C128x128); }
  OIBL_CONV_DISPATCH(C128x64);
#undef OIBL_CONV_DISPATCH
}

// f16mx: the ring kernels are the only implementation (Cin % 64 == 0, Cout % 128 == 0 — every layer
// of the backbone behind the stem)
// Patch of the halo kernel (conv_halo.h) for an Hn x Wn map: PH, PW even, PH * PW <= 256 pixels,
// (PH + 2) * (PW + 2) <= 344 halo lines; fewest patches first, then the smaller halo.
static void halo_patch(int Hn, int Wn, int* PH, int* PW) {
  long best = -1;
  int bh = 2, bw = 2, bhalo = 0;
  for (int ph = 2; ph <= 128; ph += 2) {
    int pwmax = 256 / ph;
    const int hcap = HALO_MAX_POS / (ph + 2) - 2;
    if (hcap < pwmax) pwmax = hcap;
    pwmax &= ~1;
    if (pwmax < 2) continue;
    const int tx = (Wn + pwmax - 1) / pwmax;
    int pw = ((Wn + tx - 1) / tx + 1) & ~1;  // the narrowest even width that still needs tx patches
    if (pw > pwmax) pw = pwmax;
    const long cost = (long)((Hn + ph - 1) / ph) * tx;
    const int halo = (ph + 2) * (pw + 2);
    if (best < 0 || cost < best || (cost == best && halo < bhalo)) {
      best = cost;
      bh = ph;
      bw = pw;
      bhalo = halo;
    }
  }
  *PH = bh;
  *PW = bw;
}

// what the two halo launchers fill the same way; bn: output channels of the kernel's tile
template <bool POOL>
static int halo_params(const ConvParams& p, int bn, const char* name, HaloParams& q) {
  q = {};
  q.in = p.in;
  q.w = p.w;
  q.bias = p.bias;
  q.out = p.out;
  q.in_bytes = (unsigned)((size_t)p.N * p.H * p.W * p.cin * 4);
  q.w_bytes = (unsigned)((size_t)9 * p.cout * p.cin * 4);
  q.N = p.N;
  q.H = p.H;
  q.W = p.W;
  q.cin = p.cin;
  q.cout = p.cout;
  const int Hn = POOL ? (p.H / 2) * 2 : p.H, Wn = POOL ? (p.W / 2) * 2 : p.W;
  halo_patch(Hn, Wn, &q.PH, &q.PW);
  q.tiles_y = (Hn + q.PH - 1) / q.PH;
  q.tiles_x = (Wn + q.PW - 1) / q.PW;
  const long tiles_m = (long)p.N * q.tiles_y * q.tiles_x;
  q.tiles_n = p.cout / bn;
  OIBL_REQUIRE(tiles_m * q.tiles_n <= 0x7fffffffL, "conv3x3 (%s): grid out of range", name);
  q.tiles_m = (int)tiles_m;
  ring_magic_u31((unsigned)(q.tiles_y * q.tiles_x), &q.img_mul, &q.img_sh);
  ring_magic_u31((unsigned)q.tiles_x, &q.tx_mul, &q.tx_sh);
  ring_magic_u31((unsigned)(POOL ? q.PW / 2 : q.PW), &q.pw_mul, &q.pw_sh);
  ring_magic_u31((unsigned)(q.PW + 2), &q.hp_mul, &q.hp_sh);
  q.relu = p.relu;
  q.out_f32 = p.out_f32;
  q.range_flag = p.range_flag;
  q.bias_mul = p.bias_mul;
  q.out_mul = p.out_mul;
  return OIBL_OK;
}

template <bool POOL>
static int launch_conv_halo(const ConvParams& p, hipStream_t st) {
  HaloParams q;
  if (const int rc = halo_params<POOL>(p, RingGeo<2>::BN, "halo", q)) return rc;
  q.raster = g_ring_raster;
  const dim3 grid((unsigned)(q.tiles_m * q.tiles_n));
  auto kern = conv3x3_halo_kernel<POOL, RING_MX>;
  OIBL_SET_MAX_LDS(kern, HALO_LDS);
  hipLaunchKernelGGL(kern, grid, dim3(512), HALO_LDS, st, q);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

// The 128-output-channel layers (conv2_1, conv2_2): conv_halo4.h — 256 pixels x 128 channels, 4 waves, two
// workgroups per CU.
template <bool POOL>
static int launch_conv_halo4(const ConvParams& p, hipStream_t st) {
  HaloParams q;
  if (const int rc = halo_params<POOL>(p, H4_BN, "halo4", q)) return rc;
  q.raster = g_ring_raster & 255;
  q.prof = g_prof_buf;
  auto kern = conv3x3_halo4_kernel<POOL>;
  OIBL_SET_MAX_LDS(kern, H4_LDS);
  hipLaunchKernelGGL(kern, dim3((unsigned)(q.tiles_m * q.tiles_n)), dim3(H4_THREADS), H4_LDS, st, q);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

// ---- f16mx: row sub-ranges + split-K on the ring kernels ------------------------------------------
// The ring tiles are 256 x 256 / 512 x 128 outputs and a workgroup owns a CU: a layer with T tiles runs
// ceil(T / 256) rounds and the last one may be nearly empty — conv5_x at batch 32: 300 tiles = one full
// round + 44 workgroups for a second; a single 480x640 image: 10 tiles on 256 CUs.  The plan: the FULL
// rounds run as they are; the REMAINDER tiles are contracted by s workgroups each (s = 3 or 9 in K order
// (tap, chunk): a part is 3 taps / one tap of all channel chunks; s = 2 in order (chunk, tap)), every part
// from zero accumulators into an fp32 partial tensor, and conv_mx_splitk_reduce_kernel adds bias + parts in
// a fixed order, applies ReLU (and the 2x2 max-pool), packs the f16mx lines.  Deterministic; the sums are
// those of the one-pass kernel up to fp32 association.  A pooled layer is split only as a whole (its
// remainder is not a contiguous range of the pooling kernel's quad-major rows).
constexpr int MX_CUS = 256;
struct MxSplitPlan {
  int wm;           // wave rows of the ring instantiation (2: 256 x 256 tiles, 4: 512 x 128)
  int tm_main;      // M tiles of the unsplit part (0: none)
  int tm_rem;       // M tiles of the split part (0: the layer runs in one pass)
  int s;            // parts per remainder tile
  int nsteps_part;  // K-tiles per part
  int outer_step;   // outer K indices per part
  long m_base;      // first GEMM row of the split part
  long rows_part;   // GEMM rows of the split part
};
OIBL_HOOK(int, g_mx_splitk, 1);   // test hook: 0 = never split; 2 = split, reduced by conv_mx_splitk_reduce_kernel
OIBL_HOOK(int, g_mx_variant, 0);  // test hook: kernel choice of the f16mx layers (launch_conv_mx): 0, 1 or 3
// the 128-output-channel layers run on conv_halo4.h (256-pixel tiles, two workgroups per CU): no ring rounds to balance
static bool mx_halo4_layer(int cin, int cout) {
  return (g_mx_variant == 0 || g_mx_variant == 3) && cout == 128 && cin % 64 == 0;
}
static MxSplitPlan mx_split_plan(long m_plain, int cin, int cout, int pool, int korder, int wm) {
  MxSplitPlan pl = {};
  pl.wm = wm;
  if (wm == 0 || m_plain <= 0) return pl;   // no ring tiling for this layer (Cout = 64: the stem's conv1_2)
  if (mx_halo4_layer(cin, cout)) {          // one pass, whatever the batch
    pl.tm_main = (int)((m_plain + wm * 128 - 1) / (wm * 128));
    return pl;
  }
  const int bm = wm * 128, tiles_n = cout / (wm == 2 ? 256 : 128);
  const long tm = (m_plain + bm - 1) / bm;
  const long T = tm * tiles_n;
  const int cchunks = cin >> 5, nsteps = 9 * cchunks;
  pl.tm_main = (int)tm;
  if (!g_mx_splitk) return pl;
  // full rounds of whole M-tile columns stay unsplit
  long tm_main = (T / MX_CUS) * MX_CUS / tiles_n;
  if (pool && tm_main != 0) return pl;
  const long r = (tm - tm_main) * tiles_n;
  if (r == 0) return pl;
  // cost in K-tile times: a workgroup pays ~12 K-tiles of prologue + epilogue on top of its contraction
  auto rounds = [](long wgs) { return (wgs + MX_CUS - 1) / MX_CUS; };
  const long base = rounds(r) * (nsteps + 12);
  long best = base;
  int best_s = 1;
  const int cands0[] = {3, 9}, cands1[] = {2, 4};
  for (int ci = 0; ci < 2; ++ci) {
    const int s = korder == 0 ? cands0[ci] : cands1[ci];
    const int outer = korder == 0 ? 9 : cchunks;
    if (outer % s != 0) continue;
    const int part = nsteps / s;
    if (part < 4 || (part & 1)) continue;            // the ring loop wants an even number >= 4 of K-tiles
    const long c = rounds(r * s) * (part + 12) + 4;    // + the reduction pass
    if (c < best) {
      best = c;
      best_s = s;
    }
  }
  // worth it from 10 % of the layer on (two more launches)
  const long whole = (tm_main * tiles_n / MX_CUS) * (nsteps + 12) + base;
  if (best_s == 1 || (base - best) * 10 < whole) return pl;
  pl.tm_main = (int)tm_main;
  pl.tm_rem = (int)(tm - tm_main);
  pl.s = best_s;
  pl.nsteps_part = nsteps / best_s;
  pl.outer_step = (korder == 0 ? 9 : cchunks) / best_s;
  pl.m_base = tm_main * bm;
  pl.rows_part = m_plain - pl.m_base;
  return pl;
}
static int mx_ring_wm(int cin, int cout) {
  if (cin % 64 != 0) return 0;
  if (cout % 256 == 0 && cin % 128 == 0) return 2;
  return cout % 128 == 0 ? 4 : 0;
}
static size_t mx_split_bytes(long m_plain, int cin, int cout, int pool, int korder) {
  const MxSplitPlan pl = mx_split_plan(m_plain, cin, cout, pool, korder, mx_ring_wm(cin, cout));
  return pl.tm_rem ? align_up((size_t)pl.s * pl.rows_part * cout * sizeof(float), 256) : 0;
}

// partial [s][rows_part][cout] fp32 -> out rows (f16mx lines, or fp32 when out_f32): one thread per
// (output row, 32-channel group).  POOL: an output row is a pooled pixel, its four sources are GEMM rows
// (n, 2 yo + dy, 2 xo + dx) in plain pixel order; rows_part then covers the whole layer (m_base = 0).
template <bool POOL>
__global__ void conv_mx_splitk_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ bias,
                                             char* __restrict__ out, long out_row0, long out_rows_here,
                                             long rows_part, int cout, int s, int relu, int out_f32, int H,
                                             int W, unsigned* range_flag, float bias_mul, float out_mul) {
  const int groups = cout >> 5;
  const long items = out_rows_here * groups;
  const size_t part = (size_t)rows_part * cout;
  const int Ho = H >> 1, Wo = W >> 1;
  for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (long)gridDim.x * blockDim.x) {
    const long r = it / groups;
    const int g = (int)(it - r * groups);
    float v[32];
#pragma unroll
    for (int e = 0; e < 32; ++e) v[e] = -INFINITY;
#pragma unroll
    for (int q = 0; q < (POOL ? 4 : 1); ++q) {
      long src = r;
      if constexpr (POOL) {
        const long n = r / ((long)Ho * Wo), rem = r - n * (long)Ho * Wo;
        const int yo = (int)(rem / Wo), xo = (int)(rem - (long)yo * Wo);
        src = (n * H + 2 * yo + (q >> 1)) * W + 2 * xo + (q & 1);
      }
      float a[32];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float4 b = *reinterpret_cast<const float4*>(bias + g * 32 + 4 * k);
        a[4 * k] = b.x * bias_mul;
        a[4 * k + 1] = b.y * bias_mul;
        a[4 * k + 2] = b.z * bias_mul;
        a[4 * k + 3] = b.w * bias_mul;
      }
      for (int ks = 0; ks < s; ++ks) {
        const float4* pp = reinterpret_cast<const float4*>(partial + ks * part + (size_t)src * cout + g * 32);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float4 t = pp[k];
          a[4 * k] += t.x;
          a[4 * k + 1] += t.y;
          a[4 * k + 2] += t.z;
          a[4 * k + 3] += t.w;
        }
      }
#pragma unroll
      for (int e = 0; e < 32; ++e) v[e] = fmaxf(v[e], a[e]);
    }
    if (relu) {
#pragma unroll
      for (int e = 0; e < 32; ++e) v[e] = fmaxf(v[e], 0.f);
    }
#pragma unroll
    for (int e = 0; e < 32; ++e) v[e] *= out_mul;
    char* dst = out + ((size_t)(out_row0 + r) * cout + g * 32) * 4;
    if (out_f32) {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        reinterpret_cast<float4*>(dst)[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    } else {
      uint4 line[8];
      mx_pack_line(v, line, range_flag);
#pragma unroll
      for (int k = 0; k < 8; ++k) reinterpret_cast<uint4*>(dst)[k] = line[k];
    }
  }
}

// The same reduction with EIGHT threads per (output row, 32-channel group), four channels each: the sums are
// formed by 8x as many threads as above with fully coalesced 16-byte loads (a single image's conv5_x has 19200
// lines — 75 workgroups of one-thread-per-line, each thread a chain of 9 x 8 loads: the reduce kernels were 22 %
// of a single image's forward, profiles/r04_j_single_image_kernels.md), then handed over through LDS to one
// thread per line that packs and stores it (fp32 output: stored by the eight threads directly).  Same
// operations in the same order per element as the kernel above: bit-identical (tests/test_gpu_splitk.py).
constexpr int RED_LINES = 32;    // lines per workgroup pass = 256 threads / 8
constexpr int RED_PITCH = 36;    // floats per staged line (16-byte aligned rows; a line's reader meets 4-way conflicts)
template <bool POOL>
__global__ __launch_bounds__(256) void conv_mx_splitk_reduce8_kernel(
    const float* __restrict__ partial, const float* __restrict__ bias, char* __restrict__ out, long out_row0,
    long out_rows_here, long rows_part, int cout, int s, int relu, int out_f32, int H, int W, unsigned* range_flag,
    float bias_mul, float out_mul) {
  __shared__ __attribute__((aligned(16))) float stage[RED_LINES * RED_PITCH];
  const int groups = cout >> 5;
  const long items = out_rows_here * groups;
  const size_t part = (size_t)rows_part * cout;
  const int Ho = H >> 1, Wo = W >> 1;
  const int ln = threadIdx.x >> 3, k = threadIdx.x & 7;
  for (long base = (long)blockIdx.x * RED_LINES; base < items; base += (long)gridDim.x * RED_LINES) {
    const long it = base + ln;
    const bool live = it < items;
    const long r = live ? it / groups : 0;
    const int g = live ? (int)(it - r * groups) : 0;
    float4 v = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (live) {
      float4 b = *reinterpret_cast<const float4*>(bias + g * 32 + 4 * k);
      b = make_float4(b.x * bias_mul, b.y * bias_mul, b.z * bias_mul, b.w * bias_mul);
#pragma unroll
      for (int q = 0; q < (POOL ? 4 : 1); ++q) {
        long src = r;
        if constexpr (POOL) {
          const long n = r / ((long)Ho * Wo), rem = r - n * (long)Ho * Wo;
          const int yo = (int)(rem / Wo), xo = (int)(rem - (long)yo * Wo);
          src = (n * H + 2 * yo + (q >> 1)) * W + 2 * xo + (q & 1);
        }
        float4 a = b;
        const float* pp = partial + (size_t)src * cout + g * 32 + 4 * k;
        for (int ks = 0; ks < s; ++ks) {
          const float4 t = *reinterpret_cast<const float4*>(pp + ks * part);
          a.x += t.x;
          a.y += t.y;
          a.z += t.z;
          a.w += t.w;
        }
        v = make_float4(fmaxf(v.x, a.x), fmaxf(v.y, a.y), fmaxf(v.z, a.z), fmaxf(v.w, a.w));
      }
      if (relu) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
      v = make_float4(v.x * out_mul, v.y * out_mul, v.z * out_mul, v.w * out_mul);
    }
    if (out_f32) {   // (uniform)
      if (live) *reinterpret_cast<float4*>(out + ((size_t)(out_row0 + r) * cout + g * 32 + 4 * k) * 4) = v;
      continue;
    }
    *reinterpret_cast<float4*>(&stage[ln * RED_PITCH + 4 * k]) = v;
    __syncthreads();
    if (threadIdx.x < RED_LINES && base + threadIdx.x < items) {
      const long it2 = base + threadIdx.x;
      const long r2 = it2 / groups;
      const int g2 = (int)(it2 - r2 * groups);
      float w[32];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float4 t = *reinterpret_cast<const float4*>(&stage[threadIdx.x * RED_PITCH + 4 * j]);
        w[4 * j] = t.x;
        w[4 * j + 1] = t.y;
        w[4 * j + 2] = t.z;
        w[4 * j + 3] = t.w;
      }
      uint4 line[8];
      mx_pack_line(w, line, range_flag);
      uint4* dst = reinterpret_cast<uint4*>(out + ((size_t)(out_row0 + r2) * cout + g2 * 32) * 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j] = line[j];
    }
    __syncthreads();
  }
}

// f16mx: ring kernels (Cin % 64 == 0, Cout % 128 == 0 — every layer of the backbone behind the stem).
// g_mx_variant (test hook): 0 = that; 3 = the halo kernel (conv_halo.h) for the 256-channel-tile layers —
// 0.58x the LDS-DMA bytes, +5 % on conv3_x, -5 % on conv4_x / conv5_x since the ring's K cursor left its
// LOAD segments (profiles/r03_*): kept as the tested alternative; 1 = ring kernels only.
static int launch_conv_mx_split(const ConvParams& p, int pool, const MxSplitPlan& pl, hipStream_t st) {
  // 1. the full rounds, unsplit, straight into the output (never pooled: see mx_split_plan)
  int rc;
  if (pl.tm_main) {
    RingSub main = {};
    main.tiles_m = pl.tm_main;
    rc = pl.wm == 2 ? launch_conv_ring<2, false, RING_MX>(p, st, &main)
                    : launch_conv_ring<4, false, RING_MX>(p, st, &main);
    if (rc) return rc;
  }
  // 2. the remainder tiles, s parts each, plain pixel order, raw fp32 accumulators
  ConvParams q = p;
  const long m_plain = (long)p.N * p.H * p.W;
  q.m_total = m_plain;
  q.out_rows = m_plain;
  RingSub rem = {};
  rem.tiles_m = pl.tm_rem;
  rem.m_base = pl.m_base;
  rem.parts = pl.s;
  rem.nsteps_part = pl.nsteps_part;
  rem.outer_step = pl.outer_step;
  rem.out = p.partial;
  rem.out_rows = pl.rows_part;
  rem.part_stride = (size_t)pl.rows_part * p.cout * sizeof(float);
  rc = pl.wm == 2 ? launch_conv_ring<2, false, RING_MX>(q, st, &rem)
                  : launch_conv_ring<4, false, RING_MX>(q, st, &rem);
  if (rc) return rc;
  // 3. bias + parts in order, ReLU, pool, pack
  const long out_row0 = pool ? 0 : pl.m_base;
  const long out_rows_here = pool ? p.out_rows : pl.rows_part;
  const long items = out_rows_here * (p.cout / 32);
  if (g_mx_splitk != 2) {   // (2 = test hook: the one-thread-per-line reduction below)
    unsigned blocks8 = (unsigned)((items + RED_LINES - 1) / RED_LINES);
    if (blocks8 > 16384) blocks8 = 16384;
    if (pool)
      hipLaunchKernelGGL(conv_mx_splitk_reduce8_kernel<true>, dim3(blocks8), dim3(256), 0, st, p.partial, p.bias,
                         (char*)p.out, out_row0, out_rows_here, pl.rows_part, p.cout, pl.s, p.relu, p.out_f32, p.H,
                         p.W, p.range_flag, p.bias_mul, p.out_mul);
    else
      hipLaunchKernelGGL(conv_mx_splitk_reduce8_kernel<false>, dim3(blocks8), dim3(256), 0, st, p.partial, p.bias,
                         (char*)p.out, out_row0, out_rows_here, pl.rows_part, p.cout, pl.s, p.relu, p.out_f32, p.H,
                         p.W, p.range_flag, p.bias_mul, p.out_mul);
    OIBL_LAUNCH_CHECK();
    return OIBL_OK;
  }
  unsigned blocks = (unsigned)((items + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  if (pool)
    hipLaunchKernelGGL(conv_mx_splitk_reduce_kernel<true>, dim3(blocks), dim3(256), 0, st, p.partial, p.bias,
                       (char*)p.out, out_row0, out_rows_here, pl.rows_part, p.cout, pl.s, p.relu, p.out_f32, p.H, p.W,
                       p.range_flag, p.bias_mul, p.out_mul);
  else
    hipLaunchKernelGGL(conv_mx_splitk_reduce_kernel<false>, dim3(blocks), dim3(256), 0, st, p.partial, p.bias,
                       (char*)p.out, out_row0, out_rows_here, pl.rows_part, p.cout, pl.s, p.relu, p.out_f32, p.H, p.W,
                       p.range_flag, p.bias_mul, p.out_mul);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

static int launch_conv_mx(const ConvParams& p, int pool, hipStream_t st) {
  // row sub-ranges + split-K where the tiling leaves a nearly empty round (needs the partial scratch)
  if (p.partial && g_mx_variant <= 1 && !(pool && p.out_f32) && ring_variant(p, 4)) {
    const MxSplitPlan pl = mx_split_plan((long)p.N * p.H * p.W, p.cin, p.cout, pool, p.korder, mx_ring_wm(p.cin, p.cout));
    if (pl.tm_rem) return launch_conv_mx_split(p, pool, pl, st);
  }
  const int rv = (pool && p.out_f32) ? 0 : ring_variant(p, 4);
  // the halo kernel (conv_halo.h) where it is the faster one: the 256-output-channel layers at 120 x 160
  // (conv3_1..conv3_3: 0.57 / 1.00 / 0.95 ms against 0.60 / 1.04 / 0.97 on the ring; deeper layers lose 5-10 %).
  // Hook: 1 = ring kernels only, 3 = halo kernel wherever it applies.
  const bool halo_ok = rv == 2 && ((p.cin >> 5) & 1) == 0;
  if (halo_ok && (g_mx_variant == 3 || (g_mx_variant == 0 && p.cout == 256)))
    return pool ? launch_conv_halo<true>(p, st) : launch_conv_halo<false>(p, st);
  // the 4-wave halo kernel (conv_halo4.h) for the 128-output-channel layers (rv == 4: conv2_1 / conv2_2): a third
  // of the ring's L2 -> LDS bytes per K-tile.  Hook: 1 = ring kernels.  (On every layer it was an experiment: conv3_x
  // ties with the 8-wave halo kernel, conv4_x / conv5_x lose 12-16 %, profiles/r05_*_timing.txt.)
  if (rv == 4 && mx_halo4_layer(p.cin, p.cout))
    return pool ? launch_conv_halo4<true>(p, st) : launch_conv_halo4<false>(p, st);
  if (rv == 2) return pool ? launch_conv_ring<2, true, RING_MX>(p, st) : launch_conv_ring<2, false, RING_MX>(p, st);
  if (rv == 4) return pool ? launch_conv_ring<4, true, RING_MX>(p, st) : launch_conv_ring<4, false, RING_MX>(p, st);
  set_error("conv3x3 (f16mx): unsupported layer cin=%d cout=%d at N=%d H=%d W=%d (needs Cin %% 64 == 0, "
            "Cout %% 128 == 0 and an input below 3.5 GB)", p.cin, p.cout, p.N, p.H, p.W);
  return OIBL_E_UNSUPPORTED;
}

OIBL_HOOK(int, g_conv_c64, 1);     // test hook: 0 = never the Cin = 64 kernel (stem.hip), 1 = auto, 2 = every Cin = 64 layer
OIBL_HOOK(int, g_conv_splitk, 1);  // test hook: 0 = never split K

// splitk_ws (optional): scratch for the split-K partials of layers with too few tiles
// (conv_splitk_bytes); without it every layer runs one-pass
static size_t conv_splitk_bytes(long m_total, int cin, int cout, int precision) {
  if (precision == OIBL_F16MX) return 0;  // (its own plan: mx_split_bytes)
  const int steps = 9 * (cin / (precision == OIBL_BF16 ? 64 : 32));
  const int s = conv_splitk_factor(m_total, cout, steps);
  return s ? align_up((size_t)s * m_total * cout * sizeof(float), 256) : 0;
}

// scratch of one layer's split-K partials (0: the layer runs in one pass), any precision
size_t conv_layer_scratch_bytes(int N, int h, int w, int cin, int cout, int pool, int precision) {
  if (precision == OIBL_F16MX) {   // (either K order: the order is a per-layer default a test hook can change)
    const size_t a = mx_split_bytes((long)N * h * w, cin, cout, pool, 0), b = mx_split_bytes((long)N * h * w, cin, cout, pool, 1);
    return a > b ? a : b;
  }
  const long m_total = pool ? (long)N * (h / 2) * (w / 2) * 4 : (long)N * h * w;
  return conv_splitk_bytes(m_total, cin, cout, precision);
}

// out_f32 (bf16x3 / f16mx only): write the output as plain fp32 NHWC
int conv3x3_impl(const void* in, int N, int H, int W, int cin, const void* packed_w, const float* bias, int cout,
                 int relu, int pool, int precision, void* out, hipStream_t st, int out_f32, void* splitk_ws,
                 unsigned* range_flag, float bias_mul, float out_mul) {
  OIBL_REQUIRE(in && packed_w && bias && out, "conv3x3: null pointer");
  OIBL_REQUIRE(precision_ok(precision), "conv3x3: bad precision %d", precision);
  const int bk = precision == OIBL_BF16 ? 64 : 32;
  OIBL_REQUIRE(N > 0 && H > 0 && W > 0, "conv3x3: bad shape N=%d H=%d W=%d", N, H, W);
  OIBL_REQUIRE(cin % bk == 0 && cout % 64 == 0, "conv3x3: unsupported channels cin=%d cout=%d", cin,
               cout);
  OIBL_REQUIRE(!pool || (H >= 2 && W >= 2), "conv3x3: pooling needs H,W >= 2");
  OIBL_REQUIRE((long)N * H * W < 0x7fffffffL, "conv3x3: N*H*W must be < 2^31 (split the batch)");
  OIBL_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)packed_w % 16 == 0 && (uintptr_t)out % 16 == 0,
               "conv3x3: pointers must be 16-byte aligned");
  // Cin = 64: the resident-weights / LDS-halo kernel serves Cout = 64 (conv1_2); from Cout = 128 on
  // the 512 x 128 ring kernel is faster (conv2_1: 795 vs 680 TFLOP/s) unless the hook forces c64.
  if (precision == OIBL_BF16 && cin == 64 && g_conv_c64 && !g_regstage && !g_conv_ablate &&
      (g_conv_c64 == 2 || cout % 128 != 0))
    return launch_conv_c64(in, N, H, W, packed_w, bias, cout, relu, pool, out, st);
  ConvParams p;
  p.in = in;
  p.w = packed_w;
  p.bias = bias;
  p.out = out;
  p.zero = zero_line_device_ptr();
  OIBL_REQUIRE(p.zero != nullptr, "conv3x3: zero line symbol not found");
  p.N = N;
  p.H = H;
  p.W = W;
  p.cin = cin;
  p.cout = cout;
  p.relu = relu;
  p.ablate = g_conv_ablate;
  p.out_f32 = (precision == OIBL_BF16X3 || precision == OIBL_F16MX) ? out_f32 : 0;
  p.korder = conv_korder_for(precision, cin, cout);
  p.tiles_n = 0;
  if (pool) {
    p.out_rows = (long)N * (H / 2) * (W / 2);
    p.m_total = p.out_rows * 4;
  } else {
    p.out_rows = (long)N * H * W;
    p.m_total = p.out_rows;
  }
  p.ksplit = 0;
  p.partial = (float*)splitk_ws;
  p.range_flag = range_flag;
  p.bias_mul = bias_mul;
  p.out_mul = out_mul;
  if (splitk_ws && g_conv_splitk && precision != OIBL_F16MX)
    p.ksplit = conv_splitk_factor(p.m_total, cout, 9 * (cin / bk));
  if (precision == OIBL_F16MX) return launch_conv_mx(p, pool, st);
  if (precision == OIBL_BF16X3) return launch_conv<bf16x3_t>(p, pool, st);
  return precision == OIBL_BF16 ? launch_conv<bf16_t>(p, pool, st) : launch_conv<float>(p, pool, st);
}

// ---- small kernels of the VGG16 forward (vgg.hip) ----
// They are non-template kernels and stay in this unit, behind its other non-template kernels and in this order:
// the compiler pads the end of a unit's text with 1 KiB of s_nop, build.kernel_text() counts that into the unit's
// LAST non-template kernel, and that kernel has been u8_nhwc_to_nchw_f32_kernel in every build whose figures are
// on record.
__global__ void clear_word_kernel(unsigned* w) { *w = 0u; }

// uint8 NHWC -> normalised fp32 NCHW with the loader's arithmetic ((u / 255 - mean) / std, fp32,
// correctly rounded divisions): the route of the uint8 entry point whenever the fused stem is not
// used (fp32 precision, test hooks)
__global__ void u8_nhwc_to_nchw_f32_kernel(const uint8_t* __restrict__ x, float* __restrict__ out,
                                           long npix_total, long plane, float m0, float m1, float m2,
                                           float s0, float s1, float s2) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npix_total;
       i += (long)gridDim.x * blockDim.x) {
    const long n = i / plane, pix = i - n * plane;
    const uint8_t* px = x + i * 3;
    float* o = out + n * 3 * plane + pix;
    o[0] = ((float)px[0] / 255.0f - m0) / s0;
    o[plane] = ((float)px[1] / 255.0f - m1) / s1;
    o[2 * plane] = ((float)px[2] / 255.0f - m2) / s2;
  }
}

int launch_clear_word(unsigned* w, hipStream_t st) {
  hipLaunchKernelGGL(clear_word_kernel, dim3(1), dim3(1), 0, st, w);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}
// mean3 / std3: host pointers
int launch_u8_nhwc_to_nchw_f32(const uint8_t* x, float* out, long npix_total, long plane, const float* mean3,
                               const float* std3, hipStream_t st) {
  hipLaunchKernelGGL(u8_nhwc_to_nchw_f32_kernel, dim3(2048), dim3(256), 0, st, x, out, npix_total, plane, mean3[0],
                     mean3[1], mean3[2], std3[0], std3[1], std3[2]);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

// f16mx lines -> n fp32 values (mx_join_rows_kernel); vgg.hip converts a stored activation with it
int launch_mx_join_rows(const void* src, float* dst, size_t n, int which, float mul, unsigned max_blocks,
                        hipStream_t st) {
  const unsigned b = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(mx_join_rows_kernel, dim3(b > max_blocks ? max_blocks : b), dim3(256), 0, st, (const char*)src,
                     dst, n, which, mul);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

}  // namespace oibl

using namespace oibl;

extern "C" {

#ifdef OIBL_DEBUG_HOOKS
int oibl_debug_set_prof_buffer(void* dev_u64x8) {
  g_prof_buf = (unsigned long long*)dev_u64x8;
  return OIBL_OK;
}

int oibl_debug_set_conv_c64(int on) {  // 0 = off, 1 = auto, 2 = every Cin = 64 layer
  g_conv_c64 = on < 0 ? 0 : (on > 2 ? 2 : on);
  return OIBL_OK;
}

int oibl_debug_set_conv_ablate(int mode) {
  g_conv_ablate = mode;
  return OIBL_OK;
}

int oibl_debug_set_ring_ablate(int mode) {
  g_ring_ablate = mode;
  return OIBL_OK;
}

int oibl_debug_set_conv_splitk(int on) {
  g_conv_splitk = on ? 1 : 0;
  return OIBL_OK;
}

int oibl_debug_set_mx_variant(int v) {   // 0 = auto, 1 = ring kernels only, 3 = halo kernel wherever legal
  OIBL_REQUIRE(v == 0 || v == 1 || v == 3, "oibl_debug_set_mx_variant: %d is not one of 0, 1, 3", v);
  g_mx_variant = v;
  return OIBL_OK;
}

int oibl_debug_set_conv_korder(int mode) {
  g_conv_korder = mode < 0 ? -1 : (mode ? 1 : 0);
  return OIBL_OK;
}

int oibl_debug_set_mx_splitk(int on) {
  g_mx_splitk = on == 2 ? 2 : (on ? 1 : 0);
  return OIBL_OK;
}

int oibl_debug_set_ring_raster(int mode) {
  g_ring_raster = mode;
  return OIBL_OK;
}

int oibl_debug_set_conv_tile(int mode) {
  g_conv_tile = mode;
  return OIBL_OK;
}
#endif

size_t oibl_conv3x3_packed_bytes(int cout, int cin, int precision) {
  return (size_t)9 * cout * cin * oibl_elem_size(precision);
}

int oibl_pack_conv3x3_weights(const float* w_oihw, int cout, int cin, int precision, void* packed,
                              void* stream) {
  OIBL_REQUIRE(w_oihw && packed, "pack_conv3x3_weights: null pointer");
  OIBL_REQUIRE(cout > 0 && cin > 0, "pack_conv3x3_weights: bad shape");
  OIBL_REQUIRE(precision_ok(precision), "pack_conv3x3_weights: bad precision %d", precision);
  OIBL_REQUIRE((precision != OIBL_BF16X3 && precision != OIBL_F16MX) || cin % 32 == 0,
               "pack_conv3x3_weights: bf16x3 / f16mx need Cin %% 32 == 0");
  const size_t total = (size_t)9 * cout * cin;
  unsigned blocks = (unsigned)((total + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  if (precision == OIBL_F16MX) {
    unsigned b = (unsigned)((total / 32 + 127) / 128);
    hipLaunchKernelGGL(pack_conv3x3_mx_kernel, dim3(b > 8192 ? 8192 : b), dim3(128), 0, (hipStream_t)stream, w_oihw,
                       (char*)packed, cout, cin);
  } else if (precision == OIBL_BF16)
    hipLaunchKernelGGL(pack_conv3x3_kernel<bf16_t>, dim3(blocks), dim3(256), 0,
                       (hipStream_t)stream, w_oihw, (bf16_t*)packed, cout, cin);
  else if (precision == OIBL_BF16X3)
    hipLaunchKernelGGL(pack_conv3x3_kernel<bf16x3_t>, dim3(blocks), dim3(256), 0,
                       (hipStream_t)stream, w_oihw, (bf16x3_t*)packed, cout, cin);
  else
    hipLaunchKernelGGL(pack_conv3x3_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       w_oihw, (float*)packed, cout, cin);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

int oibl_conv3x3_nhwc(const void* in, int N, int H, int W, int cin, const void* packed_w,
                      const float* bias, int cout, int relu, int pool, int precision, void* out,
                      void* stream) {
  return conv3x3_impl(in, N, H, W, cin, packed_w, bias, cout, relu, pool, precision, out,
                      (hipStream_t)stream);
}

int oibl_conv3x3_nhwc_flagged(const void* in, int N, int H, int W, int cin, const void* packed_w,
                              const float* bias, int cout, int relu, int pool, int precision, void* out,
                              uint32_t* range_flag, void* stream) {
  OIBL_REQUIRE(range_flag == nullptr || (uintptr_t)range_flag % 4 == 0, "conv3x3: range flag must be 4-byte aligned");
  return conv3x3_impl(in, N, H, W, cin, packed_w, bias, cout, relu, pool, precision, out,
                      (hipStream_t)stream, 0, nullptr, range_flag);
}

size_t oibl_conv3x3_workspace_bytes(int N, int H, int W, int cin, int cout, int pool, int precision) {
  if (N <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || !precision_ok(precision)) return 0;
  return conv_layer_scratch_bytes(N, H, W, cin, cout, pool, precision);
}

int oibl_conv3x3_nhwc_ws(const void* in, int N, int H, int W, int cin, const void* packed_w, const float* bias,
                         int cout, int relu, int pool, int precision, void* out, void* ws, size_t ws_bytes,
                         uint32_t* range_flag, void* stream) {
  OIBL_REQUIRE(range_flag == nullptr || (uintptr_t)range_flag % 4 == 0, "conv3x3: range flag must be 4-byte aligned");
  // ws == NULL: the layer runs in one pass whatever its size (exactly oibl_conv3x3_nhwc_flagged)
  const size_t need = ws ? oibl_conv3x3_workspace_bytes(N, H, W, cin, cout, pool, precision) : 0;
  if (need && ws_bytes < need) {
    set_error("conv3x3: workspace %zu < required %zu bytes", ws_bytes, need);
    return OIBL_E_WORKSPACE;
  }
  OIBL_REQUIRE(!need || (uintptr_t)ws % 256 == 0, "conv3x3: workspace must be 256-byte aligned");
  return conv3x3_impl(in, N, H, W, cin, packed_w, bias, cout, relu, pool, precision, out,
                      (hipStream_t)stream, 0, need ? ws : nullptr, range_flag);
}

int oibl_x3_split_rows(const float* src, void* dst, size_t rows, int C, void* stream) {
  OIBL_REQUIRE(src && dst, "x3_split_rows: null pointer");
  OIBL_REQUIRE(C > 0 && C % 32 == 0, "x3_split_rows: C=%d must be a positive multiple of 32", C);
  if (rows == 0) return OIBL_OK;
  const size_t n = rows * (size_t)C;
  size_t blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(x3_split_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src,
                     (char*)dst, n, C);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

int oibl_mx_split_rows_flagged(const float* src, void* dst, size_t rows, int C, uint32_t* range_flag,
                               void* stream) {
  OIBL_REQUIRE(src && dst, "mx_split_rows: null pointer");
  OIBL_REQUIRE(C > 0 && C % 32 == 0, "mx_split_rows: C %% 32 != 0");
  OIBL_REQUIRE(range_flag == nullptr || (uintptr_t)range_flag % 4 == 0, "mx_split_rows: range flag must be 4-byte aligned");
  if (rows == 0) return OIBL_OK;
  const size_t lines = rows * (size_t)(C / 32);
  unsigned b = (unsigned)((lines + 255) / 256);
  hipLaunchKernelGGL(mx_pack_rows_kernel<0>, dim3(b > 16384 ? 16384 : b), dim3(256), 0, (hipStream_t)stream,
                     (const char*)src, (char*)dst, lines, (unsigned*)range_flag);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

int oibl_mx_split_rows(const float* src, void* dst, size_t rows, int C, void* stream) {
  return oibl_mx_split_rows_flagged(src, dst, rows, C, nullptr, stream);
}

int oibl_mx_join_rows(const void* src, float* dst, size_t rows, int C, int which, void* stream) {
  OIBL_REQUIRE(src && dst, "mx_join_rows: null pointer");
  OIBL_REQUIRE(C > 0 && C % 32 == 0 && which >= 0 && which <= 3, "mx_join_rows: bad arguments");
  if (rows == 0) return OIBL_OK;
  return launch_mx_join_rows(src, dst, rows * (size_t)C, which, 1.f, 16384, (hipStream_t)stream);
}

int oibl_x3_join_rows(const void* src, float* dst, size_t rows, int C, void* stream) {
  OIBL_REQUIRE(src && dst, "x3_join_rows: null pointer");
  OIBL_REQUIRE(C > 0 && C % 32 == 0, "x3_join_rows: C=%d must be a positive multiple of 32", C);
  if (rows == 0) return OIBL_OK;
  const size_t n = rows * (size_t)C;
  size_t blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(x3_join_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     (const char*)src, dst, n, C);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

}  // extern "C"
