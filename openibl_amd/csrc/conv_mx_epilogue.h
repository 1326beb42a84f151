// What the f16mx 3x3 convolution kernels share around their K loops: the f16mx epilogue of the ring kernels
// (conv_ring.h), the halo kernel (conv_halo.h) and the 4-wave halo kernel (conv_halo4.h), and the two halo kernels'
// start of the accumulators at the bias and activation scale behind the loop.  All of them hold a 128-row x
// 64-column wave tile as f32x16_t acc[4][2] (row tile i, column tile j; wave (wm, wn) of the workgroup's BM x BN tile).
#pragma once

#include "ring_core.h"

namespace oibl {

// The accumulators start at bias * bias_mul, laid out like the results (conv3x3_ring_body, conv_ring.h: natural
// layout with pooling, transposed without).  c0: first channel of the wave tile.
// conv3x3_ring_body keeps its own copy of this block and of the next one (with the split-K zero start): it serves
// the bf16 and bf16x3 kernels too, and called from there the two helpers changed those kernels' text — six of ten
// took one or two registers more.
template <bool POOL>
__device__ __forceinline__ void conv_acc_init_bias(f32x16_t (&acc)[4][2], const float* bias, const int c0,
                                                   const float bias_mul, const int lane) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if constexpr (POOL) {
      float b = bias[c0 + j * 32 + (lane & 31)] * bias_mul;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          asm volatile("" : "+v"(b));  // 64 distinct registers, not 64 aliases of one value
          acc[i][j][r] = b;
        }
    } else {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float4 b = *reinterpret_cast<const float4*>(bias + c0 + j * 32 + 8 * g + 4 * (lane >> 5));
        b = make_float4(b.x * bias_mul, b.y * bias_mul, b.z * bias_mul, b.w * bias_mul);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[i][j][4 * g] = b.x;
          acc[i][j][4 * g + 1] = b.y;
          acc[i][j][4 * g + 2] = b.z;
          acc[i][j][4 * g + 3] = b.w;
        }
      }
    }
  }
}

// out_mul != 1 (uniform): the layer of the f16mx backbone that hands the fp32 map to the head undoes the activation
// scale (RingParams::out_mul), once behind the loop.
__device__ __forceinline__ void conv_acc_scale(f32x16_t (&acc)[4][2], const float out_mul) {
  if (out_mul != 1.f) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] *= out_mul;
  }
}

// LDS the epilogue stages in: the tile's output rows (without pooling: one half of them at a time) as fp32
template <int BM, int BN, bool POOL>
constexpr int conv_mx_epilogue_lds() {
  return (POOL ? BM / 4 : BM / 2) * BN * 4;
}

// ---- f16mx epilogue: (+ReLU) (+2x2 max-pool over register quads), transpose through LDS, f16mx lines out.
//      POOL : accumulators in the natural layout (lane = channel, registers = pixels): a pooling window is one
//             register quad -> three v_max, one 4-byte LDS write of the pooled value.
//      !POOL: accumulators transposed (lane = pixel, register quad = 4 consecutive channels): one 16-byte LDS
//             write per quad; the tile is staged in two passes of BM / 2 rows (accumulator row tiles {0, 1},
//             then {2, 3} of every wave).
// The tile (one pass of it) is staged as fp32, rows of BN floats = CPR 16-byte chunks, chunk q of row r at
// physical chunk q ^ (r % CPR): the 8 chunks of a (row, 32-channel group) item stay inside one aligned 128-byte
// block, 16 consecutive rows of one logical chunk fall on 16 distinct bank slots (the accumulator writes and the
// item reads walk rows), and a row's chunks read in order are a permutation of the row (the copy-out walks
// chunks).  Then one thread per item reads its 32 values, packs the f16mx line (mx_pack_line) and writes it back
// in place; the copy-out moves full lines, the LDS reads of a batch first, then its stores: the loads' latency is
// paid once per batch.
// out_f32 (the layer feeding the fp32 head, split-K partials): no packing, the fp32 rows go out as they are.
// Hazards: the caller's K loop ends on a workgroup barrier (its staging LDS is free); a barrier separates the
// accumulator writes from the item reads, the in-place line writes from the copy-out, and the copy-out's reads
// from the next pass's writes.
// tile_rows: where a tile row goes (RingRowMap: a run of the flattened tensor; HaloRowMap: a pixel of the patch) —
// at_byte(b): the same map for byte b of this tile's channels; store(r, v): 16 bytes to tile row r (pooled: quad
// r) there, if that row is an output row at all.  What does not depend on r is computed when a map is made, by
// hand: a map's methods are optimised before they are inlined here, where nothing looks loop-invariant yet.
// stamp(pass, k): called on all threads behind pass `pass`'s staging barrier (k = 0), packing (1) and store issue
// (2) — the ring kernels' profile stamps; a no-op elsewhere.
template <int BM, int BN, int THREADS, bool POOL, typename Rows, typename Stamp>
__device__ __forceinline__ void conv_mx_epilogue(f32x16_t (&acc)[4][2], char* smem, const int wm, const int wn,
                                                 const int lane, const int relu, const int out_f32,
                                                 unsigned* range_flag, const Rows& tile_rows, Stamp&& stamp) {
  constexpr int CPR = BN / 4;
  constexpr int ROWB = BN * 4;
  constexpr int PASSES = POOL ? 1 : 2;
  constexpr int ROWS = (POOL ? BM / 4 : BM) / PASSES;
  constexpr int ITEMS = ROWS * (BN / 32);
  constexpr int ITERS = ROWS * CPR / THREADS, BATCH = 8;
  static_assert(ITEMS % THREADS == 0 && ITERS % BATCH == 0, "f16mx epilogue shape");
  static_assert(ROWS * ROWB == conv_mx_epilogue_lds<BM, BN, POOL>(), "f16mx epilogue staging");
  static_assert(THREADS % CPR == 0, "a thread copies out the same chunk of every row it handles");
  const Rows rows = tile_rows.at_byte(((int)threadIdx.x % CPR) * 16);
  const float floor_v = relu ? 0.f : -INFINITY;
#pragma unroll
  for (int pass = 0; pass < PASSES; ++pass) {
    if constexpr (POOL) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = wn * 64 + j * 32 + (lane & 31);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float v = fmaxf(fmaxf(fmaxf(acc[i][j][4 * g], acc[i][j][4 * g + 1]),
                                        fmaxf(acc[i][j][4 * g + 2], acc[i][j][4 * g + 3])), floor_v);
            const int row = (wm * 4 + i) * 8 + 2 * g + (lane >> 5);
            *reinterpret_cast<float*>(smem + row * ROWB + (((col >> 2) ^ (row & (CPR - 1))) << 4) + (col & 3) * 4) = v;
          }
      }
    } else {
      const int half = lane >> 5;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int q = (wn * 64 + j * 32 + 8 * g + 4 * half) >> 2;  // chunk of this quad's 4 channels
#pragma unroll
          for (int i2 = 0; i2 < 2; ++i2) {
            const int i = 2 * pass + i2;
            const int row = wm * 64 + i2 * 32 + (lane & 31);
            *reinterpret_cast<float4*>(smem + row * ROWB + ((q ^ (row & (CPR - 1))) << 4)) =
                make_float4(fmaxf(acc[i][j][4 * g], floor_v), fmaxf(acc[i][j][4 * g + 1], floor_v),
                            fmaxf(acc[i][j][4 * g + 2], floor_v), fmaxf(acc[i][j][4 * g + 3], floor_v));
          }
        }
    }
    __syncthreads();
    stamp(pass, 0);
    if (!out_f32) {
#pragma unroll 1
      for (int it = 0; it < ITEMS / THREADS; ++it) {
        const int item = it * THREADS + (int)threadIdx.x;
        const int row = item % ROWS, grp = item / ROWS;
        char* const rowp = smem + row * ROWB;
        const int sw = row & (CPR - 1);
        float v[32];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float4 t = *reinterpret_cast<const float4*>(rowp + (((grp * 8 + k) ^ sw) << 4));
          v[4 * k] = t.x;
          v[4 * k + 1] = t.y;
          v[4 * k + 2] = t.z;
          v[4 * k + 3] = t.w;
        }
        uint4 line[8];
        mx_pack_line(v, line, range_flag);
#pragma unroll
        for (int k = 0; k < 8; ++k) *reinterpret_cast<uint4*>(rowp + (((grp * 8 + k) ^ sw) << 4)) = line[k];
      }
      __syncthreads();
    }
    stamp(pass, 1);
#pragma unroll
    for (int it0 = 0; it0 < ITERS; it0 += BATCH) {
      uint4 v[BATCH];
#pragma unroll
      for (int u = 0; u < BATCH; ++u) {
        const int idx = (it0 + u) * THREADS + (int)threadIdx.x;
        const int lr = idx / CPR, q = idx % CPR;
        v[u] = *reinterpret_cast<const uint4*>(smem + lr * ROWB + ((q ^ (lr & (CPR - 1))) << 4));
      }
#pragma unroll
      for (int u = 0; u < BATCH; ++u) {
        const int idx = (it0 + u) * THREADS + (int)threadIdx.x;
        const int lr = idx / CPR;
        // staged row -> tile row: all rows in order, or (two passes) 64 of every wave row's 128
        const int r = PASSES == 1 ? lr : (lr >> 6) * 128 + pass * 64 + (lr & 63);
        rows.store(r, v[u]);
      }
    }
    stamp(pass, 2);
    if (pass + 1 < PASSES) __syncthreads();  // the staging rows are rewritten by the next pass
  }
}

}  // namespace oibl
