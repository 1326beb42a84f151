// What the forward (vlad_forward_core.h) and the backward (vlad_backward_core.h) of the two NetVLAD heads agree on:
// the head's shape, the LDS pitches of a 32-pixel chunk, the norm clamp, and where a quarter's pixel lies in the map.
#pragma once

#include "gemm_core.h"

namespace oibl {

constexpr int VLAD_C = 512;
constexpr int VLAD_K = 64;
constexpr int VLAD_XP = 516;         // floats per LDS row of the chunk: 16-byte aligned, +4 banks per pixel
constexpr int VLAD_LP = 65;          // pitch of the [32][64] logit / assignment / partial tiles
constexpr float VLAD_EPS = 1e-12f;   // F.normalize's clamp of a norm

// The map pixel (row of the image's row-major 2 hq x 2 wq NHWC map) of pixel i of quarter q: q0 top-left, q1
// top-right, q2 bottom-left, q3 bottom-right, row-major inside the quarter.
__device__ __forceinline__ int quarter_map_pixel(int q, int i, int hq, int wq) {
  const int row = i / wq, col = i - row * wq;
  return ((q >> 1) * hq + row) * (2 * wq) + (q & 1) * wq + col;
}

}  // namespace oibl
