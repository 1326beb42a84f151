// The per-image geometry table of csrc/jpeg.hip: a batch of JPEG files of MIXED stored sizes.  Like
// jpeg_entropy.h this text is compiled into the library and, without hipcc, into a host program
// (tests/helpers/jpeg_mixed_harness.cpp): nothing here needs a HIP header.
//
//   jpeg_mixed_layout   host: sizes[N][2] = {H, W} -> geom[N][JPEG_MIX_GEOM_INTS] and the totals.  The images lie back
//                       to back in four spaces: the int16 coefficients coef[3][Bh][Bw][64] and the uint8 sample planes
//                       [3][Bh * 8][Bw * 8] of the workspace (Bw = 2 ceil(W / 16), Bh = 2 ceil(H / 16): 9 bytes per
//                       MCU-padded pixel, the uniform decoder's formula per image), and the packed pixels
//                       [H][W][3] uint8, every image at a multiple of JPEG_MIX_PIX_ALIGN bytes.
//   jpeg_mixed_image    device (and the host program): row n of the table, every entry forced into its range and the
//                       image's extent in all three spaces checked against the totals the CALL was given.  ok == 0:
//                       the kernels skip the image (status JPEG_ST_BAD_GEOM).  No read or write depends on the table
//                       being right: an image that passes lies inside [0, total) of every space.
//
// A row: {H, W, coefficient base in blocks of 64 coefficients, sample-plane base in units of 64 bytes, packed-pixel
// byte offset low 32 bits, high bits, 0, 0}.  The two bases are equal numbers in a table the layout function wrote (a
// block of 64 coefficients becomes 64 samples); the kernels take each from its own entry.
#pragma once

#include <stddef.h>

#include "jpeg_entropy.h"

#define JPEG_MIX_GEOM_INTS 8
enum { JPEG_MIX_H = 0, JPEG_MIX_W, JPEG_MIX_COEF, JPEG_MIX_PLANE, JPEG_MIX_PIX_LO, JPEG_MIX_PIX_HI };

// the totals, as the C ABI passes them (size_t[JPEG_MIX_TOTALS])
#define JPEG_MIX_TOTALS 6
enum {
  JPEG_MIX_T_COEF_BYTES = 0, JPEG_MIX_T_PLANE_BYTES, JPEG_MIX_T_PIXEL_BYTES, JPEG_MIX_T_MAX_BLOCKS, JPEG_MIX_T_MAX_H,
  JPEG_MIX_T_MAX_W
};

#define JPEG_MIX_PIX_ALIGN 64
#define JPEG_MIX_MAX_DIM 32768
#define JPEG_MIX_MAX_PIXEL_BYTES ((uint64_t)1 << 40)   // exclusive
#define JPEG_MIX_MAX_BLOCKS ((uint64_t)1 << 31)        // exclusive: a base is an int32

#define JPEG_ST_BAD_GEOM 5   // "geometry table inconsistent"

// why jpeg_mixed_layout refused (0: it did not); *bad is the image
#define JPEG_MIX_E_SIZE 1     // H or W outside [1, JPEG_MIX_MAX_DIM]
#define JPEG_MIX_E_BLOCKS 2   // 2^31 coefficient blocks or more
#define JPEG_MIX_E_PIXELS 3   // 2^40 packed pixel bytes or more.  A guard that cannot fire while a base is an int32: a
                              // block of 64 coefficients stands for at most 192 pixel bytes, so fewer than 2^31 blocks
                              // are fewer than 2^39 pixel bytes, and JPEG_MIX_E_BLOCKS comes first

static inline int jpeg_mixed_layout(const int32_t* sizes, int N, int32_t* geom, size_t* totals, int* bad) {
  uint64_t blocks = 0, pix = 0, pix_end = 0;
  uint64_t max_blocks = 0;
  int max_h = 0, max_w = 0;
  for (int n = 0; n < N; ++n) {
    const int H = sizes[2 * n], W = sizes[2 * n + 1];
    *bad = n;
    if (H < 1 || W < 1 || H > JPEG_MIX_MAX_DIM || W > JPEG_MIX_MAX_DIM) return JPEG_MIX_E_SIZE;
    const uint64_t bb = (uint64_t)jpeg_blocks_across(W) * (uint64_t)jpeg_blocks_across(H);
    if (blocks + 3 * bb >= JPEG_MIX_MAX_BLOCKS) return JPEG_MIX_E_BLOCKS;
    pix = (pix_end + JPEG_MIX_PIX_ALIGN - 1) / JPEG_MIX_PIX_ALIGN * JPEG_MIX_PIX_ALIGN;
    pix_end = pix + (uint64_t)H * (uint64_t)W * 3;
    if (pix_end >= JPEG_MIX_MAX_PIXEL_BYTES) return JPEG_MIX_E_PIXELS;
    int32_t* row = geom + (size_t)n * JPEG_MIX_GEOM_INTS;
    row[JPEG_MIX_H] = H, row[JPEG_MIX_W] = W;
    row[JPEG_MIX_COEF] = row[JPEG_MIX_PLANE] = (int32_t)blocks;
    row[JPEG_MIX_PIX_LO] = (int32_t)(uint32_t)(pix & 0xFFFFFFFFu), row[JPEG_MIX_PIX_HI] = (int32_t)(pix >> 32);
    row[6] = row[7] = 0;
    blocks += 3 * bb;
    if (bb > max_blocks) max_blocks = bb;
    if (H > max_h) max_h = H;
    if (W > max_w) max_w = W;
  }
  totals[JPEG_MIX_T_COEF_BYTES] = (size_t)(blocks * 64 * sizeof(int16_t));
  totals[JPEG_MIX_T_PLANE_BYTES] = (size_t)(blocks * 64);
  totals[JPEG_MIX_T_PIXEL_BYTES] = (size_t)pix_end;
  totals[JPEG_MIX_T_MAX_BLOCKS] = (size_t)max_blocks;
  totals[JPEG_MIX_T_MAX_H] = (size_t)max_h;
  totals[JPEG_MIX_T_MAX_W] = (size_t)max_w;
  *bad = -1;
  return 0;
}

// what the kernels are told about the spaces (from the call's totals; passed by value)
struct JpegMixSpaces {
  uint64_t coef_blocks;    // blocks of 64 coefficients in the workspace
  uint64_t plane_blocks;   // units of 64 sample bytes in the workspace
  uint64_t pixel_bytes;    // of the packed output
  int max_blocks, max_h, max_w;   // the grids are sized by them
};

struct JpegMixImage {
  int H, W;                // in [1, 32768] x [8, 32768]
  uint32_t coef, plane;    // the bases, in blocks
  uint64_t pix;            // byte offset of the pixels
  int ok;
};

JPEG_HD static inline JpegMixImage jpeg_mixed_image(const int32_t* row, const JpegMixSpaces& t) {
  JpegMixImage m;
  const int h = row[JPEG_MIX_H], w = row[JPEG_MIX_W];
  m.H = h < 1 ? 1 : (h > JPEG_MIX_MAX_DIM ? JPEG_MIX_MAX_DIM : h);
  m.W = w < 8 ? 8 : (w > JPEG_MIX_MAX_DIM ? JPEG_MIX_MAX_DIM : w);
  const int32_t cb = row[JPEG_MIX_COEF], pb = row[JPEG_MIX_PLANE], hi = row[JPEG_MIX_PIX_HI];
  m.coef = cb > 0 ? (uint32_t)cb : 0u;
  m.plane = pb > 0 ? (uint32_t)pb : 0u;
  m.pix = (uint64_t)(uint32_t)row[JPEG_MIX_PIX_LO] | (uint64_t)(uint32_t)(hi & 0xFF) << 32;
  const uint64_t bb = (uint64_t)jpeg_blocks_across(m.W) * (uint64_t)jpeg_blocks_across(m.H);   // <= 2^24
  m.ok = h == m.H && w == m.W && m.H <= t.max_h && m.W <= t.max_w && bb <= (uint64_t)t.max_blocks && cb >= 0 &&
         pb >= 0 && hi >= 0 && hi <= 0xFF && (uint64_t)m.coef + 3 * bb <= t.coef_blocks &&
         (uint64_t)m.plane + 3 * bb <= t.plane_blocks &&
         m.pix + (uint64_t)m.H * (uint64_t)m.W * 3 <= t.pixel_bytes;
  return m;
}
