// Coefficient tables of PIL's 8-bit bilinear resampling (resize.hip): one axis, `in` -> `out` samples.
//
// PIL computes, per axis, a window [xmin, xmin + n) of source samples for every output sample and n triangle
// weights in IEEE double, normalises them by their sum and rounds them to 22-bit fixed point; the resampling itself
// is integer.  The functions below repeat that arithmetic operation by operation.  The includer switches
// floating-point contraction OFF for the whole unit: a fused (xx + 0.5) * scale - support moves xmin.  Host and
// device compile the same text (the host side sizes the tables and serves a stand-alone check).
//
// Limits of the one resampling path (resize.hip), derived from its tile of RS_TILE_H x RS_TILE_W output pixels:
// the horizontal pass of a tile writes every source row the tile's RS_TILE_H output rows read into LDS, next to the
// tile's table rows.  A tile reads fewer than (RS_TILE_H - 1) scale + 2 support + 1 source rows: the distance of its
// first and its last centre, the support on either side, and the rounding of the two ends (rs_tile_rows).  The
// kernel sizes its LDS by the call's own scale; at a downscale factor of RS_MAX_SCALE = 16 per axis — a row of
// coefficients then has RS_MAX_KSIZE = 33 entries — that is 274 rows of 192 bytes + 80 table rows of 35 ints =
// 63 808 bytes, the most that stays inside the 64 KiB every launch may take without raising a limit.  Larger
// factors are refused.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define OIBL_RS __host__ __device__ __forceinline__
#else
#define OIBL_RS static inline
#endif

namespace oibl {

constexpr int RS_PRECISION_BITS = 22;                             // PIL: 32 - 8 - 2
constexpr int RS_TILE_H = 16;                                     // output rows of a workgroup's tile
constexpr int RS_TILE_W = 64;                                     // output columns of a workgroup's tile
constexpr int RS_MAX_SCALE = 16;                                  // largest in / out per axis
constexpr int RS_MAX_KSIZE = 2 * RS_MAX_SCALE + 1;                // 33

struct ResizeAxis {
  double scale;     // in / out
  double fs;        // max(scale, 1): the filter's scale
  double support;   // bilinear: 1.0 * fs
  double ss;        // 1 / fs
  int ksize;        // entries of a row of coefficients
};

OIBL_RS ResizeAxis rs_axis(int in_size, int out_size) {
  ResizeAxis a;
  a.scale = (double)in_size / (double)out_size;
  a.fs = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = 1.0 * a.fs;
  a.ss = 1.0 / a.fs;
  a.ksize = (int)__builtin_ceil(a.support) * 2 + 1;
  return a;
}

// an upper bound of the source rows (columns) RS_TILE_H consecutive output samples of this axis read
OIBL_RS int rs_tile_rows(const ResizeAxis& a) {
  return (int)((double)(RS_TILE_H - 1) * a.scale + 2.0 * a.support + 1.0) + 1;
}

OIBL_RS double rs_triangle(double v) {
  if (v < 0.0) v = -v;
  return v < 1.0 ? 1.0 - v : 0.0;
}

// the window of output sample xx: xmin and the number of taps n (PIL's bounds[2 xx], bounds[2 xx + 1])
OIBL_RS void rs_bounds(const ResizeAxis& a, int in_size, int xx, int& xmin, int& n) {
  const double center = ((double)xx + 0.5) * a.scale;
  xmin = (int)(center - a.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + a.support + 0.5);
  if (xmax > in_size) xmax = in_size;
  n = xmax - xmin;
}

// one row of the tables: bounds2 = {xmin, n}, coeff[0, ksize) = the fixed-point weights, zero behind the n-th
OIBL_RS void rs_table_row(const ResizeAxis& a, int in_size, int xx, int32_t* bounds2, int32_t* coeff) {
  int xmin, n;
  rs_bounds(a, in_size, xx, xmin, n);
  const double center = ((double)xx + 0.5) * a.scale;
  double ww = 0.0;
  for (int x = 0; x < n; ++x) ww += rs_triangle(((double)(x + xmin) - center + 0.5) * a.ss);
  for (int x = 0; x < a.ksize; ++x) {
    double k = 0.0;
    if (x < n) {
      k = rs_triangle(((double)(x + xmin) - center + 0.5) * a.ss);
      if (ww != 0.0) k = k / ww;
    }
    coeff[x] = k < 0.0 ? (int32_t)(-0.5 + k * 4194304.0) : (int32_t)(0.5 + k * 4194304.0);
  }
  bounds2[0] = xmin;
  bounds2[1] = n;
}

// one output byte from its accumulated sum (the caller starts the sum at 1 << 21)
OIBL_RS int rs_clip8(int ss) {
  const int v = ss >> RS_PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

}  // namespace oibl
