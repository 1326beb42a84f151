// The geometry of the colour jitter (augment.hip): how an image's pixels are shared among workgroups, and what the
// call on a packed batch of MIXED sizes (oibl_color_jitter_u8_mixed) makes of a row of the decoder's geometry table.
// Like jpeg_mixed.h this text is compiled into the library and, without hipcc, into a host program
// (tests/helpers/jitter_mixed_harness.cpp): nothing here needs a HIP header.
//
//   jitter_geom          H, W -> pixels per workgroup (`chunk`, a multiple of CJ_CHUNK chosen so that an image has at
//                        most CJ_MAX_PARTS workgroups) and the workgroups (= partial sums) of the image.
//   jitter_mixed_image   device (and the host program): row n of the table, every entry forced into its range, the
//                        image's extent checked against the packed_bytes the CALL was given and its part count
//                        against the grid the host's sizes gave.  ok == 0: both launches skip the image.  No read or
//                        write depends on the table being right: an image that passes lies inside [0, packed_bytes)
//                        and its partial sums inside its own row of the workspace.
//   jitter_mixed_host    host: sizes[N][2] -> the largest part count (the grid and the rows of the workspace).
#pragma once

#include <stddef.h>

#include "jpeg_mixed.h"

namespace oibl {

constexpr int CJ_THREADS = 256;
constexpr int CJ_WAVES = CJ_THREADS / 64;
constexpr int CJ_GROUP = 4;                        // pixels per lane and step
constexpr int CJ_STEP = CJ_THREADS * CJ_GROUP;     // pixels per workgroup and step
constexpr int CJ_CHUNK = 4 * CJ_STEP;              // the unit of a workgroup's share of an image
constexpr int CJ_MAX_PARTS = 1024;
constexpr long CJ_MAX_HW = 1L << 28;

struct JitterGeom {
  long HW;      // pixels per image
  int chunk;    // pixels per workgroup, a multiple of CJ_CHUNK
  int nparts;   // workgroups (and partial sums) per image
};

JPEG_HD static inline JitterGeom jitter_geom(int H, int W) {
  JitterGeom g;
  g.HW = (long)H * W;
  const long per = (long)CJ_CHUNK * CJ_MAX_PARTS;
  g.chunk = (int)(CJ_CHUNK * ((g.HW + per - 1) / per));
  g.nparts = (int)((g.HW + g.chunk - 1) / g.chunk);
  return g;
}

// what the kernels of the mixed call are told (from the call's arguments; passed by value)
struct JitterMixCall {
  unsigned long long packed_bytes;   // of the packed buffer(s)
  int max_parts;                     // the grid's x extent and the partial sums per row of the workspace
};

struct JitterMixImage {
  JitterGeom geo;            // of H x W, the image's OWN: the sums, and so the bits, of the uniform call on it alone
  unsigned long long pix;    // byte offset of the pixels
  int ok;
};

JPEG_HD static inline JitterMixImage jitter_mixed_image(const int32_t* row, const JitterMixCall& c) {
  JitterMixImage m;
  const int h = row[JPEG_MIX_H], w = row[JPEG_MIX_W], hi = row[JPEG_MIX_PIX_HI];
  const int H = h < 1 ? 1 : (h > JPEG_MIX_MAX_DIM ? JPEG_MIX_MAX_DIM : h);
  const int W = w < 1 ? 1 : (w > JPEG_MIX_MAX_DIM ? JPEG_MIX_MAX_DIM : w);
  m.geo = jitter_geom(H, W);
  m.pix = (unsigned long long)(uint32_t)row[JPEG_MIX_PIX_LO] | (unsigned long long)(uint32_t)(hi & 0xFF) << 32;
  m.ok = h == H && w == W && hi >= 0 && hi <= 0xFF && m.geo.HW <= CJ_MAX_HW && m.geo.nparts <= c.max_parts &&
         m.pix + (unsigned long long)m.geo.HW * 3 <= c.packed_bytes;
  return m;
}

// why jitter_mixed_host refused (0: it did not); *bad is the image
#define CJ_MIX_E_SIZE 1     // H or W outside [1, JPEG_MIX_MAX_DIM]
#define CJ_MIX_E_PIXELS 2   // more than CJ_MAX_HW pixels

static inline int jitter_mixed_host(const int32_t* sizes, int N, int* max_parts, int* bad) {
  int most = 0;
  for (int n = 0; n < N; ++n) {
    const int H = sizes[2 * n], W = sizes[2 * n + 1];
    *bad = n;
    if (H < 1 || W < 1 || H > JPEG_MIX_MAX_DIM || W > JPEG_MIX_MAX_DIM) return CJ_MIX_E_SIZE;
    if ((long)H * W > CJ_MAX_HW) return CJ_MIX_E_PIXELS;
    const int parts = jitter_geom(H, W).nparts;
    most = parts > most ? parts : most;
  }
  *bad = -1;
  *max_parts = most;
  return 0;
}

// Which bytes of an image a lane's group of CJ_GROUP pixels at `px` reads and writes as dwords (true) or one by one
// (false: the group that holds the image's end, or a base that is no multiple of 4).  The byte path reads nothing at
// or behind 3 HW (such a byte reads as zero) and writes nothing there: an image that ends inside a dword never
// touches the padding behind it or the next image's slot.
JPEG_HD static inline bool jitter_group_wide(bool base_aligned, long px, long HW) {
  return base_aligned && px + CJ_GROUP <= HW;
}

}  // namespace oibl
