// The device text the JPEG decoders share behind the parser: what one lane, one thread or one workgroup does in each
// stage, written once.  csrc/jpeg.hip wraps these bodies in two families of kernels that differ only in where an
// image's H, W and base pointers come from: for a batch of one stored size from kernel arguments and the image index,
// for a batch of mixed sizes from a per-image geometry table.  Its header comment says what the stages do.
#pragma once

#include "common.h"

#include "jpeg_chunked.h"

namespace oibl {

#define JPEG_DEV __device__ static __forceinline__

constexpr int JSCAN_MAX_LANES = 1024;

// ---- entropy, one lane per segment ----------------------------------------------------------------------------------
// Segment k of the image with geometry g (k < g.nseg checked by the caller's grid) into the image's coefficient slice.
JPEG_DEV void jpeg_entropy_lane(const uint8_t* bytes, uint32_t total_bytes, const JpegGeom& g, const int32_t* segs,
                                int S, const JpegHuff* s_huff, const uint8_t* s_zz, int k, int16_t* coef_image,
                                int32_t* seg_status) {
  if (k >= g.nseg || g.seg_first > S - 1 - k) return;   // no such segment, no slot for its status
  seg_status[g.seg_first + k] = jpeg_serial_segment(bytes, total_bytes, g, segs, S, s_huff, s_zz, k, coef_image);
}

// ---- entropy, one workgroup per segment (the schedule csrc/jpeg.hip describes) --------------------------------------
// Every thread of the workgroup calls it with the same k < g.nseg (g.seg_first <= S - 1 - k); T = blockDim.x, a power
// of two in [64, JSCAN_MAX_LANES].  s_huff and s_zz are built and a barrier lies behind them.
JPEG_DEV void jpeg_chunked_segment(const uint8_t* bytes, uint32_t total_bytes, const JpegGeom& g,
                                   const int32_t* segs, int chunk_bytes, const JpegHuff* s_huff, const uint8_t* s_zz,
                                   int k, int16_t* coef_image, int32_t* seg_status, int32_t* seg_rounds) {
  __shared__ uint32_t s_a[JSCAN_MAX_LANES], s_b[JSCAN_MAX_LANES], s_c[JSCAN_MAX_LANES], s_d[JSCAN_MAX_LANES];
  const int tid = threadIdx.x, T = blockDim.x;
  const int sidx = g.seg_first + k;
  const JpegChunkGeom q = jpeg_chunk_geom(g);
  const JpegChunkSeg sg = jpeg_chunk_segment(g, q, k, segs[2 * sidx], segs[2 * sidx + 1], total_bytes, chunk_bytes, T);
  const int L = sg.lanes;
  const bool mine = tid < L, last = tid == L - 1;
  const uint32_t start = sg.begin + (uint32_t)(mine ? tid : 0) * (uint32_t)chunk_bytes;
  const uint32_t limit = last ? 0xFFFFFFFFu : start + (uint32_t)chunk_bytes;

  // ---- speculate, settle ----
  JpegChunkState ent = jpeg_chunk_fresh(bytes, sg.begin, sg.end, start), ex = ent;
  JpegChunkSum sum = {0u, 0u, 0u, 0u};
  if (mine && !last) jpeg_chunk_speculate(bytes, sg.begin, sg.end, limit, q, s_huff, ent, ex, sum);
  int rounds = 0;
  for (int r = 0; r < L; ++r) {
    if (mine) s_a[tid] = ex.pos, s_b[tid] = ex.bcz;
    __syncthreads();
    int changed = 0;
    if (mine && tid > 0) {
      JpegChunkState e;
      e.pos = s_a[tid - 1], e.bcz = s_b[tid - 1];
      if (!jpeg_chunk_same(e, ent)) {
        ent = e, changed = 1;
        if (!last) jpeg_chunk_speculate(bytes, sg.begin, sg.end, limit, q, s_huff, ent, ex, sum);
      }
    }
    ++rounds;
    if (!__syncthreads_or(changed)) break;
  }

  // ---- scan: inclusive over the lanes, then one to the left ----
  if (!mine || last) sum.blocks = sum.dc0 = sum.dc1 = sum.dc2 = 0u;
  s_a[tid] = sum.blocks, s_b[tid] = sum.dc0, s_c[tid] = sum.dc1, s_d[tid] = sum.dc2;
  for (int off = 1; off < L; off <<= 1) {
    __syncthreads();
    uint32_t a = 0, b = 0, c = 0, d = 0;
    if (tid >= off) a = s_a[tid - off], b = s_b[tid - off], c = s_c[tid - off], d = s_d[tid - off];
    __syncthreads();
    s_a[tid] += a, s_b[tid] += b, s_c[tid] += c, s_d[tid] += d;
  }
  __syncthreads();
  uint32_t blk0 = 0, pred0 = 0, pred1 = 0, pred2 = 0;
  if (tid > 0) blk0 = s_a[tid - 1], pred0 = s_b[tid - 1], pred1 = s_c[tid - 1], pred2 = s_d[tid - 1];
  __syncthreads();

  // ---- write ----
  int st = JPEG_ST_OK;
  uint32_t at = 0;
  if (mine)
    st = jpeg_chunk_write(bytes, sg.begin, sg.end, total_bytes, limit, g, q, s_huff, s_zz, ent, blk0, pred0, pred1,
                          pred2, sg.first_mcu, sg.n_blocks, sg.expect_rst, tid == 0, coef_image, &at);
  s_a[tid] = st ? ((uint32_t)tid << 3 | (uint32_t)st) : 0xFFFFFFFFu;
  for (int half = T >> 1; half > 0; half >>= 1) {
    __syncthreads();
    if (tid < half) s_a[tid] = min(s_a[tid], s_a[tid + half]);
  }
  if (tid == 0) {
    seg_status[sidx] = s_a[0] == 0xFFFFFFFFu ? JPEG_ST_OK : (int32_t)(s_a[0] & 7u);
    seg_rounds[sidx] = rounds;
  }
}

// ---- IDCT -----------------------------------------------------------------------------------------------------------
// one pass of the IDCT over eight values; SHIFT = 11 (columns) or 18 (rows).  The sums are formed in unsigned
// arithmetic — the same bits as libjpeg's int32 wherever that does not overflow, and defined where a damaged stream
// makes it wrap — and descaled with an arithmetic shift.
template <int SHIFT>
JPEG_DEV void jpeg_idct8(int i0, int i1, int i2, int i3, int i4, int i5, int i6, int i7, int (&o)[8]) {
  typedef unsigned U;
  const U x0 = (U)i0, x1 = (U)i1, x2 = (U)i2, x3 = (U)i3, x4 = (U)i4, x5 = (U)i5, x6 = (U)i6, x7 = (U)i7;
  U z1 = (x2 + x6) * 4433u;
  const U t2 = z1 - x6 * 15137u, t3 = z1 + x2 * 6270u;
  const U t0 = (x0 + x4) << 13, t1 = (x0 - x4) << 13;
  const U t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  U u0 = x7, u1 = x5, u2 = x3, u3 = x1;
  z1 = u0 + u3;
  U z2 = u1 + u2, z3 = u0 + u2, z4 = u1 + u3;
  const U z5 = (z3 + z4) * 9633u;
  u0 *= 2446u, u1 *= 16819u, u2 *= 25172u, u3 *= 12299u;
  z1 *= (U)-7373, z2 *= (U)-20995;
  z3 = z3 * (U)-16069 + z5, z4 = z4 * (U)-3196 + z5;
  u0 += z1 + z3, u1 += z2 + z4, u2 += z2 + z3, u3 += z1 + z4;
  constexpr U R = 1u << (SHIFT - 1);
  o[0] = (int)(t10 + u3 + R) >> SHIFT, o[7] = (int)(t10 - u3 + R) >> SHIFT;
  o[1] = (int)(t11 + u2 + R) >> SHIFT, o[6] = (int)(t11 - u2 + R) >> SHIFT;
  o[2] = (int)(t12 + u1 + R) >> SHIFT, o[5] = (int)(t12 - u1 + R) >> SHIFT;
  o[3] = (int)(t13 + u0 + R) >> SHIFT, o[4] = (int)(t13 - u0 + R) >> SHIFT;
}

JPEG_DEV unsigned jpeg_clamp8(int v) { return (unsigned)min(max(v, 0), 255); }

// One thread, one 8 x 8 block: src[64] int16 (16-byte aligned) times the quantisation table s_q[64] through both
// passes, + 128, clamped, as eight 8-byte stores at dst, dst + Wp, ... with dst = plane + dst_at (8-byte aligned, Wp a
// multiple of 16; the address is formed behind the first pass, where it costs no registers).
JPEG_DEV void jpeg_idct_block(const int16_t* src, const int* s_q, uint8_t* plane, size_t dst_at, int Wp) {
  int x[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint4 w = reinterpret_cast<const uint4*>(src)[i];
    const unsigned u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[8 * i + 2 * j] = (int)(int16_t)(u[j] & 0xFFFFu) * s_q[8 * i + 2 * j];
      x[8 * i + 2 * j + 1] = (int)(int16_t)(u[j] >> 16) * s_q[8 * i + 2 * j + 1];
    }
  }
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    int o[8];
    jpeg_idct8<11>(x[col], x[8 + col], x[16 + col], x[24 + col], x[32 + col], x[40 + col], x[48 + col], x[56 + col],
                   o);
#pragma unroll
    for (int r = 0; r < 8; ++r) x[8 * r + col] = o[r];
  }
  uint8_t* dst = plane + dst_at;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int o[8];
    jpeg_idct8<18>(x[8 * r], x[8 * r + 1], x[8 * r + 2], x[8 * r + 3], x[8 * r + 4], x[8 * r + 5], x[8 * r + 6],
                   x[8 * r + 7], o);
    uint2 px;
    px.x = jpeg_clamp8(o[0] + 128) | jpeg_clamp8(o[1] + 128) << 8 | jpeg_clamp8(o[2] + 128) << 16 |
           jpeg_clamp8(o[3] + 128) << 24;
    px.y = jpeg_clamp8(o[4] + 128) | jpeg_clamp8(o[5] + 128) << 8 | jpeg_clamp8(o[6] + 128) << 16 |
           jpeg_clamp8(o[7] + 128) << 24;
    *reinterpret_cast<uint2*>(dst + (size_t)r * Wp) = px;
  }
}

// What the IDCT stage needs of an image's geometry for component c, as five scalars.  The stage takes these and
// jpeg_idct_plane takes the JpegGeom BY VALUE: handed on by reference, the struct stayed in scratch memory (84 bytes
// per lane in the compiler's report of this kernel, none this way).
struct JpegIdctPlane {
  int tq;               // the component's quantisation table
  int Bw, Bh;           // blocks across / down of the workspace's planes
  int bx_end, by_end;   // blocks across / down the component has: its share of the MCU grid
};

JPEG_DEV JpegIdctPlane jpeg_idct_plane(const JpegGeom g, int c) {
  JpegIdctPlane p;
  p.tq = c == 0 ? g.tq[0] : (c == 1 ? g.tq[1] : g.tq[2]);   // (a register select: no indexed array)
  p.Bw = g.Bw, p.Bh = g.Bh;
  p.bx_end = g.mcus_x * (c == 0 ? g.hs : 1), p.by_end = g.mcus_y * (c == 0 ? g.vs : 1);
  return p;
}

// The IDCT stage of one image: thread `blk` takes block blk of the plane of component c (< the image's components).
// rec: the image's record; coef_image / planes_image: its slices [3][Bh][Bw][64] int16 / uint8.  256 threads; every
// thread of the workgroup calls it (there is a barrier inside).
JPEG_DEV void jpeg_idct_stage(const uint8_t* rec, JpegIdctPlane p, int c, int blk, const int16_t* coef_image,
                              uint8_t* planes_image) {
  __shared__ int s_q[64];
  if (threadIdx.x < 64) s_q[threadIdx.x] = rec[JPEG_REC_QT + p.tq * 64 + threadIdx.x];
  __syncthreads();
  const int by = blk / p.Bw, bx = blk - by * p.Bw;
  if (bx >= p.bx_end || by >= p.by_end) return;
  const size_t plane = (size_t)p.Bw * p.Bh * 64;
  const int Wp = p.Bw * 8;
  jpeg_idct_block(coef_image + (size_t)c * plane + (size_t)blk * 64, s_q, planes_image + (size_t)c * plane,
                  (size_t)by * 8 * Wp + bx * 8, Wp);
}

// ---- upsampling and colour ------------------------------------------------------------------------------------------
// The chroma sample at output pixel (y, x) of a plane p with row stride Wp, cropped to ch x cw, replicated edges.
JPEG_DEV int jpeg_chroma(const uint8_t* p, int Wp, int cw, int ch, int hs, int vs, int y, int x) {
  if (hs == 1) return p[(size_t)y * Wp + x];
  const int c = x >> 1, side = (x & 1) ? min(c + 1, cw - 1) : max(c - 1, 0);
  if (vs == 1) {
    const uint8_t* row = p + (size_t)y * Wp;
    return (3 * row[c] + row[side] + 1 + (x & 1)) >> 2;
  }
  const int r = y >> 1, nb = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
  const uint8_t *row = p + (size_t)r * Wp, *other = p + (size_t)nb * Wp;
  const int t = 3 * row[c] + other[c], ts = 3 * row[side] + other[side];
  return (3 * t + ts + 8 - (x & 1)) >> 4;
}

// Pixel (y, x), y < H, x < W, of the image whose planes start at py: three bytes at o.
JPEG_DEV void jpeg_colour_pixel(const JpegGeom& g, const uint8_t* py, int H, int W, int y, int x, uint8_t* o) {
  const int Wp = g.Bw * 8;
  const size_t plane = (size_t)g.Bw * g.Bh * 64;
  const int Y = py[(size_t)y * Wp + x];
  int R = Y, G = Y, B = Y;
  if (g.ncomp == 3) {
    const int cw = (W + g.hs - 1) / g.hs, ch = (H + g.vs - 1) / g.vs;
    const int cb = jpeg_chroma(py + plane, Wp, cw, ch, g.hs, g.vs, y, x) - 128;
    const int cr = jpeg_chroma(py + 2 * plane, Wp, cw, ch, g.hs, g.vs, y, x) - 128;
    R = (int)jpeg_clamp8(Y + ((91881 * cr + 32768) >> 16));
    G = (int)jpeg_clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    B = (int)jpeg_clamp8(Y + ((116130 * cb + 32768) >> 16));
  }
  o[0] = (uint8_t)R, o[1] = (uint8_t)G, o[2] = (uint8_t)B;
}

// The image's status by one workgroup of (64, 4) threads, all of which call it: the largest of its segments', or the
// host's.
JPEG_DEV void jpeg_image_status(const JpegGeom& g, const int32_t* seg_status, int S, int* s_max, int32_t* status_n) {
  const int tid = threadIdx.y * 64 + threadIdx.x;
  int m = 0;
  for (int k = tid; k < g.nseg && g.seg_first <= S - 1 - k; k += 256) m = max(m, seg_status[g.seg_first + k]);
  m = max(m, __shfl_xor(m, 32, 64));
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
  if (threadIdx.x == 0) s_max[threadIdx.y] = m;
  __syncthreads();
  if (tid == 0) *status_n = g.host_status ? g.host_status : max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
}

}  // namespace oibl
