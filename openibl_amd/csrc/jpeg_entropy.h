// Entropy decoding of a baseline JPEG scan (T.81 F.2.2): the bit reader, the Huffman tables and the block / segment
// decoder of csrc/jpeg.hip.  The same text is compiled into the kernel and, without hipcc, into a host program
// (tests/helpers/jpeg_entropy_harness.cpp) that runs it under the host sanitizers: JPEG_HD is
// `__host__ __device__` under hipcc and empty otherwise, and nothing here needs a HIP header.
//
// Bounds by construction, whatever the bytes say:
//   - every byte read is checked against the segment's end (which the caller clamps to the buffer); past it the reader
//     yields zero bits and counts them, and a segment that used such bits ends with JPEG_ST_OUT_OF_BYTES;
//   - a Huffman value is read at an index masked to the 256-entry value array; a code no length matches ends the
//     segment with JPEG_ST_BAD_CODE;
//   - a coefficient index above 63 ends the segment with JPEG_ST_OVERRUN before anything is written;
//   - the segment's loop runs over at most `n_mcu` MCUs, every one of them inside the image's MCU grid, and each block
//     consumes at least one bit-reader step per coefficient, at most 64;
//   - every write is at block * 64 + k with k <= 63 and the block inside the component's MCU-padded plane.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__
#else
#define JPEG_HD
#endif

// per-image status (include/openibl_amd.h documents them)
#define JPEG_ST_OK 0
#define JPEG_ST_BAD_CODE 1
#define JPEG_ST_OVERRUN 2
#define JPEG_ST_OUT_OF_BYTES 3
#define JPEG_ST_BAD_RESTART 4

// zig-zag position -> natural (row-major) index
#define JPEG_ZIGZAG_LIST                                                                                              \
  0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, \
      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, \
      47, 55, 62, 63

// ---- the per-image record (the layout include/openibl_amd.h documents) ----------------------------------------------
#define JPEG_REC_BYTES 1408
#define JPEG_REC_QT 64           // uint8 qt[4][64], natural order
#define JPEG_REC_HUFF 320        // uint8 huff[4][272]: DC 0, DC 1, AC 0, AC 1; each counts[16] then values[256]
#define JPEG_HUFF_BYTES 272
enum {
  JPEG_H_NCOMP = 0, JPEG_H_HS, JPEG_H_VS, JPEG_H_TQ0, JPEG_H_TQ1, JPEG_H_TQ2, JPEG_H_TD0, JPEG_H_TD1, JPEG_H_TD2,
  JPEG_H_TA0, JPEG_H_TA1, JPEG_H_TA2, JPEG_H_DRI, JPEG_H_SEG_FIRST, JPEG_H_NSEG, JPEG_H_STATUS
};

// What the three stages derive from a record's header and the batch's H x W; every field is forced into its valid
// range, so a damaged record cannot index outside anything.
struct JpegGeom {
  int ncomp;           // 1 or 3
  int hs, vs;          // luma sampling factors: (1,1), (2,1) or (2,2); chroma is (1,1)
  int mcus_x, mcus_y;  // the MCU grid
  int Bw, Bh;          // blocks across / down of the workspace's planes: 2 ceil(W / 16), 2 ceil(H / 16)
  int tq[3], td[3], ta[3];
  int dri, seg_first, nseg, host_status;
};

JPEG_HD static inline int jpeg_blocks_across(int W) { return 2 * ((W + 15) / 16); }

// segments of an image of `total` MCUs with restart interval dri (0: none): ceil(total / dri), without forming
// total + dri (a record may hold any 32-bit interval)
JPEG_HD static inline int jpeg_segments_wanted(int total, int dri) {
  return dri > 0 ? total / dri + (total % dri != 0) : 1;
}

JPEG_HD static inline JpegGeom jpeg_geom(const int32_t* hdr, int H, int W) {
  JpegGeom g;
  g.ncomp = hdr[JPEG_H_NCOMP] == 3 ? 3 : 1;
  g.hs = (g.ncomp == 3 && hdr[JPEG_H_HS] == 2) ? 2 : 1;
  g.vs = (g.hs == 2 && hdr[JPEG_H_VS] == 2) ? 2 : 1;
  g.mcus_x = (W + 8 * g.hs - 1) / (8 * g.hs);
  g.mcus_y = (H + 8 * g.vs - 1) / (8 * g.vs);
  g.Bw = jpeg_blocks_across(W);
  g.Bh = jpeg_blocks_across(H);
  for (int c = 0; c < 3; ++c) {
    g.tq[c] = hdr[JPEG_H_TQ0 + c] & 3;
    g.td[c] = hdr[JPEG_H_TD0 + c] & 1;
    g.ta[c] = hdr[JPEG_H_TA0 + c] & 1;
  }
  const int total = g.mcus_x * g.mcus_y;   // <= 4096 * 4096
  g.dri = hdr[JPEG_H_DRI] > 0 ? hdr[JPEG_H_DRI] : 0;
  const int want = jpeg_segments_wanted(total, g.dri);
  g.seg_first = hdr[JPEG_H_SEG_FIRST] > 0 ? hdr[JPEG_H_SEG_FIRST] : 0;
  g.nseg = hdr[JPEG_H_NSEG] < 0 ? 0 : (hdr[JPEG_H_NSEG] > want ? want : hdr[JPEG_H_NSEG]);
  g.host_status = hdr[JPEG_H_STATUS];
  return g;
}

// ---- bits ---------------------------------------------------------------------------------------------------------
struct JpegBits {
  const uint8_t* p;
  uint32_t pos, end;   // next byte, one past the segment's last byte
  uint32_t buf;        // the next `nbits` bits, from the top
  int nbits;
  int over;            // zero bytes appended behind the segment's end
};

JPEG_HD static inline void jpeg_bits_init(JpegBits& b, const uint8_t* p, uint32_t begin, uint32_t end) {
  b.p = p, b.pos = begin < end ? begin : end, b.end = end, b.buf = 0, b.nbits = 0, b.over = 0;
}

// at least 25 bits afterwards; FF 00 is the data byte FF.  One byte per load: an aligned eight-byte window in front of
// the loads was measured and was slower (profiles/jpeg_decode_bench_window.txt: 29.1 against 26.6 ms per restart-free
// 480 x 640 scan) — a lane is bound by its dependent chain of table look-ups and shifts, not by the loads.
JPEG_HD static inline void jpeg_bits_fill(JpegBits& b) {
  while (b.nbits <= 24) {
    uint32_t byte = 0;
    if (b.pos < b.end) {
      byte = b.p[b.pos++];
      if (byte == 0xFF && b.pos < b.end && b.p[b.pos] == 0) ++b.pos;
    } else {
      ++b.over;
    }
    b.buf |= byte << (24 - b.nbits);
    b.nbits += 8;
  }
}
JPEG_HD static inline uint32_t jpeg_bits_peek(const JpegBits& b, int n) { return b.buf >> (32 - n); }   // 1 <= n <= 16
JPEG_HD static inline void jpeg_bits_skip(JpegBits& b, int n) { b.buf <<= n, b.nbits -= n; }
// bits of the segment itself that are still unread in the buffer; negative: bits from behind its end were used
JPEG_HD static inline int jpeg_bits_real(const JpegBits& b) { return b.nbits - 8 * b.over; }

// ---- Huffman tables -------------------------------------------------------------------------------------------------
struct JpegHuff {
  uint16_t look[256];    // by the next 8 bits: length << 8 | value for codes of up to 8 bits, 0 otherwise
  int32_t maxcode[17];   // [l]: the largest code of length l, -1 if there is none
  int32_t valoff[17];    // [l]: index of the first value of length l minus its first code
  uint8_t vals[256];
};

// counts_values: counts[16] then values[256] (a record's table)
JPEG_HD static inline void jpeg_huff_build(JpegHuff* t, const uint8_t* counts_values) {
  for (int i = 0; i < 256; ++i) t->look[i] = 0, t->vals[i] = counts_values[16 + i];
  int code = 0, k = 0;
  t->maxcode[0] = -1, t->valoff[0] = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = counts_values[l - 1];
    t->valoff[l] = k - code;
    for (int j = 0; j < n; ++j, ++code, ++k) {
      if (l > 8 || k >= 256) continue;
      const int first = code << (8 - l), span = 1 << (8 - l);
      for (int i = first; i < first + span && i < 256; ++i) t->look[i] = (uint16_t)((l << 8) | t->vals[k]);
    }
    t->maxcode[l] = n ? code - 1 : -1;
    code <<= 1;
  }
}

// the next symbol, or -1 if no code matches
JPEG_HD static inline int jpeg_huff_decode(JpegBits& b, const JpegHuff* t) {
  jpeg_bits_fill(b);
  const uint32_t e = t->look[jpeg_bits_peek(b, 8)];
  if (e) {
    jpeg_bits_skip(b, (int)(e >> 8));
    return (int)(e & 255);
  }
  const int code16 = (int)jpeg_bits_peek(b, 16);
  for (int l = 9; l <= 16; ++l) {
    const int code = code16 >> (16 - l);
    if (code <= t->maxcode[l]) {
      jpeg_bits_skip(b, l);
      return t->vals[(code + t->valoff[l]) & 255];
    }
  }
  return -1;
}

// s more bits as the signed value of T.81's EXTEND; 0 <= s <= 15
JPEG_HD static inline int jpeg_receive_extend(JpegBits& b, int s) {
  if (s == 0) return 0;
  jpeg_bits_fill(b);
  const int v = (int)jpeg_bits_peek(b, s);
  jpeg_bits_skip(b, s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block into out[64] (natural order, zeroed by the caller); zz: zig-zag position -> natural index.
JPEG_HD static inline int jpeg_decode_block(JpegBits& b, const JpegHuff* dc, const JpegHuff* ac, const uint8_t* zz,
                                            int& pred, int16_t* out) {
  int s = jpeg_huff_decode(b, dc);
  if (s < 0 || s > 15) return JPEG_ST_BAD_CODE;
  pred = (int)((unsigned)pred + (unsigned)jpeg_receive_extend(b, s));   // (a damaged stream may wrap: no signed overflow)
  out[0] = (int16_t)pred;
  for (int k = 1; k < 64;) {
    const int rs = jpeg_huff_decode(b, ac);
    if (rs < 0) return JPEG_ST_BAD_CODE;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;   // EOB
      k += 16;              // ZRL
      continue;
    }
    k += r;
    if (k > 63) return JPEG_ST_OVERRUN;
    out[zz[k & 63]] = (int16_t)jpeg_receive_extend(b, s);
    ++k;
  }
  return JPEG_ST_OK;
}

// One segment (a restart interval, or the whole scan): MCUs [first_mcu, first_mcu + n_mcu) of the image, clipped to
// its MCU grid, into the image's coefficient slice coef[3][Bh][Bw][64].  bytes[begin, end) is the segment;
// total_bytes bounds both.  expect_rst: 0..7 if the marker FF D0+expect_rst must stand at `end`, -1 for the last
// segment.  huff: the record's four tables, built (DC 0, DC 1, AC 0, AC 1).
JPEG_HD static inline int jpeg_decode_segment(const uint8_t* bytes, uint32_t begin, uint32_t end, uint32_t total_bytes,
                                              const JpegGeom& g, const JpegHuff* huff, const uint8_t* zz,
                                              int first_mcu, int n_mcu, int expect_rst, int16_t* coef) {
  if (end > total_bytes) end = total_bytes;
  JpegBits b;
  jpeg_bits_init(b, bytes, begin, end);
  const int total = g.mcus_x * g.mcus_y;
  if (first_mcu < 0) first_mcu = 0;
  if (first_mcu > total) first_mcu = total;
  if (n_mcu < 0 || n_mcu > total - first_mcu) n_mcu = total - first_mcu;
  const int last = first_mcu + n_mcu;
  const size_t plane = (size_t)g.Bw * g.Bh * 64;
  int pred0 = 0, pred1 = 0, pred2 = 0;
  for (int m = first_mcu; m < last; ++m) {
    const int my = m / g.mcus_x, mx = m - my * g.mcus_x;
    for (int v = 0; v < g.vs; ++v)
      for (int h = 0; h < g.hs; ++h) {
        int16_t* out = coef + ((size_t)(my * g.vs + v) * g.Bw + (mx * g.hs + h)) * 64;
        const int st = jpeg_decode_block(b, huff + g.td[0], huff + 2 + g.ta[0], zz, pred0, out);
        if (st) return st;
      }
    if (g.ncomp == 3) {
      int16_t* out = coef + plane + ((size_t)my * g.Bw + mx) * 64;
      int st = jpeg_decode_block(b, huff + g.td[1], huff + 2 + g.ta[1], zz, pred1, out);
      if (st) return st;
      st = jpeg_decode_block(b, huff + g.td[2], huff + 2 + g.ta[2], zz, pred2, out + plane);
      if (st) return st;
    }
    if (jpeg_bits_real(b) < 0) return JPEG_ST_OUT_OF_BYTES;
  }
  // discard to the byte boundary: the segment's bytes must all be used, and its marker must stand behind them
  const int real = jpeg_bits_real(b);
  if (b.pos != b.end || real >= 8) return JPEG_ST_BAD_RESTART;
  if (expect_rst >= 0 &&
      !(end + 2 <= total_bytes && end + 2 > end && bytes[end] == 0xFF && bytes[end + 1] == 0xD0 + (expect_rst & 7)))
    return JPEG_ST_BAD_RESTART;
  return JPEG_ST_OK;
}

// Segment k of the image with geometry g as the serial route decodes it: row g.seg_first + k of the batch's segment
// table segs[S][2], clamped at 0, the MCUs of restart interval k (all of them without restarts) and the marker that
// must follow.  Returns the segment's status; JPEG_ST_OK, with nothing read or written, for a k the image or the
// table does not have.
JPEG_HD static inline int jpeg_serial_segment(const uint8_t* bytes, uint32_t total_bytes, const JpegGeom& g,
                                              const int32_t* segs, int S, const JpegHuff* huff, const uint8_t* zz,
                                              int k, int16_t* coef_image) {
  if (k >= g.nseg || g.seg_first > S - 1 - k) return JPEG_ST_OK;
  const int sidx = g.seg_first + k;
  const int total = g.mcus_x * g.mcus_y;
  const int want = jpeg_segments_wanted(total, g.dri);
  const int32_t sb = segs[2 * sidx], se = segs[2 * sidx + 1];
  const uint32_t begin = sb > 0 ? (uint32_t)sb : 0u, end = se > 0 ? (uint32_t)se : 0u;
  return jpeg_decode_segment(bytes, begin, end, total_bytes, g, huff, zz, g.dri ? k * g.dri : 0,
                             g.dri ? g.dri : total, (g.dri && k + 1 < want) ? (k & 7) : -1, coef_image);
}
