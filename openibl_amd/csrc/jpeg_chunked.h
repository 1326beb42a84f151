// Parallel entropy decoding inside one segment (a restart-free scan, or a long restart interval) by self-synchronising
// Huffman decoding: the chunk state machine of csrc/jpeg.hip on top         of jpeg_entropy.h.  Like that file it is
// compiled into the kernel and, without hipcc, into a host program (tests/helpers/jpeg_chunked_harness.cpp).
//
// A segment bytes[begin, end) is cut into chunks of `chunk_bytes` raw bytes, one lane each.  The decoder's state at a
// symbol boundary is JpegChunkState: where the next bit stands, the block-in-MCU index c and the zig-zag position z
// (z = 0: a DC symbol is next).  A symbol is a Huffman code with the extra bits behind it; it belongs to the chunk
// its first bit stands in.
//
//   jpeg_chunk_fresh      the guess a lane starts from: its chunk's first bit, c = 0, z = 0
//   jpeg_chunk_speculate  decode from an entry without writing, up to the first symbol that starts at or behind
//                         `limit`; reports the exit state and what the chunk owns (DC symbols, DC sums per component).
//                         Tolerant: a code no length matches skips one bit, a coefficient index above 63 ends the
//                         block — the rule changes how many rounds the settle phase takes, never the result.
//   jpeg_chunk_write      decode from the final entry once more, strictly, and write absolute coefficients; the same
//                         events are JPEG_ST_BAD_CODE / JPEG_ST_OVERRUN, and the lane that completes the segment
//                         makes the checks jpeg_decode_segment makes behind its last MCU.
//
// Positions.  A byte at raw index j is stuffing exactly when b[j] == 0, j > begin and b[j - 1] == 0xFF (what
// jpeg_bits_fill skips); the rule is local, so a lane can start anywhere.  The position handed from lane to lane is
// canonical — the raw index of the data byte that holds the next bit, and the bit within it — and does not depend on
// how far the reader had prefetched.  Indices at or behind `end` are the virtual zero bytes of JpegBits::over.
//
// Bounds by construction, whatever the bytes say:
//   - every loop step consumes at least one bit, and a lane with a limit stops at it: at most 8 * (limit - entry)
//     steps, and a few virtual bytes behind the end; the writing lane without a limit stops with the segment's blocks,
//     at the first status, or at the end of the MCU that used virtual bytes;
//   - a write goes to block * 64 + k with k <= 63 and the block index, taken from the prefix over the chunks, checked
//     against the segment's block count first, so the block lies inside the segment's MCUs and those inside the grid;
//   - no array is indexed by a decoded value except the masked Huffman values and the 64-entry zig-zag table.
#pragma once

#include "jpeg_entropy.h"

struct JpegChunkState {
  uint32_t pos;   // raw index of the byte that holds the next bit (never a stuffing byte; >= end: virtual)
  uint32_t bcz;   // bit within it (0 = the top one) | c << 3 | z << 6
};

struct JpegChunkSum {
  uint32_t blocks;             // DC symbols the chunk owns
  uint32_t dc0, dc1, dc2;      // their differences summed per component, unsigned as jpeg_decode_block sums them
};

JPEG_HD static inline uint32_t jpeg_chunk_pack(int bit, int c, int z) { return (uint32_t)(bit | c << 3 | z << 6); }
JPEG_HD static inline bool jpeg_chunk_same(const JpegChunkState& a, const JpegChunkState& b) {
  return a.pos == b.pos && a.bcz == b.bcz;
}

// what the geometry means for the order of blocks inside an MCU
struct JpegChunkGeom {
  int bpm, luma;      // blocks per MCU; how many of them are luma
  uint32_t td, ta;    // bit comp: the component's DC / AC table
};

JPEG_HD static inline JpegChunkGeom jpeg_chunk_geom(const JpegGeom& g) {
  JpegChunkGeom q;
  q.luma = g.hs * g.vs;
  q.bpm = g.ncomp == 3 ? q.luma + 2 : 1;
  q.td = (uint32_t)(g.td[0] | g.td[1] << 1 | g.td[2] << 2);
  q.ta = (uint32_t)(g.ta[0] | g.ta[1] << 1 | g.ta[2] << 2);
  return q;
}

JPEG_HD static inline bool jpeg_is_stuffing(const uint8_t* p, uint32_t j, uint32_t begin, uint32_t end) {
  return j > begin && j < end && p[j] == 0 && p[j - 1] == 0xFF;
}

// a reader at a canonical position
JPEG_HD static inline void jpeg_chunk_open(JpegBits& b, const uint8_t* p, uint32_t end, const JpegChunkState& s) {
  jpeg_bits_init(b, p, s.pos, end);
  b.over = s.pos > end ? (int)(s.pos - end) : 0;
  const int bit = (int)(s.bcz & 7);
  if (bit) {
    jpeg_bits_fill(b);
    jpeg_bits_skip(b, bit);
  }
}

// the canonical position of the reader's next bit: back from the next byte to load over the unread data bytes
JPEG_HD static inline void jpeg_chunk_where(const JpegBits& b, uint32_t begin, uint32_t& pos, int& bit) {
  uint32_t j = b.pos + (uint32_t)b.over;
  for (int n = b.nbits; n > 0; n -= 8) {
    --j;
    if (jpeg_is_stuffing(b.p, j, begin, b.end)) --j;
  }
  pos = j, bit = (8 - (b.nbits & 7)) & 7;
}

// does the next symbol start at or behind raw index `limit`?  (the bytes in the buffer lie in front of the next byte
// to load: while that one is not behind the limit, nothing else is)
JPEG_HD static inline bool jpeg_chunk_reached(const JpegBits& b, uint32_t begin, uint32_t limit) {
  if (b.nbits > 0 && b.pos + (uint32_t)b.over <= limit) return false;
  uint32_t pos;
  int bit;
  jpeg_chunk_where(b, begin, pos, bit);
  return pos >= limit;
}

// the entry lane `lane` guesses: the first bit of its chunk (one byte later if the chunk begins on a stuffing byte);
// lane 0's is the segment's true entry
JPEG_HD static inline JpegChunkState jpeg_chunk_fresh(const uint8_t* p, uint32_t begin, uint32_t end, uint32_t start) {
  JpegChunkState s;
  s.pos = start + (jpeg_is_stuffing(p, start, begin, end) ? 1u : 0u);
  s.bcz = 0;
  return s;
}

JPEG_HD static inline void jpeg_chunk_speculate(const uint8_t* bytes, uint32_t begin, uint32_t end, uint32_t limit,
                                                const JpegChunkGeom& q, const JpegHuff* huff,
                                                const JpegChunkState& in, JpegChunkState& out, JpegChunkSum& sum) {
  JpegBits b;
  jpeg_chunk_open(b, bytes, end, in);
  int c = (int)(in.bcz >> 3 & 7), z = (int)(in.bcz >> 6 & 63);
  if (c >= q.bpm) c = 0;
  sum.blocks = sum.dc0 = sum.dc1 = sum.dc2 = 0;
  while (!jpeg_chunk_reached(b, begin, limit)) {
    const int comp = c < q.luma ? 0 : c - q.luma + 1;
    if (z == 0) {
      const int s = jpeg_huff_decode(b, huff + (q.td >> comp & 1));
      if (s < 0) {
        jpeg_bits_skip(b, 1);
        continue;
      }
      const uint32_t d = (uint32_t)jpeg_receive_extend(b, s & 15);
      ++sum.blocks;
      sum.dc0 += comp == 0 ? d : 0u, sum.dc1 += comp == 1 ? d : 0u, sum.dc2 += comp == 2 ? d : 0u;
      z = 1;
      continue;
    }
    const int rs = jpeg_huff_decode(b, huff + 2 + (q.ta >> comp & 1));
    if (rs < 0) {
      jpeg_bits_skip(b, 1);
      continue;
    }
    const int r = rs >> 4, s = rs & 15;
    if (s == 0) {
      z = r == 15 ? z + 16 : 64;
    } else {
      z += r;
      if (z <= 63) {
        jpeg_receive_extend(b, s);
        ++z;
      }
    }
    if (z >= 64) z = 0, c = c + 1 == q.bpm ? 0 : c + 1;
  }
  int bit;
  jpeg_chunk_where(b, begin, out.pos, bit);
  out.bcz = jpeg_chunk_pack(bit, c, z);
}

// The checks jpeg_decode_segment makes behind its last MCU, at the canonical position of the next bit: fewer than
// eight bits of the segment are left, and the restart marker stands behind it.
JPEG_HD static inline int jpeg_chunk_finish(const JpegBits& b, uint32_t begin, uint32_t total_bytes, int expect_rst) {
  const uint32_t end = b.end;
  uint32_t pos;
  int bit;
  jpeg_chunk_where(b, begin, pos, bit);
  if (pos < end) {
    const uint32_t next = pos + 1 + (jpeg_is_stuffing(b.p, pos + 1, begin, end) ? 1u : 0u);
    if (bit == 0 || next < end) return JPEG_ST_BAD_RESTART;
  }
  if (expect_rst >= 0 && !(end + 2 <= total_bytes && end + 2 > end && b.p[end] == 0xFF &&
                           b.p[end + 1] == 0xD0 + (expect_rst & 7)))
    return JPEG_ST_BAD_RESTART;
  return JPEG_ST_OK;
}

// the block with scan-order index cur of a segment that starts at MCU first_mcu (cur < the segment's blocks)
JPEG_HD static inline int16_t* jpeg_chunk_block(int16_t* coef, const JpegGeom& g, const JpegChunkGeom& q, int first_mcu,
                                                uint32_t cur, int& c) {
  const int m = first_mcu + (int)(cur / (uint32_t)q.bpm);
  c = (int)(cur % (uint32_t)q.bpm);
  const int my = m / g.mcus_x, mx = m - my * g.mcus_x;
  const size_t plane = (size_t)g.Bw * g.Bh * 64;
  if (c < q.luma) {
    const int v = g.hs == 2 ? c >> 1 : c, h = g.hs == 2 ? c & 1 : 0;
    return coef + ((size_t)(my * g.vs + v) * g.Bw + (mx * g.hs + h)) * 64;
  }
  return coef + (size_t)(c - q.luma + 1) * plane + ((size_t)my * g.Bw + mx) * 64;
}

// The strict pass of one lane.  in: its final entry; blk0 and pred0..2: the prefix over the chunks in front of it (DC
// symbols, DC sums); n_blocks: the segment's blocks; limit: the next chunk's first byte, 0xFFFFFFFF for the last
// lane; first_lane: lane 0, which completes a segment of no blocks.  Returns the lane's status; *at: the scan-order
// index of the block it stood in when it reported one (n_blocks for the checks behind the last block).
JPEG_HD static inline int jpeg_chunk_write(const uint8_t* bytes, uint32_t begin, uint32_t end, uint32_t total_bytes,
                                           uint32_t limit, const JpegGeom& g, const JpegChunkGeom& q,
                                           const JpegHuff* huff, const uint8_t* zz, const JpegChunkState& in,
                                           uint32_t blk0, uint32_t pred0, uint32_t pred1, uint32_t pred2,
                                           int first_mcu, uint32_t n_blocks, int expect_rst, bool first_lane,
                                           int16_t* coef, uint32_t* at) {
  JpegBits b;
  jpeg_chunk_open(b, bytes, end, in);
  int z = (int)(in.bcz >> 6 & 63);
  if (z > 0 && blk0 == 0) return JPEG_ST_OK;   // (only behind damage: a block nobody began)
  uint32_t cur = z > 0 ? blk0 - 1 : blk0;
  *at = cur < n_blocks ? cur : n_blocks;
  if (cur >= n_blocks) return first_lane && n_blocks == 0 ? jpeg_chunk_finish(b, begin, total_bytes, expect_rst)
                                                          : JPEG_ST_OK;
  int c;
  int16_t* out = jpeg_chunk_block(coef, g, q, first_mcu, cur, c);
  while (!jpeg_chunk_reached(b, begin, limit)) {
    const int comp = c < q.luma ? 0 : c - q.luma + 1;
    if (z == 0) {
      const int s = jpeg_huff_decode(b, huff + (q.td >> comp & 1));
      if (s < 0 || s > 15) return JPEG_ST_BAD_CODE;
      const uint32_t d = (uint32_t)jpeg_receive_extend(b, s);
      pred0 += comp == 0 ? d : 0u, pred1 += comp == 1 ? d : 0u, pred2 += comp == 2 ? d : 0u;
      out[0] = (int16_t)(int)(comp == 0 ? pred0 : (comp == 1 ? pred1 : pred2));
      z = 1;
      continue;
    }
    const int rs = jpeg_huff_decode(b, huff + 2 + (q.ta >> comp & 1));
    if (rs < 0) return JPEG_ST_BAD_CODE;
    const int r = rs >> 4, s = rs & 15;
    if (s == 0) {
      z = r == 15 ? z + 16 : 64;
    } else {
      z += r;
      if (z > 63) return JPEG_ST_OVERRUN;
      out[zz[z & 63]] = (int16_t)jpeg_receive_extend(b, s);
      ++z;
    }
    if (z < 64) continue;
    z = 0, ++cur;   // the block is done
    if (c + 1 == q.bpm && jpeg_bits_real(b) < 0) return JPEG_ST_OUT_OF_BYTES;   // (the end of an MCU)
    *at = cur;
    if (cur == n_blocks) return jpeg_chunk_finish(b, begin, total_bytes, expect_rst);
    out = jpeg_chunk_block(coef, g, q, first_mcu, cur, c);
  }
  return JPEG_ST_OK;
}

// ---- the segment as the workgroup sees it ---------------------------------------------------------------------------
struct JpegChunkSeg {
  uint32_t begin, end;   // clamped to the buffer
  int first_mcu, expect_rst;
  uint32_t n_blocks;
  int lanes;             // chunks, at most max_lanes: the last lane takes the remainder
};

JPEG_HD static inline JpegChunkSeg jpeg_chunk_segment(const JpegGeom& g, const JpegChunkGeom& q, int k, int32_t sb,
                                                      int32_t se, uint32_t total_bytes, int chunk_bytes,
                                                      int max_lanes) {
  JpegChunkSeg s;
  s.end = se > 0 ? (uint32_t)se : 0u;
  if (s.end > total_bytes) s.end = total_bytes;
  s.begin = sb > 0 ? (uint32_t)sb : 0u;
  if (s.begin > s.end) s.begin = s.end;
  const int total = g.mcus_x * g.mcus_y;
  const int want = jpeg_segments_wanted(total, g.dri);
  long long first = g.dri ? (long long)k * g.dri : 0;   // as jpeg_decode_segment clamps them
  if (first > total) first = total;
  int n_mcu = g.dri ? g.dri : total;
  if (n_mcu > total - (int)first) n_mcu = total - (int)first;
  s.first_mcu = (int)first;
  s.n_blocks = (uint32_t)n_mcu * (uint32_t)q.bpm;
  s.expect_rst = (g.dri && k + 1 < want) ? (k & 7) : -1;
  const uint32_t len = s.end - s.begin, cb = (uint32_t)chunk_bytes;
  const uint32_t chunks = len / cb + (len % cb != 0);
  s.lanes = chunks < 1 ? 1 : (chunks > (uint32_t)max_lanes ? max_lanes : (int)chunks);
  return s;
}
