// The workgroup of jpeg_chunked_segment (openibl_amd/csrc/jpeg_stages.h) on the host, for the harnesses that run the
// chunk state machine of jpeg_chunked.h under the host sanitizers: per phase a loop over the lanes, with a snapshot of
// the exit table where the kernel has the barrier between writing and reading it.  The lane tables have the kernel's
// 1024 entries on the heap, so that a lane count above it ends the run like any other access outside a buffer.
#pragma once

#include <algorithm>
#include <vector>

#include "jpeg_chunked.h"

static const int kMaxLanes = 1024;   // JSCAN_MAX_LANES

struct JpegEmulSegment {
  int status;        // of the first lane in scan order that reports one
  int rounds, lanes;
  int32_t damaged;   // the scan-order index inside the segment of the block at which that lane reported it, -1 if none
};

// Segment k of the image with geometry g as its workgroup decodes it, into the image's coefficient slice; a k the
// image or the table segs[S][2] does not have is left alone, as the kernels leave it.
static JpegEmulSegment jpeg_emul_chunked_segment(const uint8_t* bytes, uint32_t total_bytes, const JpegGeom& g,
                                                 const int32_t* segs, int S, const JpegHuff* huff, const uint8_t* zz,
                                                 int chunk_bytes, int k, int16_t* coef_image) {
  JpegEmulSegment res = {0, 0, 0, -1};
  if (k >= g.nseg || g.seg_first > S - 1 - k) return res;
  const int sidx = g.seg_first + k;
  const JpegChunkGeom q = jpeg_chunk_geom(g);
  const JpegChunkSeg sg =
      jpeg_chunk_segment(g, q, k, segs[2 * sidx], segs[2 * sidx + 1], total_bytes, chunk_bytes, kMaxLanes);
  const int L = res.lanes = sg.lanes;
  // the kernel's s_a .. s_d, the snapshot the barrier makes of s_a / s_b, the lanes' registers
  std::vector<JpegChunkState> ent(kMaxLanes), ex(kMaxLanes), seen(kMaxLanes);
  std::vector<JpegChunkSum> sum(kMaxLanes);
  std::vector<uint32_t> limit(kMaxLanes);
  for (int t = 0; t < L; ++t) {
    const uint32_t start = sg.begin + (uint32_t)t * (uint32_t)chunk_bytes;
    limit[t] = t == L - 1 ? 0xFFFFFFFFu : start + (uint32_t)chunk_bytes;
    ent[t] = ex[t] = jpeg_chunk_fresh(bytes, sg.begin, sg.end, start);
    sum[t] = JpegChunkSum{0u, 0u, 0u, 0u};
    if (t < L - 1) jpeg_chunk_speculate(bytes, sg.begin, sg.end, limit[t], q, huff, ent[t], ex[t], sum[t]);
  }
  for (int r = 0; r < L; ++r) {
    std::copy(ex.begin(), ex.begin() + L, seen.begin());   // the barrier
    int changed = 0;
    for (int t = 1; t < L; ++t) {
      if (jpeg_chunk_same(seen[t - 1], ent[t])) continue;
      ent[t] = seen[t - 1], changed = 1;
      if (t < L - 1) jpeg_chunk_speculate(bytes, sg.begin, sg.end, limit[t], q, huff, ent[t], ex[t], sum[t]);
    }
    ++res.rounds;
    if (!changed) break;
  }
  uint32_t blk0 = 0, p0 = 0, p1 = 0, p2 = 0;
  for (int t = 0; t < L; ++t) {   // (every lane writes, as on the device; the first status in scan order counts)
    uint32_t at = 0;
    const int st = jpeg_chunk_write(bytes, sg.begin, sg.end, total_bytes, limit[t], g, q, huff, zz, ent[t], blk0, p0,
                                    p1, p2, sg.first_mcu, sg.n_blocks, sg.expect_rst, t == 0, coef_image, &at);
    if (st && !res.status) res.status = st, res.damaged = (int32_t)at;
    if (t < L - 1) blk0 += sum[t].blocks, p0 += sum[t].dc0, p1 += sum[t].dc1, p2 += sum[t].dc2;
  }
  return res;
}
