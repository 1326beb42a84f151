// Host harness of openibl_amd/csrc/jpeg_chunked.h: the chunk state machine of jscan_chunk_kernel, compiled without
// hipcc into a program of its own so that it can run under the host sanitizers (tests/test_jpeg_chunked_cpu.py builds
// it with -fsanitize=address,undefined).  It emulates the workgroup: per segment a loop over the lanes for each phase,
// with a snapshot of the exit table where the kernel has the barrier between writing and reading it, on heap buffers
// of exactly the kernel's sizes (1024-entry lane tables, the coefficient planes, the scan), so that any access outside
// them ends the run.  The same input goes through jpeg_decode_segment, the serial route.
//
//   jpeg_chunked_harness IN OUT
//   IN : int32 cases; per case int32 {H, W, total_bytes, nseg, chunk_bytes}, uint8 record[1408], int32 segs[nseg][2],
//        uint8 bytes[total_bytes]
//   OUT: per case int32 {serial status, chunked status, ncoef, segments decoded}, per decoded segment int32 {serial
//        status, chunked status, rounds, lanes, damaged}, int16 serial coef[ncoef], int16 chunked coef[ncoef]
//        (coef[3][Bh][Bw][64], the kernel's layout; damaged: the scan-order index inside the segment of the block at
//        which the strict pass reported its status, -1 if it reported none)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jpeg_chunked.h"

static const uint8_t kZigzag[64] = {JPEG_ZIGZAG_LIST};
static const int kMaxLanes = 1024;   // JSCAN_MAX_LANES

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return fprintf(stderr, "cannot open the files\n"), 2;
  int32_t cases = 0;
  if (!get(in, &cases, 4)) return 2;
  for (int32_t i = 0; i < cases; ++i) {
    int32_t head[5];
    if (!get(in, head, sizeof head)) return 2;
    const int H = head[0], W = head[1], total_bytes = head[2], nseg = head[3], chunk_bytes = head[4];
    if (H < 1 || W < 8 || H > 32768 || W > 32768 || total_bytes < 0 || nseg < 0 || chunk_bytes < 4 ||
        chunk_bytes > 65536)
      return 2;
    std::vector<int32_t> rec32(JPEG_REC_BYTES / 4);   // the record is 4-byte aligned, as on the device
    uint8_t* rec = reinterpret_cast<uint8_t*>(rec32.data());
    std::vector<int32_t> segs(2 * (size_t)nseg);
    uint8_t* bytes = (uint8_t*)malloc(total_bytes ? total_bytes : 1);   // exactly the scan: reads behind it are caught
    if (!get(in, rec, JPEG_REC_BYTES) || !get(in, segs.data(), segs.size() * 4) || !get(in, bytes, total_bytes))
      return 2;
    rec32[JPEG_H_SEG_FIRST] = 0;
    rec32[JPEG_H_NSEG] = nseg;
    const JpegGeom g = jpeg_geom(rec32.data(), H, W);
    const JpegChunkGeom q = jpeg_chunk_geom(g);
    const size_t plane = (size_t)g.Bw * g.Bh * 64;
    int16_t* coef_s = (int16_t*)calloc(3 * plane, sizeof(int16_t));
    int16_t* coef_c = (int16_t*)calloc(3 * plane, sizeof(int16_t));
    JpegHuff* huff = (JpegHuff*)malloc(4 * sizeof(JpegHuff));
    for (int t = 0; t < 4; ++t) jpeg_huff_build(huff + t, rec + JPEG_REC_HUFF + t * JPEG_HUFF_BYTES);
    // the lane tables: the kernel's s_a .. s_d, the snapshot the barrier makes of s_a / s_b, the lanes' registers
    JpegChunkState* ent = (JpegChunkState*)malloc(kMaxLanes * sizeof(JpegChunkState));
    JpegChunkState* ex = (JpegChunkState*)malloc(kMaxLanes * sizeof(JpegChunkState));
    JpegChunkState* seen = (JpegChunkState*)malloc(kMaxLanes * sizeof(JpegChunkState));
    JpegChunkSum* sum = (JpegChunkSum*)malloc(kMaxLanes * sizeof(JpegChunkSum));
    const int total = g.mcus_x * g.mcus_y;
    const int want = jpeg_segments_wanted(total, g.dri);
    int32_t status_s = 0, status_c = 0;
    std::vector<int32_t> rows;
    for (int k = 0; k < g.nseg; ++k) {
      const int32_t sb = segs[2 * k], se = segs[2 * k + 1];
      const int st_s = jpeg_decode_segment(bytes, sb > 0 ? (uint32_t)sb : 0u, se > 0 ? (uint32_t)se : 0u,
                                           (uint32_t)total_bytes, g, huff, kZigzag, g.dri ? k * g.dri : 0,
                                           g.dri ? g.dri : total, (g.dri && k + 1 < want) ? (k & 7) : -1, coef_s);
      // ---- what the workgroup of segment k does ----
      const JpegChunkSeg sg = jpeg_chunk_segment(g, q, k, sb, se, (uint32_t)total_bytes, chunk_bytes, kMaxLanes);
      const int L = sg.lanes;
      std::vector<uint32_t> limit(L);
      for (int t = 0; t < L; ++t) {
        const uint32_t start = sg.begin + (uint32_t)t * (uint32_t)chunk_bytes;
        limit[t] = t == L - 1 ? 0xFFFFFFFFu : start + (uint32_t)chunk_bytes;
        ent[t] = ex[t] = jpeg_chunk_fresh(bytes, sg.begin, sg.end, start);
        sum[t] = JpegChunkSum{0u, 0u, 0u, 0u};
        if (t < L - 1) jpeg_chunk_speculate(bytes, sg.begin, sg.end, limit[t], q, huff, ent[t], ex[t], sum[t]);
      }
      int rounds = 0;
      for (int r = 0; r < L; ++r) {
        memcpy(seen, ex, (size_t)L * sizeof(JpegChunkState));   // the barrier
        int changed = 0;
        for (int t = 1; t < L; ++t) {
          if (jpeg_chunk_same(seen[t - 1], ent[t])) continue;
          ent[t] = seen[t - 1], changed = 1;
          if (t < L - 1) jpeg_chunk_speculate(bytes, sg.begin, sg.end, limit[t], q, huff, ent[t], ex[t], sum[t]);
        }
        ++rounds;
        if (!changed) break;
      }
      uint32_t blk0 = 0, p0 = 0, p1 = 0, p2 = 0;
      int st_c = 0;
      int32_t damaged = -1;
      for (int t = 0; t < L; ++t) {   // (every lane writes, as on the device; the first status in scan order counts)
        uint32_t at = 0;
        const int st = jpeg_chunk_write(bytes, sg.begin, sg.end, (uint32_t)total_bytes, limit[t], g, q, huff, kZigzag,
                                        ent[t], blk0, p0, p1, p2, sg.first_mcu, sg.n_blocks, sg.expect_rst, t == 0,
                                        coef_c, &at);
        if (st && !st_c) st_c = st, damaged = (int32_t)at;
        if (t < L - 1) blk0 += sum[t].blocks, p0 += sum[t].dc0, p1 += sum[t].dc1, p2 += sum[t].dc2;
      }
      if (st_s > status_s) status_s = st_s;
      if (st_c > status_c) status_c = st_c;
      const int32_t row[5] = {st_s, st_c, rounds, L, damaged};
      rows.insert(rows.end(), row, row + 5);
    }
    if (g.host_status) status_s = status_c = g.host_status;
    const int32_t tail[4] = {status_s, status_c, (int32_t)(3 * plane), g.nseg};
    fwrite(tail, 4, 4, out);
    fwrite(rows.data(), 4, rows.size(), out);
    fwrite(coef_s, sizeof(int16_t), 3 * plane, out);
    fwrite(coef_c, sizeof(int16_t), 3 * plane, out);
    free(sum), free(seen), free(ex), free(ent), free(huff), free(coef_c), free(coef_s), free(bytes);
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}
