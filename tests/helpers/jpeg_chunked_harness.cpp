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
#include "jpeg_workgroup_emul.h"

static const uint8_t kZigzag[64] = {JPEG_ZIGZAG_LIST};

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
    const size_t plane = (size_t)g.Bw * g.Bh * 64;
    int16_t* coef_s = (int16_t*)calloc(3 * plane, sizeof(int16_t));
    int16_t* coef_c = (int16_t*)calloc(3 * plane, sizeof(int16_t));
    JpegHuff* huff = (JpegHuff*)malloc(4 * sizeof(JpegHuff));
    for (int t = 0; t < 4; ++t) jpeg_huff_build(huff + t, rec + JPEG_REC_HUFF + t * JPEG_HUFF_BYTES);
    int32_t status_s = 0, status_c = 0;
    std::vector<int32_t> rows;
    for (int k = 0; k < g.nseg; ++k) {
      const int st_s =
          jpeg_serial_segment(bytes, (uint32_t)total_bytes, g, segs.data(), nseg, huff, kZigzag, k, coef_s);
      const JpegEmulSegment c = jpeg_emul_chunked_segment(bytes, (uint32_t)total_bytes, g, segs.data(), nseg, huff,
                                                          kZigzag, chunk_bytes, k, coef_c);
      if (st_s > status_s) status_s = st_s;
      if (c.status > status_c) status_c = c.status;
      const int32_t row[5] = {st_s, c.status, c.rounds, c.lanes, c.damaged};
      rows.insert(rows.end(), row, row + 5);
    }
    if (g.host_status) status_s = status_c = g.host_status;
    const int32_t tail[4] = {status_s, status_c, (int32_t)(3 * plane), g.nseg};
    fwrite(tail, 4, 4, out);
    fwrite(rows.data(), 4, rows.size(), out);
    fwrite(coef_s, sizeof(int16_t), 3 * plane, out);
    fwrite(coef_c, sizeof(int16_t), 3 * plane, out);
    free(huff), free(coef_c), free(coef_s), free(bytes);
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}
