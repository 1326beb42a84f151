// Host harness of openibl_amd/csrc/jpeg_entropy.h: the text the entropy kernel is made of, compiled without hipcc
// into a program of its own so that it can run under the host sanitizers (tests/test_jpeg_decode_cpu.py builds it with
// -fsanitize=address,undefined).  It decodes every case of an input file the way jpeg_entropy_kernel does — the four
// tables built from the record, one jpeg_serial_segment per row of the segment table — into heap buffers of exactly
// the sizes the kernel's bounds are stated for, so that any access outside them ends the run.
//
//   jpeg_entropy_harness IN OUT
//   IN : int32 cases; per case int32 {H, W, total_bytes, nseg}, uint8 record[1408], int32 segs[nseg][2],
//        uint8 bytes[total_bytes]
//   OUT: per case int32 {status, ncoef}, int16 coef[ncoef]   (coef[3][Bh][Bw][64], the kernel's layout)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jpeg_entropy.h"

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
    int32_t head[4];
    if (!get(in, head, sizeof head)) return 2;
    const int H = head[0], W = head[1], total_bytes = head[2], nseg = head[3];
    if (H < 1 || W < 8 || H > 32768 || W > 32768 || total_bytes < 0 || nseg < 0) return 2;
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
    int16_t* coef = (int16_t*)calloc(3 * plane, sizeof(int16_t));
    JpegHuff* huff = (JpegHuff*)malloc(4 * sizeof(JpegHuff));
    for (int t = 0; t < 4; ++t) jpeg_huff_build(huff + t, rec + JPEG_REC_HUFF + t * JPEG_HUFF_BYTES);
    int32_t status = 0;
    for (int k = 0; k < g.nseg; ++k) {   // what lane k of the kernel does
      const int st = jpeg_serial_segment(bytes, (uint32_t)total_bytes, g, segs.data(), nseg, huff, kZigzag, k, coef);
      if (st > status) status = st;
    }
    if (g.host_status) status = g.host_status;
    const int32_t tail[2] = {status, (int32_t)(3 * plane)};
    fwrite(tail, 4, 2, out);
    fwrite(coef, sizeof(int16_t), 3 * plane, out);
    free(huff), free(coef), free(bytes);
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}
