// Host harness of openibl_amd/csrc/jpeg_mixed.h: the layout function and the entropy stage of the jmix_* kernels of
// csrc/jpeg.hip on a batch of images of mixed sizes, compiled without hipcc into a program of its own so that it can
// run under the host sanitizers (tests/test_jpeg_mixed_cpu.py builds it with -fsanitize=address,undefined).  What such
// a kernel does per image is done here per image, with the same shared text: the table row through
// jpeg_mixed_image against the call's totals, jpeg_geom with the row's H and W, then every segment through
// jpeg_serial_segment (the serial route) and through the chunk state machine as a workgroup runs it (the chunked
// route; the loop of tests/helpers/jpeg_workgroup_emul.h), into ONE coefficient buffer of exactly the layout's size
// per route, so that an access outside an image's extent that leaves the buffer ends the run, and one that stays
// inside shows as a difference from the same image decoded alone.
//
//   jpeg_mixed_harness IN OUT
//   IN : int32 {N, S, scan_len, chunk_bytes, overrides}, int32 sizes[N][2], uint8 records[N][1408],
//        int32 segs[S][2], uint8 scan[scan_len], int32 override[overrides][3] = {image, entry, value}: written into
//        the geometry table behind the layout function (an inconsistent table)
//   OUT: int32 geom[N][8], int64 totals[6], then per image int32 {status serial, status chunked, status alone, ok,
//        ncoef}, int16 alone[ncoef], int16 serial[ncoef], int16 chunked[ncoef] (ncoef = 0 for an image the table check
//        refuses; `alone`: the image decoded on its own by jpeg_serial_segment into a buffer of its own)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jpeg_chunked.h"
#include "jpeg_mixed.h"
#include "jpeg_workgroup_emul.h"

static const uint8_t kZigzag[64] = {JPEG_ZIGZAG_LIST};

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return fprintf(stderr, "cannot open the files\n"), 2;
  int32_t head[5];
  if (!get(in, head, sizeof head)) return 2;
  const int N = head[0], S = head[1], scan_len = head[2], chunk_bytes = head[3], overrides = head[4];
  if (N < 1 || N > 65535 || S < 0 || scan_len < 0 || chunk_bytes < 4 || chunk_bytes > 65536 || overrides < 0) return 2;
  std::vector<int32_t> sizes(2 * (size_t)N), rec32((size_t)N * JPEG_REC_BYTES / 4), segs(2 * (size_t)S);
  std::vector<int32_t> over(3 * (size_t)overrides);
  uint8_t* bytes = (uint8_t*)malloc(scan_len ? scan_len : 1);   // exactly the scans: reads behind them are caught
  if (!get(in, sizes.data(), sizes.size() * 4) || !get(in, rec32.data(), rec32.size() * 4) ||
      !get(in, segs.data(), segs.size() * 4) || !get(in, bytes, scan_len) || !get(in, over.data(), over.size() * 4))
    return 2;
  fclose(in);

  // ---- the layout, then what the test wants wrong in it ----
  std::vector<int32_t> geom((size_t)N * JPEG_MIX_GEOM_INTS);
  size_t totals[JPEG_MIX_TOTALS];
  int bad = -1;
  if (jpeg_mixed_layout(sizes.data(), N, geom.data(), totals, &bad))
    return fprintf(stderr, "layout: image %d\n", bad), 3;
  const std::vector<int32_t> geom_written = geom;
  for (int i = 0; i < overrides; ++i) {
    if (over[3 * i] < 0 || over[3 * i] >= N || over[3 * i + 1] < 0 || over[3 * i + 1] >= JPEG_MIX_GEOM_INTS) return 2;
    geom[(size_t)over[3 * i] * JPEG_MIX_GEOM_INTS + over[3 * i + 1]] = over[3 * i + 2];
  }
  JpegMixSpaces sp;   // as oibl_jpeg_decode_mixed fills it
  sp.plane_blocks = totals[JPEG_MIX_T_PLANE_BYTES] / 64;
  sp.coef_blocks = sp.plane_blocks;
  sp.pixel_bytes = totals[JPEG_MIX_T_PIXEL_BYTES];
  sp.max_blocks = (int)totals[JPEG_MIX_T_MAX_BLOCKS];
  sp.max_h = (int)totals[JPEG_MIX_T_MAX_H];
  sp.max_w = (int)totals[JPEG_MIX_T_MAX_W];
  const size_t ncoef_all = totals[JPEG_MIX_T_COEF_BYTES] / sizeof(int16_t);
  int16_t* coef_s = (int16_t*)calloc(ncoef_all, sizeof(int16_t));   // exactly the layout's coefficients, per route
  int16_t* coef_c = (int16_t*)calloc(ncoef_all, sizeof(int16_t));
  JpegHuff* huff = (JpegHuff*)malloc(4 * sizeof(JpegHuff));

  fwrite(geom_written.data(), 4, geom_written.size(), out);
  const int64_t t64[JPEG_MIX_TOTALS] = {(int64_t)totals[0], (int64_t)totals[1], (int64_t)totals[2],
                                        (int64_t)totals[3], (int64_t)totals[4], (int64_t)totals[5]};
  fwrite(t64, 8, JPEG_MIX_TOTALS, out);

  struct Done { int32_t st_s, st_c, st_a, ok; size_t at, n; std::vector<int16_t> alone; };
  std::vector<Done> done(N);
  for (int n = 0; n < N; ++n) {
    const uint8_t* rec = reinterpret_cast<const uint8_t*>(rec32.data()) + (size_t)n * JPEG_REC_BYTES;
    const int32_t* hdr = reinterpret_cast<const int32_t*>(rec);
    Done& d = done[n];
    for (int t = 0; t < 4; ++t) jpeg_huff_build(huff + t, rec + JPEG_REC_HUFF + t * JPEG_HUFF_BYTES);
    // the image alone, with the sizes the test gave
    {
      const JpegGeom g = jpeg_geom(hdr, sizes[2 * n], sizes[2 * n + 1]);
      d.alone.assign((size_t)3 * g.Bw * g.Bh * 64, 0);
      d.st_a = 0;
      for (int k = 0; k < g.nseg; ++k) {
        const int st = jpeg_serial_segment(bytes, (uint32_t)scan_len, g, segs.data(), S, huff, kZigzag, k,
                                           d.alone.data());
        if (st > d.st_a) d.st_a = st;
      }
      if (g.host_status) d.st_a = g.host_status;
    }
    // the image as the jmix_* kernels see it
    const JpegMixImage im = jpeg_mixed_image(geom.data() + (size_t)n * JPEG_MIX_GEOM_INTS, sp);
    d.ok = im.ok, d.at = (size_t)im.coef * 64, d.n = 0;
    d.st_s = d.st_c = JPEG_ST_BAD_GEOM;
    if (!im.ok) continue;
    const JpegGeom g = jpeg_geom(hdr, im.H, im.W);
    d.n = (size_t)3 * g.Bw * g.Bh * 64;
    d.st_s = d.st_c = 0;
    for (int k = 0; k < g.nseg; ++k) {
      const int ss =
          jpeg_serial_segment(bytes, (uint32_t)scan_len, g, segs.data(), S, huff, kZigzag, k, coef_s + d.at);
      const int sc = jpeg_emul_chunked_segment(bytes, (uint32_t)scan_len, g, segs.data(), S, huff, kZigzag, chunk_bytes,
                                               k, coef_c + d.at).status;
      if (ss > d.st_s) d.st_s = ss;
      if (sc > d.st_c) d.st_c = sc;
    }
    if (g.host_status) d.st_s = d.st_c = g.host_status;
  }
  for (int n = 0; n < N; ++n) {
    const Done& d = done[n];
    const int32_t row[5] = {d.st_s, d.st_c, d.st_a, d.ok, (int32_t)d.n};
    fwrite(row, 4, 5, out);
    if (!d.n) continue;
    // an accepted row of an overridden table may have another size than the test's: the image alone is then cut or
    // padded to the accepted extent (the test compares only rows it left alone)
    std::vector<int16_t> alone(d.n, 0);
    memcpy(alone.data(), d.alone.data(), (d.n < d.alone.size() ? d.n : d.alone.size()) * sizeof(int16_t));
    fwrite(alone.data(), 2, d.n, out);
    fwrite(coef_s + d.at, 2, d.n, out);
    fwrite(coef_c + d.at, 2, d.n, out);
  }
  free(huff), free(coef_c), free(coef_s), free(bytes);
  return fclose(out) == 0 ? 0 : 2;
}
