// Host harness of openibl_amd/csrc/augment_geom.h and augment_pixel.h: the geometry of the colour jitter on a packed
// batch of mixed sizes (oibl_color_jitter_u8_mixed) and its pixel text, compiled without hipcc into a program of its
// own so that it can run under the host sanitizers (tests/test_jitter_mixed_cpu.py builds it with
// -fsanitize=address,undefined and -ffp-contract=off, the contraction setting of augment.hip).
//
//   jitter_mixed_harness sweep
//       For a sweep of sizes: the part arithmetic of jitter_mixed_image on the row the layout function wrote agrees
//       with jitter_geom of the uniform call, an image has at most CJ_MAX_PARTS parts, and the lanes' groups of all
//       parts — walked as the kernels walk them — cover every pixel exactly once, in order (arithmetic only: no pixel
//       is touched, so 2^28 pixels are in the sweep).  Prints one line per size; exit status 1 on the first failure.
//
//   jitter_mixed_harness run IN OUT
//       What the two launches do, workgroup by workgroup and lane by lane, IN PLACE on a buffer of exactly
//       packed_bytes bytes: a read or write outside it ends the run, one outside an image's [offset, offset + 3 H W)
//       shows in OUT (the caller fills the padding with a pattern).  Groups go by dwords or by bytes as
//       jitter_group_wide says.
//       IN : int32 {N, overrides, with_records}, int32 sizes[N][2], int32 records[N][8], uint8 packed[packed_bytes]
//            (packed_bytes: the layout function's total for `sizes`), int32 override[overrides][3] = {image, entry,
//            value}: written into the geometry table behind the layout function (an inconsistent table)
//       OUT: int64 packed_bytes, int32 ok[N], uint8 packed[packed_bytes]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "augment_geom.h"
#include "augment_pixel.h"

using namespace oibl;

#define CHECK(cond, ...) \
  do { \
    if (!(cond)) { \
      fprintf(stderr, "FAILED %s: ", #cond); \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n"); \
      exit(1); \
    } \
  } while (0)

// ---- sweep ----------------------------------------------------------------------------------------------------------
static void sweep_one(int H, int W) {
  const int32_t sizes[2] = {H, W};
  int32_t row[JPEG_MIX_GEOM_INTS];
  size_t totals[JPEG_MIX_TOTALS];
  int bad = -1, max_parts = 0;
  const long HW = (long)H * W;
  // the layout's own limit (coefficient blocks) is not the jitter's: lay a large image out by hand
  if (jpeg_mixed_layout(sizes, 1, row, totals, &bad) != 0) {
    memset(row, 0, sizeof row);
    row[JPEG_MIX_H] = H, row[JPEG_MIX_W] = W;
    totals[JPEG_MIX_T_PIXEL_BYTES] = (size_t)HW * 3;
  }
  CHECK(jitter_mixed_host(sizes, 1, &max_parts, &bad) == 0, "%d x %d", H, W);
  const JitterMixCall call = {(unsigned long long)totals[JPEG_MIX_T_PIXEL_BYTES], max_parts};
  const JitterMixImage im = jitter_mixed_image(row, call);
  const JitterGeom u = jitter_geom(H, W);
  CHECK(im.ok && im.pix == 0, "%d x %d", H, W);
  CHECK(im.geo.HW == u.HW && im.geo.chunk == u.chunk && im.geo.nparts == u.nparts && u.HW == HW, "%d x %d", H, W);
  CHECK(u.nparts >= 1 && u.nparts <= CJ_MAX_PARTS && u.nparts == max_parts, "%d x %d: %d parts", H, W, u.nparts);
  CHECK(u.chunk >= CJ_CHUNK && u.chunk % CJ_CHUNK == 0, "%d x %d: chunk %d", H, W, u.chunk);
  CHECK((long)(u.nparts - 1) * u.chunk < HW, "%d x %d: an empty last part", H, W);
  long next = 0;
  for (int part = 0; part < im.geo.nparts; ++part) {
    const long begin = (long)part * im.geo.chunk;
    CHECK(begin == next, "%d x %d: part %d begins at %ld, the last ended at %ld", H, W, part, begin, next);
    for (int s = 0; s < im.geo.chunk; s += CJ_STEP) {
      for (int t = 0; t < CJ_THREADS; ++t) {
        const long px = begin + s + (long)t * CJ_GROUP;
        if (px >= HW) break;                  // this lane and every lane behind it
        CHECK(px == next, "%d x %d: part %d step %d lane %d at %ld, expected %ld", H, W, part, s, t, px, next);
        const bool full = px + CJ_GROUP <= HW;
        CHECK(jitter_group_wide(true, px, HW) == full && !jitter_group_wide(false, px, HW), "%d x %d", H, W);
        next += full ? CJ_GROUP : HW - px;
      }
    }
    const long end = begin + im.geo.chunk < HW ? begin + im.geo.chunk : HW;
    CHECK(next == end, "%d x %d: part %d ends at %ld, not %ld", H, W, part, next, end);
  }
  CHECK(next == HW, "%d x %d: %ld of %ld pixels", H, W, next, HW);
  printf("%d x %d: %ld pixels, %d parts of %d, 3 H W %% 4 = %ld\n", H, W, HW, u.nparts, u.chunk, 3 * HW % 4);
}

static int sweep() {
  static const int kSizes[][2] = {
      {1, 1}, {1, 2}, {1, 3}, {5, 7}, {8, 8}, {37, 53}, {48, 64}, {63, 65}, {64, 64}, {64, 65}, {1, 4097}, {120, 160},
      {480, 640}, {2048, 2048}, {2048, 2049}, {4097, 1024}, {1100, 4000}, {32768, 1}, {1, 32768}, {16384, 16384},
      {32768, 8192}, {8192, 32768}};
  for (const auto& s : kSizes) sweep_one(s[0], s[1]);
  // what the host refuses, and what the workspace query then says
  int max_parts = 0, bad = -1;
  const int32_t big[4] = {8, 8, 16385, 16384}, zero[2] = {0, 4}, wide[2] = {4, 32769}, neg[2] = {-3, 4};
  CHECK(jitter_mixed_host(big, 2, &max_parts, &bad) == CJ_MIX_E_PIXELS && bad == 1, "2^28 + 16384 pixels");
  CHECK(jitter_mixed_host(zero, 1, &max_parts, &bad) == CJ_MIX_E_SIZE && bad == 0, "0 x 4");
  CHECK(jitter_mixed_host(wide, 1, &max_parts, &bad) == CJ_MIX_E_SIZE && bad == 0, "4 x 32769");
  CHECK(jitter_mixed_host(neg, 1, &max_parts, &bad) == CJ_MIX_E_SIZE && bad == 0, "-3 x 4");
  printf("ok\n");
  return 0;
}

// ---- run ------------------------------------------------------------------------------------------------------------
// load_group of augment.hip: dwords where jitter_group_wide says so, else bytes, those behind the image as zero
static void load_group(const uint8_t* img, long px, long HW, bool dwords, int (&c)[12]) {
  if (jitter_group_wide(dwords, px, HW)) {
    uint32_t v[3];
    memcpy(v, img + 3 * px, 12);
    for (int k = 0; k < 12; ++k) c[k] = (int)((v[k >> 2] >> (8 * (k & 3))) & 255u);
  } else {
    for (int k = 0; k < 12; ++k) {
      const long at = 3 * px + k;
      c[k] = at < 3 * HW ? (int)img[at] : 0;
    }
  }
}

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static int run(const char* in_name, const char* out_name) {
  FILE* in = fopen(in_name, "rb");
  FILE* out = fopen(out_name, "wb");
  if (!in || !out) return fprintf(stderr, "cannot open the files\n"), 2;
  int32_t head[3];
  if (!get(in, head, sizeof head)) return 2;
  const int N = head[0], overrides = head[1], with_records = head[2];
  if (N < 1 || N > 65535 || overrides < 0) return 2;
  std::vector<int32_t> sizes(2 * (size_t)N), recs(8 * (size_t)N), geom((size_t)N * JPEG_MIX_GEOM_INTS);
  if (!get(in, sizes.data(), sizes.size() * 4) || !get(in, recs.data(), recs.size() * 4)) return 2;
  size_t totals[JPEG_MIX_TOTALS];
  int bad = -1;
  JitterMixCall call = {0, 0};
  if (jpeg_mixed_layout(sizes.data(), N, geom.data(), totals, &bad) != 0) return 2;
  if (jitter_mixed_host(sizes.data(), N, &call.max_parts, &bad) != 0) return 2;
  call.packed_bytes = totals[JPEG_MIX_T_PIXEL_BYTES];
  std::vector<uint8_t> packed((size_t)call.packed_bytes);      // exactly: the sanitizer sees every byte behind it
  if (!get(in, packed.data(), packed.size())) return 2;
  for (int k = 0; k < overrides; ++k) {
    int32_t o[3];
    if (!get(in, o, sizeof o) || o[0] < 0 || o[0] >= N || o[1] < 0 || o[1] >= JPEG_MIX_GEOM_INTS) return 2;
    geom[(size_t)o[0] * JPEG_MIX_GEOM_INTS + o[1]] = o[2];
  }
  fclose(in);

  std::vector<unsigned long long> parts((size_t)N * call.max_parts, 0xDEADBEEFull);   // the workspace, [N][max_parts]
  std::vector<int32_t> ok((size_t)N);
  const JitterRecord* records = with_records ? reinterpret_cast<const JitterRecord*>(recs.data()) : nullptr;
  // launch 1, grid (max_parts, N)
  for (int n = 0; n < N && records; ++n)
    for (int part = 0; part < call.max_parts; ++part) {
      const JitterMixImage im = jitter_mixed_image(geom.data() + (size_t)n * JPEG_MIX_GEOM_INTS, call);
      if (!im.ok || part >= im.geo.nparts) continue;
      CHECK(im.pix + (unsigned long long)im.geo.HW * 3 <= call.packed_bytes, "image %d passes the buffer", n);
      const JitterOps ops = cj_decode(records + n);
      if (ops.contrast_at == 4) continue;
      const uint8_t* img = packed.data() + im.pix;
      const bool dwords = (uintptr_t)im.pix % 4 == 0;
      unsigned long long sum = 0;
      for (int s = 0; s < im.geo.chunk; s += CJ_STEP)
        for (int t = 0; t < CJ_THREADS; ++t) {
          const long px = (long)part * im.geo.chunk + s + (long)t * CJ_GROUP;
          if (px >= im.geo.HW) break;
          int c[12];
          load_group(img, px, im.geo.HW, dwords, c);
          for (int j = 0; j < CJ_GROUP; ++j)
            if (px + j < im.geo.HW) {
              int r = c[3 * j], g = c[3 * j + 1], b = c[3 * j + 2];
              cj_apply(ops, 0, ops.contrast_at, 0, r, g, b);
              sum += (unsigned)cj_luma(r, g, b);
            }
        }
      parts[(size_t)n * call.max_parts + part] = sum;
    }
  // launch 2, in place
  for (int n = 0; n < N; ++n) {
    const JitterMixImage im = jitter_mixed_image(geom.data() + (size_t)n * JPEG_MIX_GEOM_INTS, call);
    ok[n] = im.ok;
    if (!im.ok) continue;
    CHECK(im.geo.nparts <= call.max_parts, "image %d has %d parts, the grid %d", n, im.geo.nparts, call.max_parts);
    const JitterOps ops = cj_decode(records ? records + n : nullptr);
    int mean = 0;
    if (ops.contrast_at < 4) {
      unsigned long long sum = 0;
      for (int i = 0; i < im.geo.nparts; ++i) sum += parts[(size_t)n * call.max_parts + i];
      mean = cj_contrast_mean(sum, im.geo.HW);
    }
    uint8_t* img = packed.data() + im.pix;
    const bool dwords = (uintptr_t)im.pix % 4 == 0;
    for (int part = 0; part < im.geo.nparts; ++part)
      for (int s = 0; s < im.geo.chunk; s += CJ_STEP)
        for (int t = 0; t < CJ_THREADS; ++t) {
          const long px = (long)part * im.geo.chunk + s + (long)t * CJ_GROUP;
          if (px >= im.geo.HW) break;
          int c[12];
          load_group(img, px, im.geo.HW, dwords, c);
          for (int j = 0; j < CJ_GROUP; ++j) cj_apply(ops, 0, 4, mean, c[3 * j], c[3 * j + 1], c[3 * j + 2]);
          if (jitter_group_wide(dwords, px, im.geo.HW)) {
            uint32_t v[3];
            for (int k = 0; k < 3; ++k)
              v[k] = (uint32_t)c[4 * k] | ((uint32_t)c[4 * k + 1] << 8) | ((uint32_t)c[4 * k + 2] << 16) |
                     ((uint32_t)c[4 * k + 3] << 24);
            memcpy(img + 3 * px, v, 12);
          } else {
            for (int k = 0; k < 12; ++k)
              if (3 * px + k < 3 * im.geo.HW) {
                CHECK(im.pix + 3 * px + k < im.pix + (unsigned long long)im.geo.HW * 3, "a tail byte outside");
                img[3 * px + k] = (uint8_t)c[k];
              }
          }
        }
  }
  const long long nbytes = (long long)call.packed_bytes;
  fwrite(&nbytes, sizeof nbytes, 1, out);
  fwrite(ok.data(), 4, ok.size(), out);
  fwrite(packed.data(), 1, packed.size(), out);
  fclose(out);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
  if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
  return fprintf(stderr, "usage: %s sweep | run IN OUT\n", argv[0]), 2;
}
