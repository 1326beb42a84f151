// The device JPEG decoder for a batch of MIXED stored sizes: the stages of csrc/jpeg.hip and the chunked entropy
// stage of csrc/jpeg_chunked.hip — the same text, jpeg_stages.h — with every image's H, W and base offsets taken from
// a per-image geometry table (jpeg_mixed.h) instead of kernel arguments.  All images' segments decode in ONE entropy
// launch, and the colour stage writes image n as a contiguous [H_n][W_n][3] block at its byte offset of one packed
// uint8 buffer, which csrc/resize.hip (oibl_resize_u8_mixed) reads into the dense batch.
//
//   jmix_entropy_kernel / jmix_chunk_kernel   grid (.., N) as in the uniform decoder; max_segments is the batch's
//   jmix_idct_kernel                          grid (ceil(largest Bw * Bh / 256), 3, N)
//   jmix_colour_kernel                        grid (ceil(largest W / 64), ceil(largest H / 4), N)
//
// The grids are sized by the batch's largest image; a workgroup outside its image leaves after reading the image's
// table row (one 32-byte row, the same address in every lane).  A tile list built next to the table would launch no
// empty workgroup but costs a second table on the host, a second indirection per workgroup and a transfer that grows
// with the pixels instead of the images; for the mixes a folder has (portrait next to landscape, two or three camera
// resolutions: a factor of 4 in area) the empty workgroups are a few microseconds of a call that takes milliseconds.
//
// Bounds: jpeg_mixed_image forces every entry of a row into its range and checks the image's extent against the totals
// this call was given; an image that fails is skipped by every stage and gets status 5.  Inside its extent an image is
// indexed exactly as in the uniform decoder.  All integer, no atomics, nothing of one image reaches another.
#include "common.h"

#include "jpeg_mixed.h"
#include "jpeg_stages.h"

namespace oibl {

__constant__ uint8_t c_jmix_zigzag[64] = {JPEG_ZIGZAG_LIST};

// grid (ceil(max_segments / 64), N), 64 threads
__global__ __launch_bounds__(64) void jmix_entropy_kernel(const uint8_t* bytes, uint32_t total_bytes,
                                                          const uint8_t* records, const int32_t* segs, int S,
                                                          const int32_t* geom, JpegMixSpaces spaces, int16_t* coef,
                                                          int32_t* seg_status) {
  __shared__ JpegHuff s_huff[4];
  __shared__ uint8_t s_zz[64];
  const int tid = threadIdx.x, n = blockIdx.y;
  const JpegMixImage im = jpeg_mixed_image(geom + (size_t)n * JPEG_MIX_GEOM_INTS, spaces);
  if (!im.ok) return;
  const uint8_t* rec = records + (size_t)n * JPEG_REC_BYTES;
  const JpegGeom g = jpeg_geom(reinterpret_cast<const int32_t*>(rec), im.H, im.W);
  if ((int)blockIdx.x * 64 >= g.nseg) return;   // the whole workgroup
  if (tid < 4) jpeg_huff_build(&s_huff[tid], rec + JPEG_REC_HUFF + tid * JPEG_HUFF_BYTES);
  s_zz[tid] = c_jmix_zigzag[tid];
  __syncthreads();
  jpeg_entropy_lane(bytes, total_bytes, g, segs, S, s_huff, s_zz, blockIdx.x * 64 + tid,
                    coef + (size_t)im.coef * 64, seg_status);
}

// grid (max_segments, N), T threads: T a power of two, 64 <= T <= 1024
__global__ __launch_bounds__(JSCAN_MAX_LANES) void jmix_chunk_kernel(const uint8_t* bytes, uint32_t total_bytes,
                                                                     const uint8_t* records, const int32_t* segs,
                                                                     int S, const int32_t* geom, JpegMixSpaces spaces,
                                                                     int chunk_bytes, int16_t* coef,
                                                                     int32_t* seg_status, int32_t* seg_rounds) {
  __shared__ JpegHuff s_huff[4];
  __shared__ uint8_t s_zz[64];
  const int tid = threadIdx.x, k = blockIdx.x, n = blockIdx.y;
  const JpegMixImage im = jpeg_mixed_image(geom + (size_t)n * JPEG_MIX_GEOM_INTS, spaces);
  if (!im.ok) return;
  const uint8_t* rec = records + (size_t)n * JPEG_REC_BYTES;
  const JpegGeom g = jpeg_geom(reinterpret_cast<const int32_t*>(rec), im.H, im.W);
  if (k >= g.nseg || g.seg_first > S - 1 - k) return;   // the whole workgroup
  if (tid < 4) jpeg_huff_build(&s_huff[tid], rec + JPEG_REC_HUFF + tid * JPEG_HUFF_BYTES);
  if (tid < 64) s_zz[tid] = c_jmix_zigzag[tid];
  __syncthreads();
  jpeg_chunked_segment(bytes, total_bytes, g, segs, chunk_bytes, s_huff, s_zz, k, coef + (size_t)im.coef * 64,
                       seg_status, seg_rounds);
}

// grid (ceil(spaces.max_blocks / 256), 3, N), 256 threads
__global__ __launch_bounds__(256) void jmix_idct_kernel(const uint8_t* records, const int32_t* geom,
                                                        JpegMixSpaces spaces, const int16_t* coef, uint8_t* planes) {
  const int n = blockIdx.z;
  const JpegMixImage im = jpeg_mixed_image(geom + (size_t)n * JPEG_MIX_GEOM_INTS, spaces);
  if (!im.ok) return;
  const uint8_t* rec = records + (size_t)n * JPEG_REC_BYTES;
  const JpegGeom g = jpeg_geom(reinterpret_cast<const int32_t*>(rec), im.H, im.W);
  const int c = blockIdx.y;
  if (c >= g.ncomp || (int)blockIdx.x * 256 >= g.Bw * g.Bh) return;   // the whole workgroup: nothing of this image here
  jpeg_idct_stage(rec, jpeg_idct_plane(g, c), c, blockIdx.x * 256 + threadIdx.x, coef + (size_t)im.coef * 64,
                  planes + (size_t)im.plane * 64);
}

// grid (ceil(spaces.max_w / 64), ceil(spaces.max_h / 4), N), (64, 4) threads
__global__ __launch_bounds__(256) void jmix_colour_kernel(const uint8_t* records, const int32_t* geom,
                                                          JpegMixSpaces spaces, const uint8_t* planes,
                                                          const int32_t* seg_status, int S, uint8_t* out,
                                                          int32_t* status) {
  __shared__ int s_max[4];
  const int n = blockIdx.z;
  const JpegMixImage im = jpeg_mixed_image(geom + (size_t)n * JPEG_MIX_GEOM_INTS, spaces);
  if (!im.ok) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) status[n] = JPEG_ST_BAD_GEOM;
    return;
  }
  if ((int)blockIdx.x * 64 >= im.W || (int)blockIdx.y * 4 >= im.H) return;   // the whole workgroup
  const JpegGeom g = jpeg_geom(reinterpret_cast<const int32_t*>(records + (size_t)n * JPEG_REC_BYTES), im.H, im.W);
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x < im.W && y < im.H)
    jpeg_colour_pixel(g, planes + (size_t)im.plane * 64, im.H, im.W, y, x,
                      out + im.pix + ((size_t)y * im.W + x) * 3);
  if (blockIdx.x == 0 && blockIdx.y == 0) jpeg_image_status(g, seg_status, S, s_max, status + n);
}

struct JmixLayout {
  size_t coef, seg_status, seg_rounds, planes, zero_bytes, total;   // byte offsets; [coef, zero_bytes): zeroed per call
};

static JmixLayout jmix_layout(const size_t* totals, int S) {
  JmixLayout l;
  size_t at = 0;
  l.coef = at, at += align_up(totals[JPEG_MIX_T_COEF_BYTES], 256);
  l.seg_status = at, at += align_up((size_t)S * sizeof(int32_t), 256);
  l.seg_rounds = at, at += align_up((size_t)S * sizeof(int32_t), 256);
  l.zero_bytes = at;
  l.planes = at, at += align_up(totals[JPEG_MIX_T_PLANE_BYTES], 256);
  l.total = at;
  return l;
}

// the totals of a layout jpeg_mixed_layout could have written
static bool jmix_totals_ok(const size_t* t) {
  const size_t planes = t[JPEG_MIX_T_PLANE_BYTES];
  return planes >= 3 * 4 * 64 && planes % 64 == 0 && planes / 64 < JPEG_MIX_MAX_BLOCKS &&
         t[JPEG_MIX_T_COEF_BYTES] == 2 * planes && t[JPEG_MIX_T_PIXEL_BYTES] >= 1 &&
         t[JPEG_MIX_T_PIXEL_BYTES] < JPEG_MIX_MAX_PIXEL_BYTES && t[JPEG_MIX_T_MAX_BLOCKS] >= 4 &&
         3 * t[JPEG_MIX_T_MAX_BLOCKS] <= planes / 64 && t[JPEG_MIX_T_MAX_H] >= 1 &&
         t[JPEG_MIX_T_MAX_H] <= JPEG_MIX_MAX_DIM && t[JPEG_MIX_T_MAX_W] >= 1 &&
         t[JPEG_MIX_T_MAX_W] <= JPEG_MIX_MAX_DIM &&
         t[JPEG_MIX_T_MAX_BLOCKS] <= (size_t)(JPEG_MIX_MAX_DIM / 8) * (JPEG_MIX_MAX_DIM / 8);
}

static bool jmix_shape_ok(int N, int S) { return N > 0 && N <= 65535 && S >= N && S <= (1 << 28); }

}  // namespace oibl

using namespace oibl;

extern "C" {

int oibl_jpeg_mixed_layout(const int32_t* sizes_host, int N, int32_t* geom_host, size_t* totals_host) {
  OIBL_REQUIRE(sizes_host && geom_host && totals_host, "jpeg_mixed_layout: null pointer");
  OIBL_REQUIRE(N > 0 && N <= 65535, "jpeg_mixed_layout: N = %d must be in [1, 65535]", N);
  int bad = -1;
  const int why = jpeg_mixed_layout(sizes_host, N, geom_host, totals_host, &bad);
  OIBL_REQUIRE(why != JPEG_MIX_E_SIZE, "jpeg_mixed_layout: image %d is %d x %d, every side must be in [1, %d]", bad,
               sizes_host[2 * bad], sizes_host[2 * bad + 1], JPEG_MIX_MAX_DIM);
  OIBL_REQUIRE(why != JPEG_MIX_E_BLOCKS, "jpeg_mixed_layout: 2^31 coefficient blocks or more at image %d", bad);
  OIBL_REQUIRE(why != JPEG_MIX_E_PIXELS, "jpeg_mixed_layout: 2^40 packed pixel bytes or more at image %d", bad);
  return OIBL_OK;
}

size_t oibl_jpeg_decode_mixed_workspace_bytes(const size_t* totals_host, int N, int S) {
  if (!totals_host || !jmix_shape_ok(N, S) || !jmix_totals_ok(totals_host)) return 0;
  return jmix_layout(totals_host, S).total;
}

int oibl_jpeg_decode_mixed(const uint8_t* scan_bytes, size_t scan_len, const void* records, const int32_t* segments,
                           int S, int max_segments, int N, const int32_t* geom_dev, const size_t* totals_host,
                           int chunk_bytes, uint8_t* out_packed, int32_t* status, void* ws, size_t ws_bytes,
                           void* stream) {
  OIBL_REQUIRE(scan_bytes && records && segments && geom_dev && totals_host && out_packed && status,
               "jpeg_decode_mixed: null pointer");
  OIBL_REQUIRE(chunk_bytes == 0 || (chunk_bytes >= 4 && chunk_bytes <= 65536),
               "jpeg_decode_mixed: chunk_bytes %d must be 0 (the serial route) or in [4, 65536]", chunk_bytes);
  OIBL_REQUIRE(jmix_shape_ok(N, S), "jpeg_decode_mixed: bad shape N=%d S=%d (N <= 65535, N <= S <= 2^28)", N, S);
  OIBL_REQUIRE(jmix_totals_ok(totals_host),
               "jpeg_decode_mixed: the totals are not those of a layout (coefficient bytes %zu, plane bytes %zu, pixel "
               "bytes %zu < 2^40, largest Bw * Bh %zu, largest H %zu and W %zu <= %d)",
               totals_host[JPEG_MIX_T_COEF_BYTES], totals_host[JPEG_MIX_T_PLANE_BYTES],
               totals_host[JPEG_MIX_T_PIXEL_BYTES], totals_host[JPEG_MIX_T_MAX_BLOCKS], totals_host[JPEG_MIX_T_MAX_H],
               totals_host[JPEG_MIX_T_MAX_W], JPEG_MIX_MAX_DIM);
  OIBL_REQUIRE(scan_len >= 1 && scan_len <= 0x7fffffffu, "jpeg_decode_mixed: scan_len %zu must be in [1, 2^31)",
               scan_len);
  OIBL_REQUIRE(max_segments >= 1 && max_segments <= S, "jpeg_decode_mixed: max_segments %d must be in [1, S = %d]",
               max_segments, S);
  OIBL_REQUIRE((uintptr_t)records % 4 == 0 && (uintptr_t)segments % 4 == 0 && (uintptr_t)status % 4 == 0 &&
                   (uintptr_t)geom_dev % 4 == 0,
               "jpeg_decode_mixed: records, segments, geom_dev and status must be 4-byte aligned");
  OIBL_REQUIRE(ws && (uintptr_t)ws % 256 == 0, "jpeg_decode_mixed: workspace must be 256-byte aligned");
  const JmixLayout l = jmix_layout(totals_host, S);
  if (ws_bytes < l.total) {
    set_error("jpeg_decode_mixed: workspace %zu < required %zu bytes", ws_bytes, l.total);
    return OIBL_E_WORKSPACE;
  }
  JpegMixSpaces sp;
  sp.plane_blocks = totals_host[JPEG_MIX_T_PLANE_BYTES] / 64;
  sp.coef_blocks = sp.plane_blocks;
  sp.pixel_bytes = totals_host[JPEG_MIX_T_PIXEL_BYTES];
  sp.max_blocks = (int)totals_host[JPEG_MIX_T_MAX_BLOCKS];
  sp.max_h = (int)totals_host[JPEG_MIX_T_MAX_H];
  sp.max_w = (int)totals_host[JPEG_MIX_T_MAX_W];
  hipStream_t st = (hipStream_t)stream;
  int16_t* coef = (int16_t*)((char*)ws + l.coef);
  int32_t* seg_status = (int32_t*)((char*)ws + l.seg_status);
  int32_t* seg_rounds = (int32_t*)((char*)ws + l.seg_rounds);
  uint8_t* planes = (uint8_t*)ws + l.planes;
  const uint8_t* rec = (const uint8_t*)records;
  OIBL_HIP_CHECK(hipMemsetAsync(coef, 0, l.zero_bytes, st));
  if (chunk_bytes == 0) {
    hipLaunchKernelGGL(jmix_entropy_kernel, dim3((unsigned)((max_segments + 63) / 64), (unsigned)N), dim3(64), 0, st,
                       scan_bytes, (uint32_t)scan_len, rec, segments, S, geom_dev, sp, coef, seg_status);
  } else {
    // no segment is longer than the batch's bytes: as many threads as its chunks, a power of two from 64 to 1024
    const size_t chunks = (scan_len + (size_t)chunk_bytes - 1) / (size_t)chunk_bytes;
    unsigned threads = 64;
    while (threads < (unsigned)JSCAN_MAX_LANES && threads < chunks) threads <<= 1;
    hipLaunchKernelGGL(jmix_chunk_kernel, dim3((unsigned)max_segments, (unsigned)N), dim3(threads), 0, st, scan_bytes,
                       (uint32_t)scan_len, rec, segments, S, geom_dev, sp, chunk_bytes, coef, seg_status, seg_rounds);
  }
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(jmix_idct_kernel, dim3((unsigned)((sp.max_blocks + 255) / 256), 3u, (unsigned)N), dim3(256), 0,
                     st, rec, geom_dev, sp, (const int16_t*)coef, planes);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(jmix_colour_kernel,
                     dim3((unsigned)((sp.max_w + 63) / 64), (unsigned)((sp.max_h + 3) / 4), (unsigned)N), dim3(64, 4),
                     0, st, rec, geom_dev, sp, (const uint8_t*)planes, (const int32_t*)seg_status, S, out_packed,
                     status);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

}  // extern "C"
