// The chunked route of the device JPEG decoder: the entropy stage of csrc/jpeg.hip with many lanes per segment, for
// scans without restart markers (one lane per image there).  A segment — a restart interval, or a whole scan — is cut
// into chunks of `chunk_bytes` raw bytes; ONE workgroup serves it, a lane per chunk, at most 1024 (the last lane takes
// what is left).  The state machine is the shared text of jpeg_chunked.h; its schedule is jpeg_chunked_segment of
// jpeg_stages.h (csrc/jpeg_mixed.hip runs the same schedule on images of mixed sizes):
//
//   speculate   every lane but the last decodes its chunk from the guess (first bit, block 0 of an MCU, DC next),
//               without writing, and keeps its exit state and what the chunk owns;
//   settle      rounds of: exits to LDS, barrier, every lane reads its left neighbour's exit and, if that differs from
//               the entry it last used, decodes again from it; barrier-or over "my entry changed".  Lane 0's entry is
//               the segment's own, so after round r the entry of lane r + 1 is final: at most `lanes` rounds, and
//               Huffman streams resynchronise after a few symbols, so in practice a handful;
//   scan        an exclusive prefix over the lanes (LDS, log2 steps) of the DC symbols and the three DC sums:
//               each lane's first block in scan order and the predictors at its entry;
//   write       every lane decodes its chunk once more from its final entry, strictly, into the zeroed coefficients;
//               the segment's status is that of the first lane in scan order that reports one (a tree minimum).
//
// Every lane of the workgroup reaches every barrier (the loop bounds and the exit test are uniform); nothing waits on
// another workgroup, nothing spins on memory, no atomics.  jpeg_idct_kernel and jpeg_colour_kernel of jpeg.hip follow
// unchanged.  The result is that of jpeg_entropy_kernel bit for bit; behind a damaged block the lanes whose entries
// came from the tolerant speculation may leave other (bounded) garbage than the serial route leaves zeros.
#include "common.h"

#include "jpeg_kernels.h"
#include "jpeg_stages.h"

namespace oibl {

constexpr int JSCAN_MAX_DIM = 32768;

__constant__ uint8_t c_jscan_zigzag[64] = {JPEG_ZIGZAG_LIST};

// grid (max_segments, N), T threads: T a power of two, 64 <= T <= 1024
__global__ __launch_bounds__(JSCAN_MAX_LANES) void jscan_chunk_kernel(const uint8_t* bytes, uint32_t total_bytes,
                                                                      const uint8_t* records, const int32_t* segs,
                                                                      int S, int H, int W, int chunk_bytes,
                                                                      int16_t* coef, int32_t* seg_status,
                                                                      int32_t* seg_rounds) {
  __shared__ JpegHuff s_huff[4];
  __shared__ uint8_t s_zz[64];
  const int tid = threadIdx.x, k = blockIdx.x, n = blockIdx.y;
  const uint8_t* rec = records + (size_t)n * JPEG_REC_BYTES;
  const JpegGeom g = jpeg_geom(reinterpret_cast<const int32_t*>(rec), H, W);
  if (k >= g.nseg || g.seg_first > S - 1 - k) return;   // the whole workgroup
  if (tid < 4) jpeg_huff_build(&s_huff[tid], rec + JPEG_REC_HUFF + tid * JPEG_HUFF_BYTES);
  if (tid < 64) s_zz[tid] = c_jscan_zigzag[tid];
  __syncthreads();
  const size_t plane = (size_t)g.Bw * g.Bh * 64;
  jpeg_chunked_segment(bytes, total_bytes, g, segs, chunk_bytes, s_huff, s_zz, k, coef + (size_t)n * 3 * plane,
                       seg_status, seg_rounds);
}

struct JscanLayout {
  size_t coef, seg_status, seg_rounds, planes, zero_bytes, total;   // byte offsets; [coef, zero_bytes) is zeroed per call
};

static JscanLayout jscan_layout(int N, int H, int W, int S) {
  const size_t plane = (size_t)jpeg_blocks_across(W) * jpeg_blocks_across(H) * 64;
  JscanLayout l;
  size_t at = 0;
  l.coef = at, at += align_up((size_t)N * 3 * plane * sizeof(int16_t), 256);
  l.seg_status = at, at += align_up((size_t)S * sizeof(int32_t), 256);
  l.seg_rounds = at, at += align_up((size_t)S * sizeof(int32_t), 256);
  l.zero_bytes = at;
  l.planes = at, at += align_up((size_t)N * 3 * plane, 256);
  l.total = at;
  return l;
}

static bool jscan_shape_ok(int N, int H, int W, int S, int chunk_bytes) {
  return N > 0 && N <= 65535 && H >= 1 && W >= 8 && H <= JSCAN_MAX_DIM && W <= JSCAN_MAX_DIM && S >= N &&
         S <= (1 << 28) && chunk_bytes >= 4 && chunk_bytes <= 65536;
}

}  // namespace oibl

using namespace oibl;

extern "C" {

size_t oibl_jpeg_decode_chunked_workspace_bytes(int N, int H, int W, int S, int chunk_bytes) {
  if (!jscan_shape_ok(N, H, W, S, chunk_bytes)) return 0;
  return jscan_layout(N, H, W, S).total;
}

int oibl_jpeg_decode_chunked(const uint8_t* scan_bytes, size_t scan_len, const void* records, const int32_t* segments,
                             int S, int max_segments, int N, int H, int W, int chunk_bytes, uint8_t* out_nhwc,
                             int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  OIBL_REQUIRE(scan_bytes && records && segments && out_nhwc && status, "jpeg_decode_chunked: null pointer");
  OIBL_REQUIRE(chunk_bytes >= 4 && chunk_bytes <= 65536, "jpeg_decode_chunked: chunk_bytes %d must be in [4, 65536]",
               chunk_bytes);
  OIBL_REQUIRE(jscan_shape_ok(N, H, W, S, chunk_bytes),
               "jpeg_decode_chunked: bad shape N=%d H=%d W=%d S=%d (N <= 65535, 1 <= H <= %d, 8 <= W <= %d, "
               "N <= S <= 2^28)", N, H, W, S, JSCAN_MAX_DIM, JSCAN_MAX_DIM);
  OIBL_REQUIRE(scan_len >= 1 && scan_len <= 0x7fffffffu, "jpeg_decode_chunked: scan_len %zu must be in [1, 2^31)",
               scan_len);
  OIBL_REQUIRE(max_segments >= 1 && max_segments <= S,
               "jpeg_decode_chunked: max_segments %d must be in [1, S = %d]", max_segments, S);
  OIBL_REQUIRE((uintptr_t)records % 4 == 0 && (uintptr_t)segments % 4 == 0 && (uintptr_t)status % 4 == 0,
               "jpeg_decode_chunked: records, segments and status must be 4-byte aligned");
  OIBL_REQUIRE(ws && (uintptr_t)ws % 256 == 0, "jpeg_decode_chunked: workspace must be 256-byte aligned");
  const JscanLayout l = jscan_layout(N, H, W, S);
  if (ws_bytes < l.total) {
    set_error("jpeg_decode_chunked: workspace %zu < required %zu bytes", ws_bytes, l.total);
    return OIBL_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int16_t* coef = (int16_t*)((char*)ws + l.coef);
  int32_t* seg_status = (int32_t*)((char*)ws + l.seg_status);
  int32_t* seg_rounds = (int32_t*)((char*)ws + l.seg_rounds);
  uint8_t* planes = (uint8_t*)ws + l.planes;
  const uint8_t* rec = (const uint8_t*)records;
  // no segment is longer than the batch's bytes: as many threads as its chunks, a power of two from 64 to 1024
  const size_t chunks = (scan_len + (size_t)chunk_bytes - 1) / (size_t)chunk_bytes;
  unsigned threads = 64;
  while (threads < (unsigned)JSCAN_MAX_LANES && threads < chunks) threads <<= 1;
  OIBL_HIP_CHECK(hipMemsetAsync(coef, 0, l.zero_bytes, st));
  hipLaunchKernelGGL(jscan_chunk_kernel, dim3((unsigned)max_segments, (unsigned)N), dim3(threads), 0, st, scan_bytes,
                     (uint32_t)scan_len, rec, segments, S, H, W, chunk_bytes, coef, seg_status, seg_rounds);
  OIBL_LAUNCH_CHECK();
  const int Bw = jpeg_blocks_across(W), Bh = jpeg_blocks_across(H);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((Bw * Bh + 255) / 256), 3u, (unsigned)N), dim3(256), 0, st, rec,
                     (const int16_t*)coef, H, W, planes);
  OIBL_LAUNCH_CHECK();
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4), (unsigned)N),
                     dim3(64, 4), 0, st, rec, (const uint8_t*)planes, (const int32_t*)seg_status, S, H, W, out_nhwc,
                     status);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

}  // extern "C"
