// Baseline JPEG decoding on the device: from the packed scan bytes of a batch to [N][H][W][3] uint8 with the bits of
// libjpeg-turbo as Pillow uses it (`Image.open(f).convert('RGB')`, the host step of ibl/utils/data/preprocessor.py).
// The markers are parsed on the host (openibl_amd/jpeg.py): per image a record with the component layout, the
// quantisation and Huffman tables and the restart interval, and per batch a table of segments — a restart interval, or
// the whole scan of an image without restarts.  Three stream-ordered launches behind one memset:
//
//   jpeg_entropy_kernel   one workgroup of ONE wave per 64 segments of one image; it builds the image's four Huffman
//                         tables in LDS (an 8-bit lookahead plus maxcode / valoff per length), then every lane decodes
//                         one segment with the shared text of jpeg_entropy.h into int16 coefficients, natural order,
//                         in the zeroed workspace: coef[N][3][Bh][Bw][64].  A segment's status goes to its own slot.
//   jpeg_idct_kernel      one thread per 8 x 8 block: coef * q in int32, libjpeg's "islow" IDCT (CONST_BITS 13,
//                         PASS1_BITS 2, columns first) entirely in registers, + 128, clamp, eight 8-byte stores into
//                         the MCU-padded component planes planes[N][3][Bh * 8][Bw * 8].
//   jpeg_colour_kernel    one thread per output pixel: the chroma sample by libjpeg's "fancy" h2v1 / h2v2 upsampling on
//                         the cropped plane with replicated edges, then YCbCr -> RGB in 16-bit fixed point.  Its first
//                         workgroup per image folds the image's segment statuses into status[n].
//
// All integer, no atomics: identical bits from run to run; an image's result depends on its own record, segments and
// bytes only.  Every index is bounded by construction (jpeg_entropy.h says how for the first stage; the other two
// index by the batch's H x W and the record's factors, which jpeg_geom forces into their ranges).  What a lane, a thread
// or a workgroup does in each stage is the text of jpeg_stages.h, shared with csrc/jpeg_mixed.hip.
#include "common.h"

#include "jpeg_stages.h"

namespace oibl {

constexpr int JPEG_MAX_DIM = 32768;

__constant__ uint8_t c_jpeg_zigzag[64] = {JPEG_ZIGZAG_LIST};

// grid (ceil(max_segments / 64), N), 64 threads
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* bytes, uint32_t total_bytes,
                                                          const uint8_t* records, const int32_t* segs, int S, int H,
                                                          int W, int16_t* coef, int32_t* seg_status) {
  __shared__ JpegHuff s_huff[4];
  __shared__ uint8_t s_zz[64];
  const int tid = threadIdx.x, n = blockIdx.y;
  const uint8_t* rec = records + (size_t)n * JPEG_REC_BYTES;
  const JpegGeom g = jpeg_geom(reinterpret_cast<const int32_t*>(rec), H, W);
  if ((int)blockIdx.x * 64 >= g.nseg) return;   // the whole workgroup
  if (tid < 4) jpeg_huff_build(&s_huff[tid], rec + JPEG_REC_HUFF + tid * JPEG_HUFF_BYTES);
  s_zz[tid] = c_jpeg_zigzag[tid];
  __syncthreads();
  const size_t plane = (size_t)g.Bw * g.Bh * 64;
  jpeg_entropy_lane(bytes, total_bytes, g, segs, S, s_huff, s_zz, blockIdx.x * 64 + tid,
                    coef + (size_t)n * 3 * plane, seg_status);
}

// grid (ceil(Bw * Bh / 256), 3, N), 256 threads
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const uint8_t* records, const int16_t* coef, int H, int W,
                                                        uint8_t* planes) {
  const int n = blockIdx.z;
  const uint8_t* rec = records + (size_t)n * JPEG_REC_BYTES;
  const JpegGeom g = jpeg_geom(reinterpret_cast<const int32_t*>(rec), H, W);
  const size_t image = (size_t)n * 3 * g.Bw * g.Bh * 64;
  const int c = blockIdx.y;
  if (c >= g.ncomp) return;   // the whole workgroup
  jpeg_idct_stage(rec, jpeg_idct_plane(g, c), c, blockIdx.x * 256 + threadIdx.x, coef + image, planes + image);
}

// grid (ceil(W / 64), ceil(H / 4), N), (64, 4) threads
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const uint8_t* records, const uint8_t* planes,
                                                          const int32_t* seg_status, int S, int H, int W,
                                                          uint8_t* out, int32_t* status) {
  __shared__ int s_max[4];
  const int n = blockIdx.z;
  const JpegGeom g = jpeg_geom(reinterpret_cast<const int32_t*>(records + (size_t)n * JPEG_REC_BYTES), H, W);
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x < W && y < H)
    jpeg_colour_pixel(g, planes + (size_t)n * 3 * g.Bw * g.Bh * 64, H, W, y, x,
                      out + (((size_t)n * H + y) * W + x) * 3);
  if (blockIdx.x == 0 && blockIdx.y == 0) jpeg_image_status(g, seg_status, S, s_max, status + n);
}

struct JpegLayout {
  size_t coef, seg_status, planes, zero_bytes, total;   // byte offsets; [coef, coef + zero_bytes) is zeroed per call
};

static JpegLayout jpeg_layout(int N, int H, int W, int S) {
  const size_t plane = (size_t)jpeg_blocks_across(W) * jpeg_blocks_across(H) * 64;
  JpegLayout l;
  size_t at = 0;
  l.coef = at, at += align_up((size_t)N * 3 * plane * sizeof(int16_t), 256);
  l.seg_status = at, at += align_up((size_t)S * sizeof(int32_t), 256);
  l.zero_bytes = at;
  l.planes = at, at += align_up((size_t)N * 3 * plane, 256);
  l.total = at;
  return l;
}

static bool jpeg_shape_ok(int N, int H, int W, int S) {
  return N > 0 && N <= 65535 && H >= 1 && W >= 8 && H <= JPEG_MAX_DIM && W <= JPEG_MAX_DIM && S >= N &&
         S <= (1 << 28);
}

}  // namespace oibl

using namespace oibl;

extern "C" {

size_t oibl_jpeg_decode_workspace_bytes(int N, int H, int W, int S) {
  if (!jpeg_shape_ok(N, H, W, S)) return 0;
  return jpeg_layout(N, H, W, S).total;
}

int oibl_jpeg_decode(const uint8_t* scan_bytes, size_t scan_len, const void* records, const int32_t* segments, int S,
                     int max_segments, int N, int H, int W, uint8_t* out_nhwc, int32_t* status, void* ws,
                     size_t ws_bytes, void* stream) {
  OIBL_REQUIRE(scan_bytes && records && segments && out_nhwc && status, "jpeg_decode: null pointer");
  OIBL_REQUIRE(jpeg_shape_ok(N, H, W, S),
               "jpeg_decode: bad shape N=%d H=%d W=%d S=%d (N <= 65535, 1 <= H <= %d, 8 <= W <= %d, N <= S <= 2^28)",
               N, H, W, S, JPEG_MAX_DIM, JPEG_MAX_DIM);
  OIBL_REQUIRE(scan_len >= 1 && scan_len <= 0x7fffffffu, "jpeg_decode: scan_len %zu must be in [1, 2^31)", scan_len);
  OIBL_REQUIRE(max_segments >= 1 && max_segments <= S,
               "jpeg_decode: max_segments %d must be in [1, S = %d]", max_segments, S);
  OIBL_REQUIRE((uintptr_t)records % 4 == 0 && (uintptr_t)segments % 4 == 0 && (uintptr_t)status % 4 == 0,
               "jpeg_decode: records, segments and status must be 4-byte aligned");
  OIBL_REQUIRE(ws && (uintptr_t)ws % 256 == 0, "jpeg_decode: workspace must be 256-byte aligned");
  const JpegLayout l = jpeg_layout(N, H, W, S);
  if (ws_bytes < l.total) {
    set_error("jpeg_decode: workspace %zu < required %zu bytes", ws_bytes, l.total);
    return OIBL_E_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  int16_t* coef = (int16_t*)((char*)ws + l.coef);
  int32_t* seg_status = (int32_t*)((char*)ws + l.seg_status);
  uint8_t* planes = (uint8_t*)ws + l.planes;
  const uint8_t* rec = (const uint8_t*)records;
  OIBL_HIP_CHECK(hipMemsetAsync(coef, 0, l.zero_bytes, st));
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((max_segments + 63) / 64), (unsigned)N), dim3(64), 0, st,
                     scan_bytes, (uint32_t)scan_len, rec, segments, S, H, W, coef, seg_status);
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
