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
// index by the batch's H x W and the record's factors, which jpeg_geom forces into their ranges).
#include "common.h"

#include "jpeg_entropy.h"

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
  const int k = blockIdx.x * 64 + tid;
  if (k >= g.nseg || g.seg_first > S - 1 - k) return;
  const int sidx = g.seg_first + k;
  const int total = g.mcus_x * g.mcus_y;
  const int want = jpeg_segments_wanted(total, g.dri);
  const int32_t sb = segs[2 * sidx], se = segs[2 * sidx + 1];
  const uint32_t begin = sb > 0 ? (uint32_t)sb : 0u, end = se > 0 ? (uint32_t)se : 0u;
  const size_t plane = (size_t)g.Bw * g.Bh * 64;
  seg_status[sidx] = jpeg_decode_segment(bytes, begin, end, total_bytes, g, s_huff, s_zz, g.dri ? k * g.dri : 0,
                                         g.dri ? g.dri : total, (g.dri && k + 1 < want) ? (k & 7) : -1,
                                         coef + (size_t)n * 3 * plane);
}

// one pass of the IDCT over eight values; SHIFT = 11 (columns) or 18 (rows).  The sums are formed in unsigned
// arithmetic — the same bits as libjpeg's int32 wherever that does not overflow, and defined where a damaged stream
// makes it wrap — and descaled with an arithmetic shift.
template <int SHIFT>
__device__ static inline void jpeg_idct8(int i0, int i1, int i2, int i3, int i4, int i5, int i6, int i7, int (&o)[8]) {
  typedef unsigned U;
  const U x0 = (U)i0, x1 = (U)i1, x2 = (U)i2, x3 = (U)i3, x4 = (U)i4, x5 = (U)i5, x6 = (U)i6, x7 = (U)i7;
  U z1 = (x2 + x6) * 4433u;
  const U t2 = z1 - x6 * 15137u, t3 = z1 + x2 * 6270u;
  const U t0 = (x0 + x4) << 13, t1 = (x0 - x4) << 13;
  const U t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  U u0 = x7, u1 = x5, u2 = x3, u3 = x1;
  z1 = u0 + u3;
  U z2 = u1 + u2, z3 = u0 + u2, z4 = u1 + u3;
  const U z5 = (z3 + z4) * 9633u;
  u0 *= 2446u, u1 *= 16819u, u2 *= 25172u, u3 *= 12299u;
  z1 *= (U)-7373, z2 *= (U)-20995;
  z3 = z3 * (U)-16069 + z5, z4 = z4 * (U)-3196 + z5;
  u0 += z1 + z3, u1 += z2 + z4, u2 += z2 + z3, u3 += z1 + z4;
  constexpr U R = 1u << (SHIFT - 1);
  o[0] = (int)(t10 + u3 + R) >> SHIFT, o[7] = (int)(t10 - u3 + R) >> SHIFT;
  o[1] = (int)(t11 + u2 + R) >> SHIFT, o[6] = (int)(t11 - u2 + R) >> SHIFT;
  o[2] = (int)(t12 + u1 + R) >> SHIFT, o[5] = (int)(t12 - u1 + R) >> SHIFT;
  o[3] = (int)(t13 + u0 + R) >> SHIFT, o[4] = (int)(t13 - u0 + R) >> SHIFT;
}

__device__ static inline unsigned jpeg_clamp8(int v) { return (unsigned)min(max(v, 0), 255); }

// grid (ceil(Bw * Bh / 256), 3, N), 256 threads
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const uint8_t* records, const int16_t* coef, int H, int W,
                                                        uint8_t* planes) {
  __shared__ int s_q[64];
  const int c = blockIdx.y, n = blockIdx.z;
  const uint8_t* rec = records + (size_t)n * JPEG_REC_BYTES;
  const JpegGeom g = jpeg_geom(reinterpret_cast<const int32_t*>(rec), H, W);
  if (c >= g.ncomp) return;
  const int tq = c == 0 ? g.tq[0] : (c == 1 ? g.tq[1] : g.tq[2]);   // (a register select: no indexed array)
  if (threadIdx.x < 64) s_q[threadIdx.x] = rec[JPEG_REC_QT + tq * 64 + threadIdx.x];
  __syncthreads();
  const int blk = blockIdx.x * 256 + threadIdx.x;
  const int by = blk / g.Bw, bx = blk - by * g.Bw;
  if (bx >= g.mcus_x * (c == 0 ? g.hs : 1) || by >= g.mcus_y * (c == 0 ? g.vs : 1)) return;
  const size_t plane = (size_t)g.Bw * g.Bh * 64;
  const int16_t* src = coef + ((size_t)n * 3 + c) * plane + (size_t)blk * 64;
  int x[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint4 w = reinterpret_cast<const uint4*>(src)[i];
    const unsigned u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[8 * i + 2 * j] = (int)(int16_t)(u[j] & 0xFFFFu) * s_q[8 * i + 2 * j];
      x[8 * i + 2 * j + 1] = (int)(int16_t)(u[j] >> 16) * s_q[8 * i + 2 * j + 1];
    }
  }
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    int o[8];
    jpeg_idct8<11>(x[col], x[8 + col], x[16 + col], x[24 + col], x[32 + col], x[40 + col], x[48 + col], x[56 + col],
                   o);
#pragma unroll
    for (int r = 0; r < 8; ++r) x[8 * r + col] = o[r];
  }
  const int Wp = g.Bw * 8;
  uint8_t* dst = planes + ((size_t)n * 3 + c) * plane + (size_t)by * 8 * Wp + bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int o[8];
    jpeg_idct8<18>(x[8 * r], x[8 * r + 1], x[8 * r + 2], x[8 * r + 3], x[8 * r + 4], x[8 * r + 5], x[8 * r + 6],
                   x[8 * r + 7], o);
    uint2 px;
    px.x = jpeg_clamp8(o[0] + 128) | jpeg_clamp8(o[1] + 128) << 8 | jpeg_clamp8(o[2] + 128) << 16 |
           jpeg_clamp8(o[3] + 128) << 24;
    px.y = jpeg_clamp8(o[4] + 128) | jpeg_clamp8(o[5] + 128) << 8 | jpeg_clamp8(o[6] + 128) << 16 |
           jpeg_clamp8(o[7] + 128) << 24;
    *reinterpret_cast<uint2*>(dst + (size_t)r * Wp) = px;
  }
}

// The chroma sample at output pixel (y, x) of a plane p with row stride Wp, cropped to ch x cw, replicated edges.
__device__ static inline int jpeg_chroma(const uint8_t* p, int Wp, int cw, int ch, int hs, int vs, int y, int x) {
  if (hs == 1) return p[(size_t)y * Wp + x];
  const int c = x >> 1, side = (x & 1) ? min(c + 1, cw - 1) : max(c - 1, 0);
  if (vs == 1) {
    const uint8_t* row = p + (size_t)y * Wp;
    return (3 * row[c] + row[side] + 1 + (x & 1)) >> 2;
  }
  const int r = y >> 1, nb = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
  const uint8_t *row = p + (size_t)r * Wp, *other = p + (size_t)nb * Wp;
  const int t = 3 * row[c] + other[c], ts = 3 * row[side] + other[side];
  return (3 * t + ts + 8 - (x & 1)) >> 4;
}

// grid (ceil(W / 64), ceil(H / 4), N), (64, 4) threads
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const uint8_t* records, const uint8_t* planes,
                                                          const int32_t* seg_status, int S, int H, int W,
                                                          uint8_t* out, int32_t* status) {
  __shared__ int s_max[4];
  const int n = blockIdx.z;
  const JpegGeom g = jpeg_geom(reinterpret_cast<const int32_t*>(records + (size_t)n * JPEG_REC_BYTES), H, W);
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x < W && y < H) {
    const int Wp = g.Bw * 8;
    const size_t plane = (size_t)g.Bw * g.Bh * 64;
    const uint8_t* py = planes + (size_t)n * 3 * plane;
    const int Y = py[(size_t)y * Wp + x];
    int R = Y, G = Y, B = Y;
    if (g.ncomp == 3) {
      const int cw = (W + g.hs - 1) / g.hs, ch = (H + g.vs - 1) / g.vs;
      const int cb = jpeg_chroma(py + plane, Wp, cw, ch, g.hs, g.vs, y, x) - 128;
      const int cr = jpeg_chroma(py + 2 * plane, Wp, cw, ch, g.hs, g.vs, y, x) - 128;
      R = (int)jpeg_clamp8(Y + ((91881 * cr + 32768) >> 16));
      G = (int)jpeg_clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
      B = (int)jpeg_clamp8(Y + ((116130 * cb + 32768) >> 16));
    }
    uint8_t* o = out + (((size_t)n * H + y) * W + x) * 3;
    o[0] = (uint8_t)R, o[1] = (uint8_t)G, o[2] = (uint8_t)B;
  }
  if (blockIdx.x == 0 && blockIdx.y == 0) {   // the image's status: the largest of its segments', or the host's
    const int tid = threadIdx.y * 64 + threadIdx.x;
    int m = 0;
    for (int k = tid; k < g.nseg && g.seg_first <= S - 1 - k; k += 256) m = max(m, seg_status[g.seg_first + k]);
    m = max(m, __shfl_xor(m, 32, 64));
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
    if (threadIdx.x == 0) s_max[threadIdx.y] = m;
    __syncthreads();
    if (tid == 0)
      status[n] = g.host_status ? g.host_status : max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
  }
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
