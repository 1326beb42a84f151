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
// or a workgroup does in each stage is the text of jpeg_stages.h; the kernels here say only where an image's H, W and
// slices come from.
//
// The chunked route (jscan_chunk_kernel, oibl_jpeg_decode_chunked): the entropy stage with many lanes per segment, for
// scans without restart markers (one lane per image on the serial route).  A segment is cut into chunks of
// `chunk_bytes` raw bytes; ONE workgroup serves it, a lane per chunk, at most 1024 (the last lane takes what is left).
// The state machine is the shared text of jpeg_chunked.h; its schedule is jpeg_chunked_segment of jpeg_stages.h:
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
// another workgroup, nothing spins on memory, no atomics.  The IDCT and colour stages follow unchanged.  The result is
// that of the serial route bit for bit; behind a damaged block the lanes whose entries came from the tolerant
// speculation may leave other (bounded) garbage than the serial route leaves zeros.
//
// A batch of MIXED stored sizes (the jmix_* kernels, oibl_jpeg_decode_mixed): the same stages and both entropy routes
// with every image's H, W and base offsets taken from a per-image geometry table (jpeg_mixed.h) instead of kernel
// arguments.  All images' segments decode in ONE entropy launch, and the colour stage writes image n as a contiguous
// [H_n][W_n][3] block at its byte offset of one packed uint8 buffer, which csrc/resize.hip (oibl_resize_u8_mixed) reads
// into the dense batch.
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
// indexed exactly as in the uniform decoder.  Nothing of one image reaches another.
//
// The host side of all three entries is one driver, jpeg_decode_run: the checks they share, the workspace layout, the
// memset and the launch sequence.  An entry supplies its kernels and what they take in place of H and W.
#include "common.h"

#include "jpeg_mixed.h"
#include "jpeg_stages.h"

namespace oibl {

constexpr int JPEG_MAX_DIM = 32768;

__constant__ uint8_t c_jpeg_zigzag[64] = {JPEG_ZIGZAG_LIST};

// ---- one stored size ------------------------------------------------------------------------------------------------
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
  if (tid < 64) s_zz[tid] = c_jpeg_zigzag[tid];
  __syncthreads();
  const size_t plane = (size_t)g.Bw * g.Bh * 64;
  jpeg_chunked_segment(bytes, total_bytes, g, segs, chunk_bytes, s_huff, s_zz, k, coef + (size_t)n * 3 * plane,
                       seg_status, seg_rounds);
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

// ---- mixed stored sizes ---------------------------------------------------------------------------------------------
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
  s_zz[tid] = c_jpeg_zigzag[tid];
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
  if (tid < 64) s_zz[tid] = c_jpeg_zigzag[tid];
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

// ---- the host side: one driver --------------------------------------------------------------------------------------
// What the three entries are given alike.
struct JpegCall {
  const char* name;   // the entry's: the prefix of its messages
  const uint8_t* scan_bytes;
  size_t scan_len;
  const void* records;
  const int32_t* segments;
  int S, max_segments, N;
  int chunk_bytes;    // 0: the serial route
  bool rounds;        // does the entry's workspace hold the rounds of the chunked route?
  void* out;
  int32_t* status;
  void* ws;
  size_t ws_bytes;
  void* stream;
};

// The workspace: coef | seg_status | [seg_rounds] | planes, as byte offsets; [coef, zero_bytes) is zeroed per call.
struct JpegLayout {
  size_t coef, seg_status, seg_rounds, planes, zero_bytes, total;
};

static JpegLayout jpeg_layout(size_t coef_bytes, size_t plane_bytes, int S, bool rounds) {
  const size_t per_segment = align_up((size_t)S * sizeof(int32_t), 256);
  JpegLayout l;
  size_t at = 0;
  l.coef = at, at += align_up(coef_bytes, 256);
  l.seg_status = at, at += per_segment;
  l.seg_rounds = at, at += rounds ? per_segment : 0;
  l.zero_bytes = at;
  l.planes = at, at += align_up(plane_bytes, 256);
  l.total = at;
  return l;
}

// Lanes of the chunked launch.  No segment is longer than the batch's bytes: as many threads as its chunks, a power of
// two from 64 to 1024.
static unsigned jpeg_chunk_lanes(size_t scan_len, int chunk_bytes) {
  const size_t chunks = (scan_len + (size_t)chunk_bytes - 1) / (size_t)chunk_bytes;
  unsigned threads = 64;
  while (threads < (unsigned)JSCAN_MAX_LANES && threads < chunks) threads <<= 1;
  return threads;
}

static bool jpeg_batch_ok(int N, int S) { return N > 0 && N <= 65535 && S >= N && S <= (1 << 28); }

static bool jpeg_shape_ok(int N, int H, int W, int S) {
  return jpeg_batch_ok(N, S) && H >= 1 && W >= 8 && H <= JPEG_MAX_DIM && W <= JPEG_MAX_DIM;
}

static bool jpeg_chunk_bytes_ok(int chunk_bytes) { return chunk_bytes >= 4 && chunk_bytes <= 65536; }

// The kernels of a batch of one stored size: H and W are kernel arguments.
struct JpegUniform {
  int H, W;

  size_t plane_bytes(int N) const { return (size_t)N * 3 * jpeg_blocks_across(W) * jpeg_blocks_across(H) * 64; }
  bool pointers() const { return true; }   // no table: nothing more to be null or misaligned
  bool aligned() const { return true; }
  const char* aligned_too() const { return ""; }

  int shape(const JpegCall& c) {
    OIBL_REQUIRE(!c.rounds || jpeg_chunk_bytes_ok(c.chunk_bytes), "%s: chunk_bytes %d must be in [4, 65536]", c.name,
                 c.chunk_bytes);
    OIBL_REQUIRE(jpeg_shape_ok(c.N, H, W, c.S),
                 "%s: bad shape N=%d H=%d W=%d S=%d (N <= 65535, 1 <= H <= %d, 8 <= W <= %d, N <= S <= 2^28)", c.name,
                 c.N, H, W, c.S, JPEG_MAX_DIM, JPEG_MAX_DIM);
    return OIBL_OK;
  }
  void entropy(const JpegCall& c, dim3 grid, dim3 block, hipStream_t st, int16_t* coef, int32_t* seg_status,
               int32_t* seg_rounds) const {
    const uint8_t* rec = (const uint8_t*)c.records;
    if (c.chunk_bytes == 0)
      hipLaunchKernelGGL(jpeg_entropy_kernel, grid, block, 0, st, c.scan_bytes, (uint32_t)c.scan_len, rec, c.segments,
                         c.S, H, W, coef, seg_status);
    else
      hipLaunchKernelGGL(jscan_chunk_kernel, grid, block, 0, st, c.scan_bytes, (uint32_t)c.scan_len, rec, c.segments,
                         c.S, H, W, c.chunk_bytes, coef, seg_status, seg_rounds);
  }
  void idct(const JpegCall& c, hipStream_t st, const int16_t* coef, uint8_t* planes) const {
    const int Bw = jpeg_blocks_across(W), Bh = jpeg_blocks_across(H);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((Bw * Bh + 255) / 256), 3u, (unsigned)c.N), dim3(256), 0, st,
                       (const uint8_t*)c.records, coef, H, W, planes);
  }
  void colour(const JpegCall& c, hipStream_t st, const uint8_t* planes, const int32_t* seg_status) const {
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4), (unsigned)c.N),
                       dim3(64, 4), 0, st, (const uint8_t*)c.records, planes, seg_status, c.S, H, W,
                       (uint8_t*)c.out, c.status);
  }
};

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

// The kernels of a batch of mixed stored sizes: they read the geometry table against the call's totals.
struct JpegMixed {
  const int32_t* geom_dev;
  const size_t* totals;
  JpegMixSpaces sp;   // of the totals, once shape() has accepted them

  size_t plane_bytes(int) const { return totals[JPEG_MIX_T_PLANE_BYTES]; }
  bool pointers() const { return geom_dev && totals; }
  bool aligned() const { return (uintptr_t)geom_dev % 4 == 0; }
  const char* aligned_too() const { return ", geom_dev"; }

  int shape(const JpegCall& c) {
    OIBL_REQUIRE(c.chunk_bytes == 0 || jpeg_chunk_bytes_ok(c.chunk_bytes),
                 "%s: chunk_bytes %d must be 0 (the serial route) or in [4, 65536]", c.name, c.chunk_bytes);
    OIBL_REQUIRE(jpeg_batch_ok(c.N, c.S), "%s: bad shape N=%d S=%d (N <= 65535, N <= S <= 2^28)", c.name, c.N, c.S);
    OIBL_REQUIRE(jmix_totals_ok(totals),
                 "%s: the totals are not those of a layout (coefficient bytes %zu, plane bytes %zu, pixel "
                 "bytes %zu < 2^40, largest Bw * Bh %zu, largest H %zu and W %zu <= %d)", c.name,
                 totals[JPEG_MIX_T_COEF_BYTES], totals[JPEG_MIX_T_PLANE_BYTES], totals[JPEG_MIX_T_PIXEL_BYTES],
                 totals[JPEG_MIX_T_MAX_BLOCKS], totals[JPEG_MIX_T_MAX_H], totals[JPEG_MIX_T_MAX_W], JPEG_MIX_MAX_DIM);
    sp.plane_blocks = totals[JPEG_MIX_T_PLANE_BYTES] / 64;
    sp.coef_blocks = sp.plane_blocks;
    sp.pixel_bytes = totals[JPEG_MIX_T_PIXEL_BYTES];
    sp.max_blocks = (int)totals[JPEG_MIX_T_MAX_BLOCKS];
    sp.max_h = (int)totals[JPEG_MIX_T_MAX_H];
    sp.max_w = (int)totals[JPEG_MIX_T_MAX_W];
    return OIBL_OK;
  }
  void entropy(const JpegCall& c, dim3 grid, dim3 block, hipStream_t st, int16_t* coef, int32_t* seg_status,
               int32_t* seg_rounds) const {
    const uint8_t* rec = (const uint8_t*)c.records;
    if (c.chunk_bytes == 0)
      hipLaunchKernelGGL(jmix_entropy_kernel, grid, block, 0, st, c.scan_bytes, (uint32_t)c.scan_len, rec, c.segments,
                         c.S, geom_dev, sp, coef, seg_status);
    else
      hipLaunchKernelGGL(jmix_chunk_kernel, grid, block, 0, st, c.scan_bytes, (uint32_t)c.scan_len, rec, c.segments,
                         c.S, geom_dev, sp, c.chunk_bytes, coef, seg_status, seg_rounds);
  }
  void idct(const JpegCall& c, hipStream_t st, const int16_t* coef, uint8_t* planes) const {
    hipLaunchKernelGGL(jmix_idct_kernel, dim3((unsigned)((sp.max_blocks + 255) / 256), 3u, (unsigned)c.N), dim3(256),
                       0, st, (const uint8_t*)c.records, geom_dev, sp, coef, planes);
  }
  void colour(const JpegCall& c, hipStream_t st, const uint8_t* planes, const int32_t* seg_status) const {
    hipLaunchKernelGGL(jmix_colour_kernel,
                       dim3((unsigned)((sp.max_w + 63) / 64), (unsigned)((sp.max_h + 3) / 4), (unsigned)c.N),
                       dim3(64, 4), 0, st, (const uint8_t*)c.records, geom_dev, sp, planes, seg_status, c.S,
                       (uint8_t*)c.out, c.status);
  }
};

// What the three entries refuse alike, with the entry's own shape check at its place among them; the layout of an
// accepted call.
template <class Kernels>
static int jpeg_check(const JpegCall& c, Kernels& k, JpegLayout& l) {
  OIBL_REQUIRE(c.scan_bytes && c.records && c.segments && k.pointers() && c.out && c.status, "%s: null pointer",
               c.name);
  if (const int refused = k.shape(c)) return refused;
  OIBL_REQUIRE(c.scan_len >= 1 && c.scan_len <= 0x7fffffffu, "%s: scan_len %zu must be in [1, 2^31)", c.name,
               c.scan_len);
  OIBL_REQUIRE(c.max_segments >= 1 && c.max_segments <= c.S, "%s: max_segments %d must be in [1, S = %d]", c.name,
               c.max_segments, c.S);
  OIBL_REQUIRE(
      (uintptr_t)c.records % 4 == 0 && (uintptr_t)c.segments % 4 == 0 && (uintptr_t)c.status % 4 == 0 && k.aligned(),
      "%s: records, segments%s and status must be 4-byte aligned", c.name, k.aligned_too());
  OIBL_REQUIRE(c.ws && (uintptr_t)c.ws % 256 == 0, "%s: workspace must be 256-byte aligned", c.name);
  const size_t planes = k.plane_bytes(c.N);
  l = jpeg_layout(planes * sizeof(int16_t), planes, c.S, c.rounds);
  if (c.ws_bytes < l.total) {
    set_error("%s: workspace %zu < required %zu bytes", c.name, c.ws_bytes, l.total);
    return OIBL_E_WORKSPACE;
  }
  return OIBL_OK;
}

// A decode call: the checks, then memset, entropy (serial or chunked), IDCT, colour on the caller's stream.
template <class Kernels>
static int jpeg_decode_run(const JpegCall& c, Kernels k) {
  JpegLayout l;
  if (const int refused = jpeg_check(c, k, l)) return refused;
  hipStream_t st = (hipStream_t)c.stream;
  int16_t* coef = (int16_t*)((char*)c.ws + l.coef);
  int32_t* seg_status = (int32_t*)((char*)c.ws + l.seg_status);
  int32_t* seg_rounds = (int32_t*)((char*)c.ws + l.seg_rounds);
  uint8_t* planes = (uint8_t*)c.ws + l.planes;
  OIBL_HIP_CHECK(hipMemsetAsync(coef, 0, l.zero_bytes, st));
  if (c.chunk_bytes == 0)
    k.entropy(c, dim3((unsigned)((c.max_segments + 63) / 64), (unsigned)c.N), dim3(64), st, coef, seg_status,
              seg_rounds);
  else
    k.entropy(c, dim3((unsigned)c.max_segments, (unsigned)c.N), dim3(jpeg_chunk_lanes(c.scan_len, c.chunk_bytes)), st,
              coef, seg_status, seg_rounds);
  OIBL_LAUNCH_CHECK();
  k.idct(c, st, coef, planes);
  OIBL_LAUNCH_CHECK();
  k.colour(c, st, planes, seg_status);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

}  // namespace oibl

using namespace oibl;

extern "C" {

size_t oibl_jpeg_decode_workspace_bytes(int N, int H, int W, int S) {
  if (!jpeg_shape_ok(N, H, W, S)) return 0;
  const size_t planes = JpegUniform{H, W}.plane_bytes(N);
  return jpeg_layout(planes * sizeof(int16_t), planes, S, false).total;
}

int oibl_jpeg_decode(const uint8_t* scan_bytes, size_t scan_len, const void* records, const int32_t* segments, int S,
                     int max_segments, int N, int H, int W, uint8_t* out_nhwc, int32_t* status, void* ws,
                     size_t ws_bytes, void* stream) {
  const JpegCall c = {"jpeg_decode", scan_bytes, scan_len, records, segments, S, max_segments, N, 0, false,
                      out_nhwc, status, ws, ws_bytes, stream};
  return jpeg_decode_run(c, JpegUniform{H, W});
}

size_t oibl_jpeg_decode_chunked_workspace_bytes(int N, int H, int W, int S, int chunk_bytes) {
  if (!jpeg_shape_ok(N, H, W, S) || !jpeg_chunk_bytes_ok(chunk_bytes)) return 0;
  const size_t planes = JpegUniform{H, W}.plane_bytes(N);
  return jpeg_layout(planes * sizeof(int16_t), planes, S, true).total;
}

int oibl_jpeg_decode_chunked(const uint8_t* scan_bytes, size_t scan_len, const void* records, const int32_t* segments,
                             int S, int max_segments, int N, int H, int W, int chunk_bytes, uint8_t* out_nhwc,
                             int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  const JpegCall c = {"jpeg_decode_chunked", scan_bytes, scan_len, records, segments, S, max_segments, N, chunk_bytes,
                      true, out_nhwc, status, ws, ws_bytes, stream};
  return jpeg_decode_run(c, JpegUniform{H, W});
}

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
  if (!totals_host || !jpeg_batch_ok(N, S) || !jmix_totals_ok(totals_host)) return 0;
  return jpeg_layout(totals_host[JPEG_MIX_T_COEF_BYTES], totals_host[JPEG_MIX_T_PLANE_BYTES], S, true).total;
}

int oibl_jpeg_decode_mixed(const uint8_t* scan_bytes, size_t scan_len, const void* records, const int32_t* segments,
                           int S, int max_segments, int N, const int32_t* geom_dev, const size_t* totals_host,
                           int chunk_bytes, uint8_t* out_packed, int32_t* status, void* ws, size_t ws_bytes,
                           void* stream) {
  const JpegCall c = {"jpeg_decode_mixed", scan_bytes, scan_len, records, segments, S, max_segments, N, chunk_bytes,
                      true, out_packed, status, ws, ws_bytes, stream};
  return jpeg_decode_run(c, JpegMixed{geom_dev, totals_host, {}});
}

}  // extern "C"
