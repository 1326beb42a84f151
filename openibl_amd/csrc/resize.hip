// Bilinear resize of raw uint8 batches (the reference's Resize: img.resize((w, h), Image.BILINEAR) on the host,
// ibl/utils/data/__init__.py of the reference), optionally fused with ToTensor + Normalize.
//
// The arithmetic is PIL's 8-bit resampling (resize_tables.h): per axis a table of windows and 22-bit fixed-point
// weights computed in IEEE double, then two integer passes, horizontal first, with a uint8 intermediate:
//   byte = clip(((1 << 21) + sum over the window of coeff * source byte) >> 22, 0, 255)
// The uint8 result equals PIL's bit for bit.
//
//   resize_table_kernel   one thread per output coordinate of one axis: bounds[out][2] = {xmin, n} and
//                         coeff[out][ksize] into the caller's workspace (the tables are too large for kernel
//                         arguments, and building them on the device keeps the call stream-ordered: no host
//                         memory, no copy, nothing owned by the library, so it can be captured into a graph);
//   resize_kernel         ONE launch for both passes.  A workgroup owns a tile of RS_TILE_H x RS_TILE_W output
//                         pixels of one image.  It copies the tile's table rows to LDS, runs the horizontal pass
//                         for exactly the source rows its output rows read — from the window start of its first row
//                         to the window end of its last — into LDS as uint8 [rows][RS_TILE_W][3], and runs the
//                         vertical pass out of LDS.
// All integer, no atomics: identical bits from run to run, and nothing of one image reaches another.
//
// A row of a tile is RS_TILE_W * 3 = 192 bytes, three steps of a wave; a wave takes every fourth row.  In the
// horizontal pass lane j of a step owns byte j of the intermediate row (pixel j / 3, channel j % 3) and reads one
// source byte per tap: consecutive lanes read consecutive bytes at scale 1 and bytes `scale` apart beyond it, from
// any base alignment (a row of W * 3 bytes starts misaligned three times out of four: there is no dword path to
// take).  The vertical pass reads the intermediate by bytes — four lanes per bank word, which the LDS broadcasts —
// and stores 64 consecutive bytes per step (uint8 NHWC) or, with a lane per pixel and a step per channel, 256
// consecutive bytes per step (fp32 NCHW).
//
// LDS per workgroup is sized by the call (dynamic): the tile's table rows, (64 + 16) rows of ksize + 2 ints, and
// rs_tile_rows(vertical axis) rows of 192 bytes.  960 x 1280 -> 480 x 640: 36 rows, 9.2 KB, so the 32 waves of a CU
// are all resident; the most, at a factor of 16 on both axes, is 63 808 bytes (resize_tables.h), two workgroups per
// CU of 160 KiB.
#include "common.h"

// the tables are PIL's doubles, operation by operation: no fused multiply-add anywhere in this unit
#pragma clang fp contract(off)

#include "augment_pixel.h"
#include "jpeg_mixed.h"
#include "resize_tables.h"

namespace oibl {

constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_ROW_BYTES = RS_TILE_W * 3;
constexpr int RS_MAX_DIM = 32768;

// grid ceil(out_size / RS_THREADS)
__global__ __launch_bounds__(RS_THREADS) void resize_table_kernel(int in_size, int out_size, int32_t* bounds,
                                                                  int32_t* coeff) {
  const int xx = blockIdx.x * RS_THREADS + threadIdx.x;
  if (xx >= out_size) return;
  const ResizeAxis a = rs_axis(in_size, out_size);
  rs_table_row(a, in_size, xx, bounds + 2 * (size_t)xx, coeff + (size_t)xx * a.ksize);
}

struct ResizeGeom {
  int H, W, H2, W2;
  int ksh, ksv;    // entries per row of the horizontal / vertical coefficient table
  int rows_cap;    // rows of the intermediate in LDS: min(rs_tile_rows(vertical axis), H)
};

static size_t resize_lds_bytes(const ResizeGeom& g) {
  return (size_t)(RS_TILE_W * (g.ksh + 2) + RS_TILE_H * (g.ksv + 2)) * sizeof(int32_t) +
         (size_t)g.rows_cap * RS_ROW_BYTES;
}

// One tile of image n: blockIdx.x / blockIdx.y choose the tile, `img` is the image's [geo.H][geo.W][3] source and the
// four tables are ITS tables, rows of geo.ksh / geo.ksv entries (resize_kernel: the batch's; resize_mixed_kernel: the
// image's own, at the batch's largest row length).  Every thread of the workgroup calls it.
template <int OUT_KIND>
__device__ __forceinline__ void resize_tile(const uint8_t* img, const int32_t* bounds_h, const int32_t* coeff_h,
                                            const int32_t* bounds_v, const int32_t* coeff_v, void* out,
                                            const ResizeGeom& geo, int n, float m0, float m1, float m2, float s0,
                                            float s1, float s2) {
  extern __shared__ int32_t s_dyn[];   // resize_lds_bytes(geo)
  const int ksh = geo.ksh, ksv = geo.ksv;
  int32_t* s_ch = s_dyn;                         // [RS_TILE_W][ksh]
  int32_t* s_cv = s_ch + RS_TILE_W * ksh;        // [RS_TILE_H][ksv]
  int32_t* s_bh = s_cv + RS_TILE_H * ksv;        // [RS_TILE_W][2]
  int32_t* s_bv = s_bh + RS_TILE_W * 2;          // [RS_TILE_H][2]
  uint8_t* s_mid = reinterpret_cast<uint8_t*>(s_bv + RS_TILE_H * 2);   // [rows_cap][RS_TILE_W][3]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ox0 = blockIdx.x * RS_TILE_W, oy0 = blockIdx.y * RS_TILE_H;
  const int tw = min(RS_TILE_W, geo.W2 - ox0), th = min(RS_TILE_H, geo.H2 - oy0);

  for (int i = tid; i < tw * ksh; i += RS_THREADS) s_ch[i] = coeff_h[(size_t)ox0 * ksh + i];
  for (int i = tid; i < th * ksv; i += RS_THREADS) s_cv[i] = coeff_v[(size_t)oy0 * ksv + i];
  for (int i = tid; i < tw * 2; i += RS_THREADS) s_bh[i] = bounds_h[(size_t)ox0 * 2 + i];
  for (int i = tid; i < th * 2; i += RS_THREADS) s_bv[i] = bounds_v[(size_t)oy0 * 2 + i];
  __syncthreads();

  // the source rows this tile reads (window starts and ends grow with the row); rs_tile_rows bounds their number
  const int row0 = s_bv[0];
  const int rows = min(s_bv[2 * (th - 1)] + s_bv[2 * (th - 1) + 1] - row0, geo.rows_cap);
  const int row_bytes = tw * 3;

  // horizontal pass: source rows [row0, row0 + rows) -> s_mid [rows][RS_TILE_W][3]
  for (int r = wave; r < rows; r += RS_WAVES) {
    const uint8_t* src = img + (size_t)(row0 + r) * geo.W * 3;
    for (int j = lane; j < row_bytes; j += 64) {
      const int col = j / 3, c = j - col * 3;
      const int cnt = s_bh[2 * col + 1];
      const uint8_t* p = src + (size_t)s_bh[2 * col] * 3 + c;
      const int32_t* k = s_ch + col * ksh;
      int ss = 1 << (RS_PRECISION_BITS - 1);
      for (int t = 0; t < cnt; ++t) ss += k[t] * (int)p[3 * t];
      s_mid[r * RS_ROW_BYTES + j] = (uint8_t)rs_clip8(ss);
    }
  }
  __syncthreads();

  // vertical pass out of LDS
  const float mu[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
  for (int oy = wave; oy < th; oy += RS_WAVES) {
    const int cnt = s_bv[2 * oy + 1];
    const uint8_t* mid = s_mid + (s_bv[2 * oy] - row0) * RS_ROW_BYTES;
    const int32_t* k = s_cv + oy * ksv;
    const size_t row = (size_t)n * geo.H2 + (oy0 + oy);
    if (OUT_KIND == OIBL_JITTER_U8_NHWC) {
      uint8_t* dst = (uint8_t*)out + (row * geo.W2 + ox0) * 3;
      for (int j = lane; j < row_bytes; j += 64) {
        int ss = 1 << (RS_PRECISION_BITS - 1);
        for (int t = 0; t < cnt; ++t) ss += k[t] * (int)mid[t * RS_ROW_BYTES + j];
        dst[j] = (uint8_t)rs_clip8(ss);
      }
    } else if (lane < tw) {
      const size_t plane = (size_t)geo.H2 * geo.W2;
      float* dst = (float*)out + (size_t)n * 3 * plane + (size_t)(oy0 + oy) * geo.W2 + ox0 + lane;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        int ss = 1 << (RS_PRECISION_BITS - 1);
        for (int t = 0; t < cnt; ++t) ss += k[t] * (int)mid[t * RS_ROW_BYTES + lane * 3 + c];
        dst[c * plane] = cj_normalize(rs_clip8(ss), mu[c], sd[c]);
      }
    }
  }
}

// grid (ceil(W2 / RS_TILE_W), ceil(H2 / RS_TILE_H), N)
template <int OUT_KIND>
__global__ __launch_bounds__(RS_THREADS) void resize_kernel(const uint8_t* x, const int32_t* bounds_h,
                                                            const int32_t* coeff_h, const int32_t* bounds_v,
                                                            const int32_t* coeff_v, void* out, ResizeGeom geo,
                                                            float m0, float m1, float m2, float s0, float s1,
                                                            float s2) {
  const int n = blockIdx.z;
  resize_tile<OUT_KIND>(x + (size_t)n * geo.H * geo.W * 3, bounds_h, coeff_h, bounds_v, coeff_v, out, geo, n, m0, m1,
                        m2, s0, s1, s2);
}

// ---- a packed batch of mixed source sizes (oibl_resize_u8_mixed) ----------------------------------------------------
// Image n is [H_n][W_n][3] at byte offset pix_n of one packed buffer; H_n, W_n and pix_n are row n of the decoder's
// geometry table (jpeg_mixed.h).  Every image has tables of its own in the workspace, all with rows of the batch's
// largest ksize per axis (ResizeMixGeom::ksh / ksv, from the host's copy of the sizes):
//   bounds_h [N][W2][2], coeff_h [N][W2][ksh], bounds_v [N][H2][2], coeff_v [N][H2][ksv]
// What the kernels read from the table is forced into range first: 1 <= H_n <= max_h, 1 <= W_n <= max_w (the largest
// sides of the host's sizes, which sized the rows, the LDS and passed the scale limit — ksize and the rows of a tile
// grow with the source size, so what holds for the largest holds for every image), and pix_n + 3 H_n W_n <=
// packed_bytes.  An image that fails the check reads nothing: its tables are those of a 1 x 1 image and its output is
// zero bytes (out_kind 0) or the normalised value of zero bytes (out_kind 1).
struct ResizeMixGeom {
  int H2, W2, ksh, ksv, rows_cap, max_h, max_w;
  unsigned long long packed_bytes;
  size_t bounds_h, coeff_h, bounds_v, coeff_v;   // int32 offsets into the workspace
};

struct ResizeMixImage {
  int H, W, ok;
  unsigned long long pix;
};

__device__ static inline ResizeMixImage resize_mixed_image(const int32_t* row, const ResizeMixGeom& mg) {
  ResizeMixImage im;
  const int h = row[JPEG_MIX_H], w = row[JPEG_MIX_W], hi = row[JPEG_MIX_PIX_HI];
  im.H = min(max(h, 1), mg.max_h), im.W = min(max(w, 1), mg.max_w);
  im.pix = (unsigned long long)(uint32_t)row[JPEG_MIX_PIX_LO] | (unsigned long long)(uint32_t)(hi & 0xFF) << 32;
  im.ok = h == im.H && w == im.W && hi >= 0 && hi <= 0xFF &&
          im.pix + (unsigned long long)im.H * (unsigned long long)im.W * 3 <= mg.packed_bytes;
  if (!im.ok) im.H = im.W = 1, im.pix = 0;
  return im;
}

// grid (ceil(max(W2, H2) / RS_THREADS), 2, N): blockIdx.y 0 the horizontal axis, 1 the vertical one
__global__ __launch_bounds__(RS_THREADS) void resize_mixed_table_kernel(const int32_t* geom, ResizeMixGeom mg,
                                                                        int32_t* ws) {
  const int xx = blockIdx.x * RS_THREADS + threadIdx.x, n = blockIdx.z;
  const bool vertical = blockIdx.y != 0;
  const int out_size = vertical ? mg.H2 : mg.W2, ks = vertical ? mg.ksv : mg.ksh;
  if (xx >= out_size) return;
  const ResizeMixImage im = resize_mixed_image(geom + (size_t)n * JPEG_MIX_GEOM_INTS, mg);
  const int in_size = vertical ? im.H : im.W;
  const ResizeAxis a = rs_axis(in_size, out_size);   // a.ksize <= ks: in_size <= the largest, which gave ks
  int32_t* bounds = ws + (vertical ? mg.bounds_v : mg.bounds_h) + ((size_t)n * out_size + xx) * 2;
  int32_t* coeff = ws + (vertical ? mg.coeff_v : mg.coeff_h) + ((size_t)n * out_size + xx) * ks;
  if (a.ksize > ks) {   // (unreachable; keeps the row inside its slot whatever the arithmetic says)
    bounds[0] = 0, bounds[1] = 0;
    return;
  }
  rs_table_row(a, in_size, xx, bounds, coeff);
  for (int t = a.ksize; t < ks; ++t) coeff[t] = 0;
}

// grid (ceil(W2 / RS_TILE_W), ceil(H2 / RS_TILE_H), N)
template <int OUT_KIND>
__global__ __launch_bounds__(RS_THREADS) void resize_mixed_kernel(const uint8_t* packed, const int32_t* geom,
                                                                  const int32_t* ws, void* out, ResizeMixGeom mg,
                                                                  float m0, float m1, float m2, float s0, float s1,
                                                                  float s2) {
  const int n = blockIdx.z;
  const ResizeMixImage im = resize_mixed_image(geom + (size_t)n * JPEG_MIX_GEOM_INTS, mg);
  if (!im.ok) {   // the whole workgroup: the tile as zero bytes
    const int ox0 = blockIdx.x * RS_TILE_W, oy0 = blockIdx.y * RS_TILE_H;
    const int tw = min(RS_TILE_W, mg.W2 - ox0), th = min(RS_TILE_H, mg.H2 - oy0);
    const float z[3] = {cj_normalize(0, m0, s0), cj_normalize(0, m1, s1), cj_normalize(0, m2, s2)};
    for (int i = threadIdx.x; i < th * tw * 3; i += RS_THREADS) {
      const int oy = i / (tw * 3), j = i - oy * tw * 3, col = j / 3, c = j - col * 3;
      if (OUT_KIND == OIBL_JITTER_U8_NHWC)
        ((uint8_t*)out)[(((size_t)n * mg.H2 + oy0 + oy) * mg.W2 + ox0) * 3 + j] = 0;
      else
        ((float*)out)[(((size_t)n * 3 + c) * mg.H2 + oy0 + oy) * mg.W2 + ox0 + col] = z[c];
    }
    return;
  }
  const ResizeGeom geo = {im.H, im.W, mg.H2, mg.W2, mg.ksh, mg.ksv, min(mg.rows_cap, im.H)};
  resize_tile<OUT_KIND>(packed + im.pix, ws + mg.bounds_h + (size_t)n * mg.W2 * 2,
                        ws + mg.coeff_h + (size_t)n * mg.W2 * mg.ksh, ws + mg.bounds_v + (size_t)n * mg.H2 * 2,
                        ws + mg.coeff_v + (size_t)n * mg.H2 * mg.ksv, out, geo, n, m0, m1, m2, s0, s1, s2);
}

// the host's view of a mixed batch: the largest sides and what follows from them; false: a size or the scale limit
static bool resize_mixed_geom(const int32_t* sizes, int N, int H2, int W2, ResizeMixGeom& mg, size_t& ws_bytes,
                              int& bad) {
  int max_h = 0, max_w = 0;
  for (int n = 0; n < N; ++n) {
    const int H = sizes[2 * n], W = sizes[2 * n + 1];
    bad = n;
    if (H < 1 || W < 1 || H > RS_MAX_DIM || W > RS_MAX_DIM) return false;
    if ((long)H > (long)RS_MAX_SCALE * H2 || (long)W > (long)RS_MAX_SCALE * W2) return false;
    max_h = H > max_h ? H : max_h, max_w = W > max_w ? W : max_w;
  }
  bad = -1;
  mg.H2 = H2, mg.W2 = W2, mg.max_h = max_h, mg.max_w = max_w;
  mg.ksh = rs_axis(max_w, W2).ksize, mg.ksv = rs_axis(max_h, H2).ksize;
  const int rows = rs_tile_rows(rs_axis(max_h, H2));
  mg.rows_cap = rows < max_h ? rows : max_h;
  size_t at = 0;   // in int32s; every table starts on a multiple of 64 of them
  mg.bounds_h = at, at += align_up((size_t)N * W2 * 2, 64);
  mg.coeff_h = at, at += align_up((size_t)N * W2 * mg.ksh, 64);
  mg.bounds_v = at, at += align_up((size_t)N * H2 * 2, 64);
  mg.coeff_v = at, at += align_up((size_t)N * H2 * mg.ksv, 64);
  ws_bytes = at * sizeof(int32_t);
  mg.packed_bytes = 0;   // (the call's)
  return true;
}

struct ResizeLayout {
  size_t bounds_h, coeff_h, bounds_v, coeff_v, total;   // byte offsets into the workspace
  int ksh, ksv;
};

static ResizeLayout resize_layout(int H, int W, int H2, int W2) {
  ResizeLayout l;
  l.ksh = rs_axis(W, W2).ksize;
  l.ksv = rs_axis(H, H2).ksize;
  size_t at = 0;
  l.bounds_h = at, at += align_up((size_t)W2 * 2 * sizeof(int32_t), 256);
  l.coeff_h = at, at += align_up((size_t)W2 * l.ksh * sizeof(int32_t), 256);
  l.bounds_v = at, at += align_up((size_t)H2 * 2 * sizeof(int32_t), 256);
  l.coeff_v = at, at += align_up((size_t)H2 * l.ksv * sizeof(int32_t), 256);
  l.total = at;
  return l;
}

static bool resize_shape_ok(int N, int H, int W, int H2, int W2) {
  return N > 0 && N <= 65535 && H > 0 && W > 0 && H2 > 0 && W2 > 0 && H <= RS_MAX_DIM && W <= RS_MAX_DIM &&
         H2 <= RS_MAX_DIM && W2 <= RS_MAX_DIM;
}

static bool resize_scale_ok(int in_size, int out_size) { return (long)in_size <= (long)RS_MAX_SCALE * out_size; }

}  // namespace oibl

using namespace oibl;

extern "C" {

size_t oibl_resize_u8_workspace_bytes(int N, int H, int W, int H2, int W2) {
  if (!resize_shape_ok(N, H, W, H2, W2) || !resize_scale_ok(H, H2) || !resize_scale_ok(W, W2)) return 0;
  return resize_layout(H, W, H2, W2).total;
}

int oibl_resize_u8_tables(int in_size, int out_size, int32_t* bounds, int32_t* coeff, int ksize_capacity,
                          int* ksize_out_host_or_null, void* stream) {
  OIBL_REQUIRE(bounds && coeff, "resize_u8_tables: null pointer");
  OIBL_REQUIRE(in_size > 0 && out_size > 0 && in_size <= RS_MAX_DIM && out_size <= RS_MAX_DIM,
               "resize_u8_tables: sizes must be in [1, %d], got %d -> %d", RS_MAX_DIM, in_size, out_size);
  OIBL_REQUIRE((uintptr_t)bounds % 4 == 0 && (uintptr_t)coeff % 4 == 0,
               "resize_u8_tables: the tables must be 4-byte aligned");
  const int ksize = rs_axis(in_size, out_size).ksize;
  if (ksize_out_host_or_null) *ksize_out_host_or_null = ksize;
  OIBL_REQUIRE(ksize <= ksize_capacity, "resize_u8_tables: %d -> %d needs %d coefficients per row, capacity %d",
               in_size, out_size, ksize, ksize_capacity);
  hipLaunchKernelGGL(resize_table_kernel, dim3((unsigned)((out_size + RS_THREADS - 1) / RS_THREADS)),
                     dim3(RS_THREADS), 0, (hipStream_t)stream, in_size, out_size, bounds, coeff);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

int oibl_resize_u8(const uint8_t* x_nhwc, int N, int H, int W, int H2, int W2, int out_kind,
                   const float* mean3_host, const float* std3_host, void* out, void* ws, size_t ws_bytes,
                   void* stream) {
  OIBL_REQUIRE(x_nhwc && out, "resize_u8: null pointer");
  OIBL_REQUIRE(resize_shape_ok(N, H, W, H2, W2),
               "resize_u8: bad shape N=%d H=%d W=%d -> H2=%d W2=%d (N <= 65535, every size in [1, %d])", N, H, W,
               H2, W2, RS_MAX_DIM);
  OIBL_REQUIRE(resize_scale_ok(H, H2) && resize_scale_ok(W, W2),
               "resize_u8: %d x %d -> %d x %d shrinks an axis by more than the limit of %d (the source rows of "
               "a tile must fit in LDS)", H, W, H2, W2, RS_MAX_SCALE);
  OIBL_REQUIRE(out_kind == OIBL_JITTER_U8_NHWC || out_kind == OIBL_JITTER_F32_NCHW,
               "resize_u8: unknown out_kind %d", out_kind);
  OIBL_REQUIRE(out_kind == OIBL_JITTER_U8_NHWC || (mean3_host && std3_host),
               "resize_u8: the fp32 output needs mean3_host and std3_host");
  OIBL_REQUIRE(out_kind == OIBL_JITTER_U8_NHWC || (uintptr_t)out % 4 == 0,
               "resize_u8: the fp32 output must be 4-byte aligned");
  OIBL_REQUIRE(ws && (uintptr_t)ws % 256 == 0, "resize_u8: workspace must be 256-byte aligned");
  const ResizeLayout l = resize_layout(H, W, H2, W2);
  if (ws_bytes < l.total) {
    set_error("resize_u8: workspace %zu < required %zu bytes", ws_bytes, l.total);
    return OIBL_E_WORKSPACE;
  }
  int32_t* bounds_h = (int32_t*)((char*)ws + l.bounds_h);
  int32_t* coeff_h = (int32_t*)((char*)ws + l.coeff_h);
  int32_t* bounds_v = (int32_t*)((char*)ws + l.bounds_v);
  int32_t* coeff_v = (int32_t*)((char*)ws + l.coeff_v);
  int rc = oibl_resize_u8_tables(W, W2, bounds_h, coeff_h, RS_MAX_KSIZE, nullptr, stream);
  if (rc != OIBL_OK) return rc;
  rc = oibl_resize_u8_tables(H, H2, bounds_v, coeff_v, RS_MAX_KSIZE, nullptr, stream);
  if (rc != OIBL_OK) return rc;

  const int rows_cap = rs_tile_rows(rs_axis(H, H2));
  const ResizeGeom geo = {H, W, H2, W2, l.ksh, l.ksv, rows_cap < H ? rows_cap : H};
  const size_t lds = resize_lds_bytes(geo);
  OIBL_REQUIRE(lds <= 65536, "resize_u8: %zu bytes of LDS per workgroup", lds);   // implied by the scale limit
  const dim3 grid((unsigned)((W2 + RS_TILE_W - 1) / RS_TILE_W), (unsigned)((H2 + RS_TILE_H - 1) / RS_TILE_H),
                  (unsigned)N), block(RS_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (out_kind == OIBL_JITTER_U8_NHWC) {
    hipLaunchKernelGGL(resize_kernel<OIBL_JITTER_U8_NHWC>, grid, block, lds, st, x_nhwc, (const int32_t*)bounds_h,
                       (const int32_t*)coeff_h, (const int32_t*)bounds_v, (const int32_t*)coeff_v, out, geo, 0.0f,
                       0.0f, 0.0f, 1.0f, 1.0f, 1.0f);
  } else {
    hipLaunchKernelGGL(resize_kernel<OIBL_JITTER_F32_NCHW>, grid, block, lds, st, x_nhwc, (const int32_t*)bounds_h,
                       (const int32_t*)coeff_h, (const int32_t*)bounds_v, (const int32_t*)coeff_v, out, geo,
                       mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0], std3_host[1], std3_host[2]);
  }
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

size_t oibl_resize_u8_mixed_workspace_bytes(const int32_t* sizes_host, int N, int H2, int W2) {
  ResizeMixGeom mg;
  size_t need = 0;
  int bad = -1;
  if (!sizes_host || N <= 0 || N > 65535 || H2 <= 0 || W2 <= 0 || H2 > RS_MAX_DIM || W2 > RS_MAX_DIM) return 0;
  return resize_mixed_geom(sizes_host, N, H2, W2, mg, need, bad) ? need : 0;
}

int oibl_resize_u8_mixed(const uint8_t* packed, size_t packed_bytes, const int32_t* geom_dev,
                         const int32_t* sizes_host, int N, int H2, int W2, int out_kind, const float* mean3_host,
                         const float* std3_host, void* out, void* ws, size_t ws_bytes, void* stream) {
  OIBL_REQUIRE(packed && geom_dev && sizes_host && out, "resize_u8_mixed: null pointer");
  OIBL_REQUIRE(N > 0 && N <= 65535 && H2 > 0 && W2 > 0 && H2 <= RS_MAX_DIM && W2 <= RS_MAX_DIM,
               "resize_u8_mixed: bad shape N=%d -> H2=%d W2=%d (N <= 65535, every size in [1, %d])", N, H2, W2,
               RS_MAX_DIM);
  OIBL_REQUIRE(packed_bytes >= 1 && packed_bytes < JPEG_MIX_MAX_PIXEL_BYTES,
               "resize_u8_mixed: packed_bytes %zu must be in [1, 2^40)", packed_bytes);
  ResizeMixGeom mg;
  size_t need = 0;
  int bad = -1;
  const bool fits = resize_mixed_geom(sizes_host, N, H2, W2, mg, need, bad);
  OIBL_REQUIRE(fits || (sizes_host[2 * bad] >= 1 && sizes_host[2 * bad + 1] >= 1 &&
                        sizes_host[2 * bad] <= RS_MAX_DIM && sizes_host[2 * bad + 1] <= RS_MAX_DIM),
               "resize_u8_mixed: bad shape: image %d is %d x %d, every size must be in [1, %d]", bad,
               sizes_host[2 * bad], sizes_host[2 * bad + 1], RS_MAX_DIM);
  OIBL_REQUIRE(fits, "resize_u8_mixed: image %d: %d x %d -> %d x %d shrinks an axis by more than the limit of %d (the "
               "source rows of a tile must fit in LDS)", bad, sizes_host[2 * bad], sizes_host[2 * bad + 1], H2, W2,
               RS_MAX_SCALE);
  OIBL_REQUIRE(out_kind == OIBL_JITTER_U8_NHWC || out_kind == OIBL_JITTER_F32_NCHW,
               "resize_u8_mixed: unknown out_kind %d", out_kind);
  OIBL_REQUIRE(out_kind == OIBL_JITTER_U8_NHWC || (mean3_host && std3_host),
               "resize_u8_mixed: the fp32 output needs mean3_host and std3_host");
  OIBL_REQUIRE(out_kind == OIBL_JITTER_U8_NHWC || (uintptr_t)out % 4 == 0,
               "resize_u8_mixed: the fp32 output must be 4-byte aligned");
  OIBL_REQUIRE((uintptr_t)geom_dev % 4 == 0, "resize_u8_mixed: geom_dev must be 4-byte aligned");
  OIBL_REQUIRE(ws && (uintptr_t)ws % 256 == 0, "resize_u8_mixed: workspace must be 256-byte aligned");
  if (ws_bytes < need) {
    set_error("resize_u8_mixed: workspace %zu < required %zu bytes", ws_bytes, need);
    return OIBL_E_WORKSPACE;
  }
  mg.packed_bytes = packed_bytes;
  const ResizeGeom largest = {mg.max_h, mg.max_w, H2, W2, mg.ksh, mg.ksv, mg.rows_cap};
  const size_t lds = resize_lds_bytes(largest);
  OIBL_REQUIRE(lds <= 65536, "resize_u8_mixed: %zu bytes of LDS per workgroup", lds);   // implied by the scale limit
  hipStream_t st = (hipStream_t)stream;
  int32_t* tables = (int32_t*)ws;
  const int longest = H2 > W2 ? H2 : W2;
  hipLaunchKernelGGL(resize_mixed_table_kernel,
                     dim3((unsigned)((longest + RS_THREADS - 1) / RS_THREADS), 2u, (unsigned)N), dim3(RS_THREADS), 0,
                     st, geom_dev, mg, tables);
  OIBL_LAUNCH_CHECK();
  const dim3 grid((unsigned)((W2 + RS_TILE_W - 1) / RS_TILE_W), (unsigned)((H2 + RS_TILE_H - 1) / RS_TILE_H),
                  (unsigned)N), block(RS_THREADS);
  if (out_kind == OIBL_JITTER_U8_NHWC) {
    hipLaunchKernelGGL(resize_mixed_kernel<OIBL_JITTER_U8_NHWC>, grid, block, lds, st, packed, geom_dev,
                       (const int32_t*)tables, out, mg, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f);
  } else {
    hipLaunchKernelGGL(resize_mixed_kernel<OIBL_JITTER_F32_NCHW>, grid, block, lds, st, packed, geom_dev,
                       (const int32_t*)tables, out, mg, mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0],
                       std3_host[1], std3_host[2]);
  }
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

}  // extern "C"
