// Training colour jitter on raw uint8 batches (torchvision's ColorJitter on PIL images: get_transformer_train,
// ibl/utils/data/__init__.py:29-35 of the reference), optionally fused with ToTensor + Normalize.
//
// The arithmetic is PIL's, rounding by rounding (augment_pixel.h): the uint8 result equals PIL's bit for bit.
//   luma        L = (19595 R + 38470 G + 7471 B + 32768) >> 16
//   blend       t = f32(d) + a * (f32(x) - f32(d)) in fp32, truncated; clipped to [0, 255] only when a is outside
//               [0, 1].  Brightness: d = 0; saturation: d = L; contrast: d = int(mean(L) + 0.5) of the image AS IT
//               STANDS when contrast's turn comes
//   hue         RGB -> HSV bytes, h += shift mod 256, HSV -> RGB (the round trip runs for shift 0 too: it is lossy)
//
// An elementwise, memory-bound pass with ONE image-wide dependency, the contrast mean:
//   jitter_partial_kernel   applies the ops ordered before contrast and writes one integer partial sum of L per
//                           workgroup (images without a contrast op return at once);
//   jitter_apply_kernel     adds the partial sums of its image (integers: any order gives the same bits), recomputes
//                           the prefix and applies all four ops, then writes uint8 NHWC or normalised fp32 NCHW.
// No atomics, no floating-point reduction: identical bits from run to run, and nothing of one image reaches another.
//
// One lane handles four consecutive pixels per step: 12 input bytes (three dwords where the image base is 4-byte
// aligned; an image of H W 3 bytes that is no multiple of 4 starts misaligned and is read and written by bytes),
// and one 16-byte store per NCHW plane (where H W is a multiple of 4 and the output is 16-byte aligned), so that a
// wave reads 768 contiguous bytes and writes 1 KiB rows.  A workgroup covers `chunk` pixels, a multiple of 4096,
// chosen so that an image has at most 1024 partial sums (augment_geom.h, which a host program compiles too).  fp64
// appears only where PIL promotes to double.
//
// A packed batch of MIXED sizes (oibl_color_jitter_u8_mixed, between oibl_jpeg_decode_mixed and oibl_resize_u8_mixed)
// runs the same two passes with every image's H, W and offset from the decoder's geometry table: see the kernels.
#include "common.h"

// PIL rounds after every operation: no fused multiply-add anywhere in this unit
#pragma clang fp contract(off)

#include "augment_geom.h"
#include "augment_pixel.h"

namespace oibl {

struct u32x3 {
  uint32_t a, b, c;
};

// the 12 bytes of pixels [px, px + 4) of an image; bytes behind the image read as zero
__device__ __forceinline__ void load_group(const uint8_t* img, long px, long HW, bool dwords, int (&c)[12]) {
  if (jitter_group_wide(dwords, px, HW)) {
    const u32x3 w = *reinterpret_cast<const u32x3*>(img + 3 * px);
    const uint32_t v[3] = {w.a, w.b, w.c};
#pragma unroll
    for (int k = 0; k < 12; ++k) c[k] = (int)((v[k >> 2] >> (8 * (k & 3))) & 255u);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const long at = 3 * px + k;
      c[k] = at < 3 * HW ? (int)img[at] : 0;
    }
  }
}

__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* s_red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  unsigned long long t = 0;
#pragma unroll
  for (int w = 0; w < CJ_WAVES; ++w) t += s_red[w];
  __syncthreads();   // s_red may be written again
  return t;
}

// The two passes over ONE image `img` of geo.HW pixels, as workgroup `part` of its geo.nparts: the uniform kernels
// and the kernels of a packed batch of mixed sizes run this text, so an image has the same bits in both.

// the workgroup's partial sum of L behind the ops ordered before contrast (ops.contrast_at < 4)
__device__ __forceinline__ unsigned long long jitter_partial_part(const uint8_t* img, const JitterOps& ops,
                                                                  const JitterGeom& geo, int part,
                                                                  unsigned long long* s_red) {
  const bool dwords = (uintptr_t)img % 4 == 0;
  const long begin = (long)part * geo.chunk;
  unsigned long long sum = 0;
  for (int s = 0; s < geo.chunk; s += CJ_STEP) {
    const long px = begin + s + (long)threadIdx.x * CJ_GROUP;
    if (px >= geo.HW) break;
    int c[12];
    load_group(img, px, geo.HW, dwords, c);
#pragma unroll
    for (int j = 0; j < CJ_GROUP; ++j) {
      if (px + j < geo.HW) {
        int r = c[3 * j], g = c[3 * j + 1], b = c[3 * j + 2];
        cj_apply(ops, 0, ops.contrast_at, 0, r, g, b);
        sum += (unsigned)cj_luma(r, g, b);
      }
    }
  }
  return block_sum(sum, s_red);
}

// the contrast op's degenerate value from the image's partial sums (integers: any order gives the same bits)
__device__ __forceinline__ int jitter_mean(const JitterOps& ops, const unsigned long long* parts,
                                           const JitterGeom& geo, unsigned long long* s_red) {
  if (ops.contrast_at == 4) return 0;
  unsigned long long sum = 0;
  for (int i = threadIdx.x; i < geo.nparts; i += CJ_THREADS) sum += parts[i];
  return cj_contrast_mean(block_sum(sum, s_red), geo.HW);
}

// all four ops on the workgroup's pixels; out8 [HW][3] or outf [3][HW] is the IMAGE's output (out8 may be img)
template <int OUT_KIND>
__device__ __forceinline__ void jitter_apply_part(const uint8_t* img, const JitterOps& ops, int mean, uint8_t* out8,
                                                  float* outf, const JitterGeom& geo, int part, float m0, float m1,
                                                  float m2, float s0, float s1, float s2) {
  const bool dwords = (uintptr_t)img % 4 == 0;
  const bool out_wide = OUT_KIND == OIBL_JITTER_U8_NHWC ? (uintptr_t)out8 % 4 == 0
                                                        : ((uintptr_t)outf % 16 == 0 && geo.HW % 4 == 0);
  const float mu[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
  const long begin = (long)part * geo.chunk;
  for (int s = 0; s < geo.chunk; s += CJ_STEP) {
    const long px = begin + s + (long)threadIdx.x * CJ_GROUP;
    if (px >= geo.HW) break;
    int c[12];
    load_group(img, px, geo.HW, dwords, c);
#pragma unroll
    for (int j = 0; j < CJ_GROUP; ++j) cj_apply(ops, 0, 4, mean, c[3 * j], c[3 * j + 1], c[3 * j + 2]);
    const bool full = px + CJ_GROUP <= geo.HW;
    if (OUT_KIND == OIBL_JITTER_U8_NHWC) {
      if (jitter_group_wide(out_wide, px, geo.HW)) {
        uint32_t v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
          v[k] = (uint32_t)c[4 * k] | ((uint32_t)c[4 * k + 1] << 8) | ((uint32_t)c[4 * k + 2] << 16) |
                 ((uint32_t)c[4 * k + 3] << 24);
        *reinterpret_cast<u32x3*>(out8 + 3 * px) = u32x3{v[0], v[1], v[2]};
      } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
          if (3 * px + k < 3 * geo.HW) out8[3 * px + k] = (uint8_t)c[k];
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        float v[CJ_GROUP];
#pragma unroll
        for (int j = 0; j < CJ_GROUP; ++j) v[j] = cj_normalize(c[3 * j + ch], mu[ch], sd[ch]);
        float* plane = outf + (size_t)ch * geo.HW + px;
        if (out_wide && full) {
          *reinterpret_cast<f32x4_t*>(plane) = f32x4_t{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
          for (int j = 0; j < CJ_GROUP; ++j)
            if (px + j < geo.HW) plane[j] = v[j];
        }
      }
    }
  }
}

// grid (nparts, N)
__global__ __launch_bounds__(CJ_THREADS) void jitter_partial_kernel(const uint8_t* x, const JitterRecord* records,
                                                                    unsigned long long* parts, JitterGeom geo) {
  __shared__ unsigned long long s_red[CJ_WAVES];
  const int n = blockIdx.y, part = blockIdx.x;
  const JitterOps ops = cj_decode(records + n);
  if (ops.contrast_at == 4) return;                 // uniform: the whole workgroup leaves
  const unsigned long long sum = jitter_partial_part(x + (size_t)n * geo.HW * 3, ops, geo, part, s_red);
  if (threadIdx.x == 0) parts[(size_t)n * geo.nparts + part] = sum;
}

// grid (nparts, N); records == nullptr: no jitter
template <int OUT_KIND>
__global__ __launch_bounds__(CJ_THREADS) void jitter_apply_kernel(const uint8_t* x, const JitterRecord* records,
                                                                  const unsigned long long* parts, void* out,
                                                                  JitterGeom geo, float m0, float m1, float m2,
                                                                  float s0, float s1, float s2) {
  __shared__ unsigned long long s_red[CJ_WAVES];
  const int n = blockIdx.y, part = blockIdx.x;
  const JitterOps ops = cj_decode(records ? records + n : nullptr);
  const int mean = jitter_mean(ops, parts + (size_t)n * geo.nparts, geo, s_red);
  jitter_apply_part<OUT_KIND>(x + (size_t)n * geo.HW * 3, ops, mean, (uint8_t*)out + (size_t)n * geo.HW * 3,
                              (float*)out + (size_t)n * geo.HW * 3, geo, part, m0, m1, m2, s0, s1, s2);
}

// ---- a packed batch of mixed sizes (oibl_color_jitter_u8_mixed) -----------------------------------------------------
// Image n is [H_n][W_n][3] at byte offset pix_n of the packed buffer the mixed decoder writes and the mixed resize
// reads; H_n, W_n and pix_n are row n of the decoder's geometry table (jitter_mixed_image of augment_geom.h forces
// them into range and checks them against the call's packed_bytes).  The chunk and the part count are those of the
// image's OWN H_n W_n, so its partial sums — and its bits — are those of the uniform call on that image alone; its
// sums have row n of the workspace, [N][max_parts].  An image whose row fails the check is skipped by both launches.
// In place (out == packed): a lane writes exactly the bytes it read, and the group that holds the image's end goes
// by bytes, so nothing behind 3 H_n W_n — the padding up to the next multiple of 64, the next image — is touched.

// grid (max_parts, N)
__global__ __launch_bounds__(CJ_THREADS) void jitter_mixed_partial_kernel(const uint8_t* packed, const int32_t* geom,
                                                                          const JitterRecord* records,
                                                                          unsigned long long* parts, JitterMixCall mc) {
  __shared__ unsigned long long s_red[CJ_WAVES];
  const int n = blockIdx.y, part = blockIdx.x;
  const JitterMixImage im = jitter_mixed_image(geom + (size_t)n * JPEG_MIX_GEOM_INTS, mc);
  if (!im.ok || part >= im.geo.nparts) return;      // uniform: the whole workgroup leaves
  const JitterOps ops = cj_decode(records + n);
  if (ops.contrast_at == 4) return;
  const unsigned long long sum = jitter_partial_part(packed + im.pix, ops, im.geo, part, s_red);
  if (threadIdx.x == 0) parts[(size_t)n * mc.max_parts + part] = sum;
}

// grid (max_parts, N); records == nullptr: a copy
__global__ __launch_bounds__(CJ_THREADS) void jitter_mixed_apply_kernel(const uint8_t* packed, const int32_t* geom,
                                                                        const JitterRecord* records,
                                                                        const unsigned long long* parts,
                                                                        uint8_t* out_packed, JitterMixCall mc) {
  __shared__ unsigned long long s_red[CJ_WAVES];
  const int n = blockIdx.y, part = blockIdx.x;
  const JitterMixImage im = jitter_mixed_image(geom + (size_t)n * JPEG_MIX_GEOM_INTS, mc);
  if (!im.ok || part >= im.geo.nparts) return;
  const JitterOps ops = cj_decode(records ? records + n : nullptr);
  const int mean = jitter_mean(ops, parts + (size_t)n * mc.max_parts, im.geo, s_red);
  jitter_apply_part<OIBL_JITTER_U8_NHWC>(packed + im.pix, ops, mean, out_packed + im.pix, nullptr, im.geo, part, 0.0f,
                                         0.0f, 0.0f, 1.0f, 1.0f, 1.0f);
}

}  // namespace oibl

using namespace oibl;

extern "C" {

size_t oibl_color_jitter_u8_workspace_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0 || (long)H * W > CJ_MAX_HW) return 0;
  return align_up((size_t)N * jitter_geom(H, W).nparts * sizeof(unsigned long long), 256);
}

int oibl_color_jitter_u8(const uint8_t* x_nhwc, int N, int H, int W, const void* records, int out_kind,
                         const float* mean3_host, const float* std3_host, void* out, void* ws, size_t ws_bytes,
                         void* stream) {
  OIBL_REQUIRE(x_nhwc && out, "color_jitter_u8: null pointer");
  OIBL_REQUIRE(N > 0 && H > 0 && W > 0 && (long)H * W <= CJ_MAX_HW && N <= 65535,
               "color_jitter_u8: bad shape N=%d H=%d W=%d", N, H, W);
  OIBL_REQUIRE(out_kind == OIBL_JITTER_U8_NHWC || out_kind == OIBL_JITTER_F32_NCHW,
               "color_jitter_u8: unknown out_kind %d", out_kind);
  OIBL_REQUIRE(out_kind == OIBL_JITTER_U8_NHWC || (mean3_host && std3_host),
               "color_jitter_u8: the fp32 output needs mean3_host and std3_host");
  OIBL_REQUIRE(out_kind == OIBL_JITTER_U8_NHWC || (uintptr_t)out % 4 == 0,
               "color_jitter_u8: the fp32 output must be 4-byte aligned");
  OIBL_REQUIRE(!records || (uintptr_t)records % 4 == 0, "color_jitter_u8: records must be 4-byte aligned");
  const JitterGeom geo = jitter_geom(H, W);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)geo.nparts, (unsigned)N), block(CJ_THREADS);
  unsigned long long* parts = (unsigned long long*)ws;
  if (records) {
    OIBL_REQUIRE(ws && (uintptr_t)ws % 256 == 0, "color_jitter_u8: workspace must be 256-byte aligned");
    const size_t need = oibl_color_jitter_u8_workspace_bytes(N, H, W);
    if (ws_bytes < need) {
      set_error("color_jitter_u8: workspace %zu < required %zu bytes", ws_bytes, need);
      return OIBL_E_WORKSPACE;
    }
    hipLaunchKernelGGL(jitter_partial_kernel, grid, block, 0, st, x_nhwc, (const JitterRecord*)records, parts, geo);
    OIBL_LAUNCH_CHECK();
  }
  if (out_kind == OIBL_JITTER_U8_NHWC) {
    hipLaunchKernelGGL(jitter_apply_kernel<OIBL_JITTER_U8_NHWC>, grid, block, 0, st, x_nhwc,
                       (const JitterRecord*)records, (const unsigned long long*)parts, out, geo, 0.0f, 0.0f, 0.0f,
                       1.0f, 1.0f, 1.0f);
  } else {
    hipLaunchKernelGGL(jitter_apply_kernel<OIBL_JITTER_F32_NCHW>, grid, block, 0, st, x_nhwc,
                       (const JitterRecord*)records, (const unsigned long long*)parts, out, geo, mean3_host[0],
                       mean3_host[1], mean3_host[2], std3_host[0], std3_host[1], std3_host[2]);
  }
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

size_t oibl_color_jitter_u8_mixed_workspace_bytes(const int32_t* sizes_host, int N) {
  int max_parts = 0, bad = -1;
  if (!sizes_host || N <= 0 || N > 65535 || jitter_mixed_host(sizes_host, N, &max_parts, &bad)) return 0;
  return align_up((size_t)N * max_parts * sizeof(unsigned long long), 256);
}

int oibl_color_jitter_u8_mixed(const uint8_t* packed, size_t packed_bytes, const int32_t* geom_dev,
                               const int32_t* sizes_host, int N, const void* records, uint8_t* out_packed, void* ws,
                               size_t ws_bytes, void* stream) {
  OIBL_REQUIRE(packed && geom_dev && sizes_host && out_packed, "color_jitter_u8_mixed: null pointer");
  OIBL_REQUIRE(N > 0 && N <= 65535, "color_jitter_u8_mixed: bad shape: N = %d must be in [1, 65535]", N);
  OIBL_REQUIRE(packed_bytes >= 1 && packed_bytes < JPEG_MIX_MAX_PIXEL_BYTES,
               "color_jitter_u8_mixed: packed_bytes %zu must be in [1, 2^40)", packed_bytes);
  JitterMixCall mc = {packed_bytes, 0};
  int bad = -1;
  const int why = jitter_mixed_host(sizes_host, N, &mc.max_parts, &bad);
  OIBL_REQUIRE(why != CJ_MIX_E_SIZE, "color_jitter_u8_mixed: bad shape: image %d is %d x %d, every side must be in "
               "[1, %d]", bad, sizes_host[2 * bad], sizes_host[2 * bad + 1], JPEG_MIX_MAX_DIM);
  OIBL_REQUIRE(why != CJ_MIX_E_PIXELS, "color_jitter_u8_mixed: bad shape: image %d is %d x %d, more than 2^28 pixels",
               bad, sizes_host[2 * bad], sizes_host[2 * bad + 1]);
  OIBL_REQUIRE((uintptr_t)geom_dev % 4 == 0, "color_jitter_u8_mixed: geom_dev must be 4-byte aligned");
  OIBL_REQUIRE(!records || (uintptr_t)records % 4 == 0, "color_jitter_u8_mixed: records must be 4-byte aligned");
  if (!records && out_packed == packed) return OIBL_OK;   // no jitter, in place: nothing to do
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)mc.max_parts, (unsigned)N), block(CJ_THREADS);
  unsigned long long* parts = (unsigned long long*)ws;
  if (records) {
    const size_t need = align_up((size_t)N * mc.max_parts * sizeof(unsigned long long), 256);
    if (!ws || (uintptr_t)ws % 256 != 0) {
      set_error("color_jitter_u8_mixed: workspace must be 256-byte aligned (%zu bytes)", need);
      return OIBL_E_WORKSPACE;
    }
    if (ws_bytes < need) {
      set_error("color_jitter_u8_mixed: workspace %zu < required %zu bytes", ws_bytes, need);
      return OIBL_E_WORKSPACE;
    }
    hipLaunchKernelGGL(jitter_mixed_partial_kernel, grid, block, 0, st, packed, geom_dev,
                       (const JitterRecord*)records, parts, mc);
    OIBL_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(jitter_mixed_apply_kernel, grid, block, 0, st, packed, geom_dev, (const JitterRecord*)records,
                     (const unsigned long long*)parts, out_packed, mc);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

}  // extern "C"
