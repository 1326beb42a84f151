// The front of the VGG16 backbone on gfx950 (ibl/models/vgg.py:40-42, modules 0-4), launch side: conv1_1 alone
// (conv1_1.h), the Cin = 64 "resident weights + LDS halo" kernel (conv_c64.h), and the fused stems — conv1_1 + ReLU +
// conv1_2 + ReLU + 2x2 max-pool in one launch — in bf16 (stem_bf16.h), bf16x3 (stem_x3.h) and f16mx (stem_mx12.h;
// stem_mx16.h for uint8 input).  Every kernel has a header of its own, included below inside namespace oibl; what the
// persistent stems share is stem_parts.h.  This file keeps the parameters, the hooks, the launchers and the C entry
// points.  The convolutions behind the stem are conv.hip, the forward pass that calls both vgg.hip.
#include "conv_internal.h"
#include "gemm_core.h"
#include "ring_core.h"

namespace oibl {

OIBL_HOOK(int, g_conv11_valu, 0);  // test hook: force the vector-ALU conv1_1 in bf16 mode too
OIBL_HOOK(int, g_stem3_prio, 0);  // bf16x3 stem, test hook: producer issue priority | consumer priority << 2
OIBL_HOOK(int, g_stem_mx12, 1);  // test hook: 0 = the float32-input f16mx stem on vgg_stem_mx_kernel<false> (A/B, bit comparisons)
OIBL_HOOK(unsigned*, g_stem_mx_flag, nullptr);  // test hook: the range flag oibl_vgg16_stem_mx hands its kernel (the entry has none)
#ifdef OIBL_DEBUG_HOOKS
static int g_stem_mx_route = 0;  // the kernel the last float32-input f16mx stem launched: 12 or 16 (waves); 0 = none yet
#endif

struct StemParams {
  const void* x;     // U8 = false: [N][3][H][W] fp32 (normalised); U8 = true: [N][H][W][3] uint8
  float mean[3], stdv[3];  // U8 only: the loader's Normalize constants
  const float* w1;   // conv1_1 [64][3][3][3] fp32
  const float* b1;
  const char* w2;    // conv1_2 packed [9][64][64] bf16
  const float* b2;
  char* out;
  unsigned x_bytes;
  int N, H, W;
  int tiles_x, tiles_y, ntiles;
  unsigned long long* prof;  // optional (test hook): shader-clock totals of block 0, waves 0 and 4
  int prod_prio;             // bf16x3 stem: issue priority of the producer role outside its MFMAs
  unsigned* range_flag;      // f16mx stem: raised when a conv1_1 / conv1_2 output hits the fp16 bound; may be null
  float act_scale = 1.f;     // f16mx stem: conv1_1's weights and both biases are multiplied by this (g_mx_act_shift)
};

#include "conv_c64.h"
#include "stem_parts.h"
#include "conv1_1.h"
#include "stem_bf16.h"
#include "stem_x3.h"
#include "stem_mx16.h"
#include "stem_mx12.h"

int launch_conv_c64(const void* in, int N, int H, int W, const void* w, const float* bias, int cout, int relu,
                    int pool, void* out, hipStream_t st) {
  C64Params p;
  p.in = (const char*)in;
  p.w = (const char*)w;
  p.bias = bias;
  p.out = (char*)out;
  p.zero = (const char*)zero_line_device_ptr();
  OIBL_REQUIRE(p.zero != nullptr, "conv3x3: zero line symbol not found");
  p.N = N;
  p.H = H;
  p.W = W;
  p.cout = cout;
  p.relu = relu;
  p.prof = g_prof_buf;
  p.tiles_x = (W + 31) / 32;
  p.tiles_y = (H + 7) / 8;
  const long nt = (long)N * p.tiles_x * p.tiles_y;
  OIBL_REQUIRE(nt < 0x7fffffffL, "conv3x3: too many tiles");
  p.ntiles = (int)nt;
  const int slices = cout / 64;
  int gx = 256 / slices;  // one resident workgroup per CU
  if (gx < 1) gx = 1;
  if (gx > p.ntiles) gx = p.ntiles;
  auto kern = pool ? conv3x3_c64_kernel<true> : conv3x3_c64_kernel<false>;
  if (pool)
    OIBL_SET_MAX_LDS(conv3x3_c64_kernel<true>, C64_LDS_BYTES);
  else
    OIBL_SET_MAX_LDS(conv3x3_c64_kernel<false>, C64_LDS_BYTES);
  hipLaunchKernelGGL(kern, dim3(gx, slices), dim3(256), C64_LDS_BYTES, st, p);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

// mean3 / std3: host pointers, used only when U8
template <bool U8>
static int launch_vgg_stem_impl(const void* x, int N, int H, int W, const float* mean3, const float* std3,
                                const float* w1, const float* b1, const void* packed_w2, const float* b2,
                                void* out, hipStream_t st) {
  StemParams p;
  p.x = x;
  for (int c = 0; c < 3; ++c) {
    p.mean[c] = U8 ? mean3[c] : 0.f;
    p.stdv[c] = U8 ? std3[c] : 1.f;
  }
  p.w1 = w1;
  p.b1 = b1;
  p.w2 = (const char*)packed_w2;
  p.b2 = b2;
  p.out = (char*)out;
  p.x_bytes = (unsigned)((size_t)N * 3 * H * W * (U8 ? 1 : 4));
  p.N = N;
  p.H = H;
  p.W = W;
  p.tiles_x = (W + 31) / 32;
  p.tiles_y = (H + 7) / 8;
  const long nt = (long)N * p.tiles_x * p.tiles_y;
  OIBL_REQUIRE(nt < 0x7fffffffL, "vgg stem: too many tiles");
  p.ntiles = (int)nt;
  p.prof = g_prof_buf;
  int gx = 256;  // one persistent workgroup per CU
  if (gx > p.ntiles) gx = p.ntiles;
  constexpr int lds = U8 ? ST_LDS_BYTES_U8 : ST_LDS_BYTES;
  auto kern = vgg_stem_kernel<U8>;
  OIBL_SET_MAX_LDS(kern, lds);
  hipLaunchKernelGGL(kern, dim3(gx), dim3(512), lds, st, p);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}
int launch_vgg_stem(const void* x, int N, int H, int W, const float* mean3, const float* std3, const float* w1,
                    const float* b1, const void* packed_w2, const float* b2, void* out, hipStream_t st) {
  return mean3 != nullptr && std3 != nullptr
             ? launch_vgg_stem_impl<true>(x, N, H, W, mean3, std3, w1, b1, packed_w2, b2, out, st)
             : launch_vgg_stem_impl<false>(x, N, H, W, nullptr, nullptr, w1, b1, packed_w2, b2, out, st);
}

// u8_mean3 / u8_std3 (host pointers, both or neither): x is the raw uint8 NHWC image and the kernel normalises
// (stem_parts.h, "uint8 input")
int launch_vgg_stem_x3(const void* x, int N, int H, int W, const float* w1, const float* b1, const void* packed_w2,
                       const float* b2, void* out, hipStream_t st, bool mx, unsigned* range_flag,
                       const float* u8_mean3, const float* u8_std3, float act_scale) {
  StemParams p = {};
  p.range_flag = range_flag;
  p.act_scale = act_scale;
  const bool u8 = u8_mean3 != nullptr && u8_std3 != nullptr;
  if (u8) {
    for (int c = 0; c < 3; ++c) {   // v = u * a + b (see the kernel): a in `mean`, b in `stdv`
      p.mean[c] = (float)(1.0 / (255.0 * (double)u8_std3[c]));
      p.stdv[c] = (float)(-(double)u8_mean3[c] / (double)u8_std3[c]);
    }
  }
  p.x = x;
  p.w1 = w1;
  p.b1 = b1;
  p.w2 = (const char*)packed_w2;
  p.b2 = b2;
  p.out = (char*)out;
  // (uint8: the descriptor covers the tensor rounded up to whole dwords — the 12-byte window loads are dword
  //  aligned, and the range check drops a dword that is only partly inside; the up to 3 extra bytes share the
  //  last valid byte's dword, hence its page, and are never used: the taps they belong to are masked)
  p.x_bytes = u8 ? (unsigned)align_up((size_t)N * 3 * H * W, 4) : (unsigned)((size_t)N * 3 * H * W * 4);
  p.N = N;
  p.H = H;
  p.W = W;
  p.tiles_x = (W + 31) / 32;
  p.tiles_y = (H + 7) / 8;
  const long nt = (long)N * p.tiles_x * p.tiles_y;
  OIBL_REQUIRE(nt < 0x7fffffffL, "vgg stem: too many tiles");
  p.ntiles = (int)nt;
  p.prof = g_prof_buf;
  // f16mx: producers at priority 2, consumers at 3 unless the hook says otherwise (tests/gpu_stem_mx_bench.py:
  // 1.72 ms against 1.80 ms with equal priorities; the bf16x3 roles are at their best with equal ones)
  p.prod_prio = (mx && g_stem3_prio == 0) ? 14 : g_stem3_prio;
  // one persistent workgroup per CU.  bf16x3: two workgroups (output-channel halves) per tile range; f16mx: one, both
  // output-channel halves inside it
  const dim3 grid3((unsigned)(128 < p.ntiles ? 128 : p.ntiles), 2), gridmx((unsigned)(256 < p.ntiles ? 256 : p.ntiles), 1);
  if (mx && u8) {
    auto kern = vgg_stem_mx_kernel<true>;
    OIBL_SET_MAX_LDS(kern, S3_LDS_BYTES);
    hipLaunchKernelGGL(kern, gridmx, dim3(1024), S3_LDS_BYTES, st, p);
  } else if (mx && g_stem_mx12) {
    OIBL_SET_MAX_LDS(stem_mx12_kernel, S3_LDS_BYTES);
    hipLaunchKernelGGL(stem_mx12_kernel, gridmx, dim3(64 * (4 + M12_PROD)), S3_LDS_BYTES, st, p);
#ifdef OIBL_DEBUG_HOOKS
    g_stem_mx_route = 12;
#endif
  } else if (mx) {
    auto kern = vgg_stem_mx_kernel<false>;
    OIBL_SET_MAX_LDS(kern, S3_LDS_BYTES);
    hipLaunchKernelGGL(kern, gridmx, dim3(1024), S3_LDS_BYTES, st, p);
#ifdef OIBL_DEBUG_HOOKS
    g_stem_mx_route = 16;
#endif
  } else if (u8) {
    auto kern = vgg_stem_x3_kernel<true>;
    OIBL_SET_MAX_LDS(kern, S3_LDS_BYTES);
    hipLaunchKernelGGL(kern, grid3, dim3(1024), S3_LDS_BYTES, st, p);
  } else {
    auto kern = vgg_stem_x3_kernel<false>;
    OIBL_SET_MAX_LDS(kern, S3_LDS_BYTES);
    hipLaunchKernelGGL(kern, grid3, dim3(1024), S3_LDS_BYTES, st, p);
  }
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

}  // namespace oibl

using namespace oibl;

extern "C" {

int oibl_vgg16_stem_bf16(const float* x_nchw, int N, int H, int W, const float* w1_oihw,
                         const float* b1, const void* packed_w2, const float* b2, void* out,
                         void* stream) {
  OIBL_REQUIRE(x_nchw && w1_oihw && b1 && packed_w2 && b2 && out, "vgg16_stem: null pointer");
  OIBL_REQUIRE(N > 0 && H >= 2 && W >= 2, "vgg16_stem: bad shape N=%d H=%d W=%d", N, H, W);
  OIBL_REQUIRE(stem_eligible(N, H, W), "vgg16_stem: input of %d x 3 x %d x %d exceeds 3.5 GB", N, H, W);
  OIBL_REQUIRE((uintptr_t)packed_w2 % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)x_nchw % 4 == 0,
               "vgg16_stem: packed weights / output must be 16-byte aligned");
  return launch_vgg_stem(x_nchw, N, H, W, nullptr, nullptr, w1_oihw, b1, packed_w2, b2, out, (hipStream_t)stream);
}

int oibl_vgg16_stem_x3(const float* x_nchw, int N, int H, int W, const float* w1_oihw, const float* b1,
                       const void* packed_w2, const float* b2, void* out, void* stream) {
  OIBL_REQUIRE(x_nchw && w1_oihw && b1 && packed_w2 && b2 && out, "vgg16_stem_x3: null pointer");
  OIBL_REQUIRE(N > 0 && H >= 2 && W >= 2, "vgg16_stem_x3: bad shape N=%d H=%d W=%d", N, H, W);
  OIBL_REQUIRE(stem_eligible(N, H, W), "vgg16_stem_x3: input of %d x 3 x %d x %d exceeds 3.5 GB", N, H, W);
  OIBL_REQUIRE((uintptr_t)packed_w2 % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)x_nchw % 4 == 0,
               "vgg16_stem_x3: packed weights / output must be 16-byte aligned");
  return launch_vgg_stem_x3(x_nchw, N, H, W, w1_oihw, b1, packed_w2, b2, out, (hipStream_t)stream);
}

int oibl_vgg16_stem_mx(const float* x_nchw, int N, int H, int W, const float* w1_oihw, const float* b1,
                       const void* packed_w2, const float* b2, void* out, void* stream) {
  OIBL_REQUIRE(x_nchw && w1_oihw && b1 && packed_w2 && b2 && out, "vgg16_stem_mx: null pointer");
  OIBL_REQUIRE(N > 0 && H >= 2 && W >= 3, "vgg16_stem_mx: bad shape N=%d H=%d W=%d (needs H >= 2, W >= 3)", N, H, W);
  OIBL_REQUIRE(stem_eligible(N, H, W), "vgg16_stem_mx: input of %d x 3 x %d x %d exceeds 3.5 GB", N, H, W);
  OIBL_REQUIRE((uintptr_t)packed_w2 % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)x_nchw % 4 == 0,
               "vgg16_stem_mx: packed weights / output must be 16-byte aligned");
  return launch_vgg_stem_x3(x_nchw, N, H, W, w1_oihw, b1, packed_w2, b2, out, (hipStream_t)stream, true, g_stem_mx_flag);
}

#ifdef OIBL_DEBUG_HOOKS
int oibl_debug_set_stem3_prio(int prio) {
  g_stem3_prio = prio < 0 ? 0 : (prio & 15);
  return OIBL_OK;
}

int oibl_debug_set_stem_mx12(int on) {
  g_stem_mx12 = on ? 1 : 0;
  return OIBL_OK;
}

int oibl_debug_last_stem_mx_route(void) { return g_stem_mx_route; }

int oibl_debug_set_stem_mx_flag(void* dev_u32) {
  g_stem_mx_flag = (unsigned*)dev_u32;
  return OIBL_OK;
}

int oibl_debug_set_conv11_valu(int on) {
  g_conv11_valu = on ? 1 : 0;
  return OIBL_OK;
}

// One uint8 stem alone (tests/test_gpu_stem_u8.py): x [N][H][W][3] uint8 -> out [N][H/2][W/2][64] in the precision's
// container, through the launch vgg_forward_impl makes for raw bytes — vgg_stem_kernel<true> (bf16),
// vgg_stem_x3_kernel<true> (bf16x3), vgg_stem_mx_kernel<true> (f16mx; act_scale and the range flag are
// its alone).  mean3 / std3 are host pointers.  The 4-byte stems fetch aligned dwords: x must start on one, the
// condition under which vgg_forward_impl takes this route.
int oibl_debug_vgg16_stem_u8(const void* x_u8_nhwc, int N, int H, int W, const float* mean3_host, const float* std3_host,
                             const float* w1_oihw, const float* b1, const void* packed_w2, const float* b2,
                             int precision, float act_scale, void* range_flag_dev_u32, void* out, void* stream) {
  OIBL_REQUIRE(x_u8_nhwc && mean3_host && std3_host && w1_oihw && b1 && packed_w2 && b2 && out,
               "debug_vgg16_stem_u8: null pointer");
  OIBL_REQUIRE(precision == OIBL_BF16 || precision == OIBL_BF16X3 || precision == OIBL_F16MX,
               "debug_vgg16_stem_u8: bad precision %d (bf16, bf16x3 or f16mx)", precision);
  const bool mx = precision == OIBL_F16MX;
  OIBL_REQUIRE(N > 0 && H >= 2 && W >= (mx ? 3 : 2), "debug_vgg16_stem_u8: bad shape N=%d H=%d W=%d (needs H >= 2, W >= %d)",
               N, H, W, mx ? 3 : 2);
  OIBL_REQUIRE(stem_eligible(N, H, W), "debug_vgg16_stem_u8: input of %d x 3 x %d x %d exceeds 3.5 GB", N, H, W);
  OIBL_REQUIRE((uintptr_t)packed_w2 % 16 == 0 && (uintptr_t)out % 16 == 0,
               "debug_vgg16_stem_u8: packed weights / output must be 16-byte aligned");
  if (precision == OIBL_BF16)
    return launch_vgg_stem(x_u8_nhwc, N, H, W, mean3_host, std3_host, w1_oihw, b1, packed_w2, b2, out, (hipStream_t)stream);
  OIBL_REQUIRE((uintptr_t)x_u8_nhwc % 4 == 0,
               "debug_vgg16_stem_u8: the bf16x3 / f16mx stems need a 4-byte aligned image (vgg_forward_impl normalises "
               "a misaligned one in a pass of its own)");
  OIBL_REQUIRE(mx || act_scale == 1.f, "debug_vgg16_stem_u8: act_scale %g belongs to f16mx only", (double)act_scale);
  return launch_vgg_stem_x3(x_u8_nhwc, N, H, W, w1_oihw, b1, packed_w2, b2, out, (hipStream_t)stream, mx,
                            mx ? (unsigned*)range_flag_dev_u32 : nullptr, mean3_host, std3_host, mx ? act_scale : 1.f);
}
#endif

int oibl_conv1_1_nchw(const float* x_nchw, int N, int H, int W, const float* w_oihw,
                      const float* bias, int precision, void* out, void* stream) {
  OIBL_REQUIRE(x_nchw && w_oihw && bias && out, "conv1_1: null pointer");
  OIBL_REQUIRE(N > 0 && H > 0 && W > 0, "conv1_1: bad shape N=%d H=%d W=%d", N, H, W);
  OIBL_REQUIRE(precision_ok(precision), "conv1_1: bad precision %d", precision);
  const long nstrips = (long)N * H * ((W + 7) / 8);
  const long grid = (nstrips + 3) / 4;
  OIBL_REQUIRE(grid <= 0x7fffffffL, "conv1_1: grid too large");
  if (precision == OIBL_BF16X3 || (precision == OIBL_BF16 && !g_conv11_valu)) {
    const int tiles_per_row = (W + C11_TW - 1) / C11_TW;
    const long ntiles = (long)N * H * tiles_per_row;
    const unsigned blocks = (unsigned)(ntiles < 4096 ? ntiles : 4096);
    if (precision == OIBL_BF16X3)
      hipLaunchKernelGGL(conv1_1_mfma_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                         x_nchw, w_oihw, bias, (char*)out, N, H, W, tiles_per_row, ntiles);
    else
      hipLaunchKernelGGL(conv1_1_mfma_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                         x_nchw, w_oihw, bias, (char*)out, N, H, W, tiles_per_row, ntiles);
  } else if (precision == OIBL_BF16)
    hipLaunchKernelGGL(conv1_1_kernel<bf16_t>, dim3((unsigned)grid), dim3(256), 0,
                       (hipStream_t)stream, x_nchw, w_oihw, bias, (bf16_t*)out, N, H, W);
  else
    hipLaunchKernelGGL(conv1_1_kernel<float>, dim3((unsigned)grid), dim3(256), 0,
                       (hipStream_t)stream, x_nchw, w_oihw, bias, (float*)out, N, H, W);
  OIBL_LAUNCH_CHECK();
  return OIBL_OK;
}

}  // extern "C"
