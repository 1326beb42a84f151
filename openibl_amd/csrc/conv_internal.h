// What crosses the boundaries between conv.hip (3x3 convolutions), stem.hip (conv1_1, the Cin = 64 kernel, the
// fused stems) and vgg.hip (the VGG16 forward): declarations only.  Internal.
#pragma once

#include "common.h"

namespace oibl {

// Test hooks read in more than one of the three units, on the pattern of g_regstage (common.h): defined once
// (conv.hip) in the debug library, compile-time constants in the product.  A hook read in one unit is an
// OIBL_HOOK there.
#ifdef OIBL_DEBUG_HOOKS
extern unsigned long long* g_prof_buf;
extern int g_conv_tile, g_conv_ablate;
#else
constexpr unsigned long long* g_prof_buf = nullptr;
constexpr int g_conv_tile = 0, g_conv_ablate = 0;
#endif

static inline bool precision_ok(int precision) {
  return precision == OIBL_BF16 || precision == OIBL_F32 || precision == OIBL_BF16X3 || precision == OIBL_F16MX;
}
// the fused stems address their input through one 32-bit buffer descriptor
static inline bool stem_eligible(int N, int H, int W) {
  return H >= 2 && W >= 2 && (size_t)N * 3 * H * W * 4 < (size_t)0xE0000000u;
}

// ---- conv.hip ----
int conv3x3_impl(const void* in, int N, int H, int W, int cin, const void* packed_w, const float* bias, int cout,
                 int relu, int pool, int precision, void* out, hipStream_t st, int out_f32 = 0,
                 void* splitk_ws = nullptr, unsigned* range_flag = nullptr, float bias_mul = 1.f, float out_mul = 1.f);
size_t conv_layer_scratch_bytes(int N, int h, int w, int cin, int cout, int pool, int precision);
int launch_mx_join_rows(const void* src, float* dst, size_t n, int which, float mul, unsigned max_blocks,
                        hipStream_t st);
int launch_clear_word(unsigned* w, hipStream_t st);
int launch_u8_nhwc_to_nchw_f32(const uint8_t* x, float* out, long npix_total, long plane, const float* mean3,
                               const float* std3, hipStream_t st);

// ---- stem.hip ----
int launch_conv_c64(const void* in, int N, int H, int W, const void* w, const float* bias, int cout, int relu,
                    int pool, void* out, hipStream_t st);
// mean3 / std3 (host pointers, both or neither): x is the raw uint8 NHWC image and the kernel normalises
int launch_vgg_stem(const void* x, int N, int H, int W, const float* mean3, const float* std3, const float* w1,
                    const float* b1, const void* packed_w2, const float* b2, void* out, hipStream_t st);
int launch_vgg_stem_x3(const void* x, int N, int H, int W, const float* w1, const float* b1, const void* packed_w2,
                       const float* b2, void* out, hipStream_t st, bool mx = false, unsigned* range_flag = nullptr,
                       const float* u8_mean3 = nullptr, const float* u8_std3 = nullptr, float act_scale = 1.f);

}  // namespace oibl
