// Per-pixel arithmetic of the colour jitter (augment.hip): PIL's, rounding by rounding.
//
// PIL computes the blends of ImageEnhance in C `float` and its HSV conversions in a mixture of `float` and values
// promoted to double; the functions below repeat every operation in the type PIL's code has it in, each rounded on
// its own.  The includer switches floating-point contraction OFF for the whole unit: one fused multiply-add where
// PIL rounds twice moves a truncated byte.  Host and device compile the same text (the host side serves a
// stand-alone check against the fixture).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define OIBL_PX __host__ __device__ __forceinline__
#else
#define OIBL_PX static inline
#endif

namespace oibl {

enum { CJ_BRIGHTNESS = 0, CJ_CONTRAST = 1, CJ_SATURATION = 2, CJ_HUE = 3 };

// one record per image (include/openibl_amd.h: oibl_color_jitter_u8)
struct JitterRecord {
  int32_t op[4];
  float factor[3];
  uint32_t hue;
};
static_assert(sizeof(JitterRecord) == 32, "a jitter record is 32 bytes");

// PIL's RGB -> L
OIBL_PX int cj_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

OIBL_PX int cj_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ToTensor + Normalize of one byte, both divisions IEEE: the fp32 output of augment.hip and of resize.hip
OIBL_PX float cj_normalize(int c, float mean, float std) { return ((float)c / 255.0f - mean) / std; }

// Image.blend(degenerate d, image x, a) of one byte; `inside` = 0 <= a <= 1, where PIL does not clip
OIBL_PX int cj_blend(int d, int x, float a, bool inside) {
  const float df = (float)d;
  const float t = df + a * ((float)x - df);
  if (!inside) {
    if (t <= 0.0f) return 0;
    if (t >= 255.0f) return 255;
  }
  return (int)t;
}

// R(x) of the HSV -> RGB direction: the double product is stored to float, then rounded half up
OIBL_PX int cj_round8(double x) { return cj_clip8((int)__builtin_floorf((float)x + 0.5f)); }

// RGB -> HSV (bytes), h += shift mod 256, HSV -> RGB
OIBL_PX void cj_hue(int& r, int& g, int& b, int shift) {
  const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
  const int v = maxc;
  int H = 0, S = 0;
  if (maxc != minc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h0;
    if (r == maxc)
      h0 = bc - gc;
    else if (g == maxc)
      h0 = (float)(2.0 + (double)rc - (double)bc);
    else
      h0 = (float)(4.0 + (double)gc - (double)rc);
    // fmod(h0 / 6 + 1, 1): the argument is in [5/6, 11/6], so the remainder is x - trunc(x), exact
    const double hx = (double)h0 / 6.0 + 1.0;
    const float h1 = (float)(hx - __builtin_trunc(hx));
    H = cj_clip8((int)((double)h1 * 255.0));
    S = cj_clip8((int)((double)s * 255.0));
  }
  H = (H + shift) & 255;
  if (S == 0) {
    r = g = b = v;
    return;
  }
  const float fh = (float)((double)H * 6.0 / 255.0);
  const float fi = __builtin_floorf(fh);
  const float f = fh - fi;
  const float fs = (float)((double)S / 255.0);
  const double F = (double)f, Sd = (double)fs, vf = (double)v;
  const int p = cj_round8(vf * (1.0 - Sd));
  const int q = cj_round8(vf * (1.0 - Sd * F));
  const int t = cj_round8(vf * (1.0 - Sd * (1.0 - F)));
  switch ((int)fi % 6) {
    case 0: r = v, g = t, b = p; break;
    case 1: r = q, g = v, b = p; break;
    case 2: r = p, g = v, b = t; break;
    case 3: r = p, g = q, b = v; break;
    case 4: r = t, g = p, b = v; break;
    default: r = v, g = p, b = q; break;
  }
}

// the factors of a record, read once per workgroup
struct JitterOps {
  int op[4];
  float a[3];
  bool inside[3];
  int shift;
  int contrast_at;   // the place of the (first) contrast op, 4 = none
};

OIBL_PX JitterOps cj_decode(const JitterRecord* rec) {
  JitterOps o;
  o.contrast_at = 4;
  for (int k = 0; k < 4; ++k) {
    int c = rec ? rec->op[k] : -1;
    if (c < 0 || c > 3 || (c == CJ_CONTRAST && o.contrast_at < 4)) c = -1;
    if (c == CJ_CONTRAST) o.contrast_at = k;
    o.op[k] = c;
  }
  for (int k = 0; k < 3; ++k) {
    o.a[k] = rec ? rec->factor[k] : 1.0f;
    o.inside[k] = o.a[k] >= 0.0f && o.a[k] <= 1.0f;
  }
  o.shift = rec ? (int)(rec->hue & 255u) : 0;
  return o;
}

// ops [first, last) of the record on one pixel; `mean` is the contrast op's degenerate value
OIBL_PX void cj_apply(const JitterOps& o, int first, int last, int mean, int& r, int& g, int& b) {
#if defined(__HIPCC__)
#pragma unroll   // four static places: the record stays in registers
#endif
  for (int k = 0; k < 4; ++k) {
    if (k < first || k >= last) continue;
    switch (o.op[k]) {
      case CJ_BRIGHTNESS:
        r = cj_blend(0, r, o.a[0], o.inside[0]);
        g = cj_blend(0, g, o.a[0], o.inside[0]);
        b = cj_blend(0, b, o.a[0], o.inside[0]);
        break;
      case CJ_CONTRAST:
        r = cj_blend(mean, r, o.a[1], o.inside[1]);
        g = cj_blend(mean, g, o.a[1], o.inside[1]);
        b = cj_blend(mean, b, o.a[1], o.inside[1]);
        break;
      case CJ_SATURATION: {
        const int L = cj_luma(r, g, b);
        r = cj_blend(L, r, o.a[2], o.inside[2]);
        g = cj_blend(L, g, o.a[2], o.inside[2]);
        b = cj_blend(L, b, o.a[2], o.inside[2]);
        break;
      }
      case CJ_HUE:
        cj_hue(r, g, b, o.shift);
        break;
      default:
        break;
    }
  }
}

// int(sum / count + 0.5), the division in double (ImageStat.mean, ImageEnhance.Contrast)
OIBL_PX int cj_contrast_mean(unsigned long long sum, long count) {
  return (int)((double)sum / (double)count + 0.5);
}

}  // namespace oibl
