// Pillow's C arithmetic for the RandAugment ops, one value at a time (used by csrc/randaug.hip).
// Every function is the expression of the named Pillow source with its rounding: C `float` and
// `double` operations one by one, never contracted into a fused multiply-add.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RA_HD __device__ __forceinline__
#else
#define RA_HD inline
#endif
// Contraction is switched off inside every function that computes in floating point (the build's
// default would fuse a multiply and the add after it, which moves a result by one); a compiler
// without the pragma needs -ffp-contract=off.
#define RA_NO_CONTRACT _Pragma("clang fp contract(off)")

namespace dcp {
namespace ra {

enum Op {
  IDENTITY = 0, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS,
  POSTERIZE, SOLARIZE, AUTOCONTRAST, EQUALIZE, NUM_OPS
};

// Filter.c clip8: also the clip of Blend.c's extrapolation branch
RA_HD int clip8(float v) { return v <= 0.0f ? 0 : (v >= 255.0f ? 255 : (int)v); }

// Convert.c rgb2l: L24(rgb) >> 16
RA_HD int lum(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Blend.c ImagingBlend(deg, img, alpha): (UINT8)(deg + alpha * (img - deg)) in C float.  For alpha in
// [0, 1] the value lies between the two bytes, so the clip of the other branch changes nothing there.
RA_HD int blend(int deg, int img, float alpha) {
  RA_NO_CONTRACT
  const float scaled = alpha * (float)(img - deg);
  return clip8((float)deg + scaled);
}

// Filter.c ImagingFilter3x3 with ImageFilter.SMOOTH ((1,1,1),(1,5,1),(1,1,1)) / 13 on the interior
// pixel whose 3 x 3 neighbourhood of one channel is up[], mid[], dn[] (rows y-1, y, y+1): the
// kernel's first row meets row y+1, and the 0.5 of the rounding is the sum's first term.
RA_HD int smooth(const int up[3], const int mid[3], const int dn[3]) {
  RA_NO_CONTRACT
  const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
  float ss = 0.5f;
  ss += ((float)dn[0] * k1 + (float)dn[1] * k1) + (float)dn[2] * k1;
  ss += ((float)mid[0] * k1 + (float)mid[1] * k5) + (float)mid[2] * k1;
  ss += ((float)up[0] * k1 + (float)up[1] * k1) + (float)up[2] * k1;
  return clip8(ss);
}

// The byte -> byte ops that need no image statistics beyond `mean` (ImageEnhance.Contrast's
// int(mean(L) + 0.5)): entry v of their lookup table.  p is the plan's parameter word.
RA_HD int lut_param(int op, int p, int mean, int v) {
  union { int i; float f; } u;
  u.i = p;
  switch (op) {
    case BRIGHTNESS: return blend(0, v, u.f);
    case CONTRAST: return blend(mean, v, u.f);
    case POSTERIZE: return v & ~((1 << (8 - p)) - 1);  // ImageOps.posterize
    case SOLARIZE: return v < p ? v : 255 - v;         // ImageOps.solarize
    default: return v;
  }
}

// ImageOps.autocontrast (cutoff 0) of a channel whose lowest / highest occupied bins are lo / hi:
// Python doubles, int() truncating toward zero, then the clamp.
RA_HD int autocontrast_lut(int lo, int hi, int v) {
  RA_NO_CONTRACT
  if (hi <= lo) return v;
  const double scale = 255.0 / (double)(hi - lo);
  const double offset = -(double)lo * scale;
  const int ix = (int)((double)v * scale + offset);
  return ix < 0 ? 0 : (ix > 255 ? 255 : ix);
}

// ImageOps.equalize: step = (total - last occupied bin) // 255; entry v = (step // 2 + sum of the
// bins below v) // step, stored through Image.point's clip to a byte.  The identity when at most
// one bin is occupied or step is 0.
RA_HD int equalize_step(int occupied, int total, int last_count) {
  return occupied <= 1 ? 0 : (total - last_count) / 255;
}
RA_HD int equalize_lut(int step, int below, int v) {
  if (step == 0) return v;
  const int q = (step / 2 + below) / step;
  return q > 255 ? 255 : q;
}

// Geometry.c affine_fixed: the source pixel index of output (x, y), or -1 for the fill
RA_HD int affine_src(const int a[6], int x, int y, int H, int W) {
  const int xin = (a[2] + a[1] * y + a[0] * x) >> 16;
  const int yin = (a[5] + a[4] * y + a[3] * x) >> 16;
  return (xin >= 0 && xin < W && yin >= 0 && yin < H) ? yin * W + xin : -1;
}

}  // namespace ra
}  // namespace dcp
