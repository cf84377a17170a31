// The per-pixel steps of the training-image augmentation (include/list_augment.h), written once for augment_kernels.hip,
// for the host-only list_augment_pixel and for tests/csrc/augment_host.cpp.  Plain C++ (IEEE float32 / float64 arithmetic,
// fmod, floor and rint only); build with -ffp-contract=off: the formulas assume that no product is fused into a sum.
//
// Every step maps uint8 RGB to uint8 RGB the way Pillow 12 does between two enhancers:
//   brightness  ImageEnhance.Brightness: Image.blend(black, image, f), float32
//   saturation  ImageEnhance.Color: Image.blend(image.convert("L"), image, f), float32
//   hue         image.convert("HSV"), H + shift mod 256, convert("RGB"); the conversions are Pillow's, rounding for
//               rounding (where a value is rounded to float32 on the way, Pillow keeps it in a float variable)
// Levels are carried as int (0 ... 255).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AUGMENT_HD __host__ __device__ __forceinline__
#else
#define AUGMENT_HD inline
#endif

// ops mask and the values of an order slot (include/list_augment.h)
enum { AUGMENT_FLIP = 1, AUGMENT_BRIGHTNESS = 2, AUGMENT_SATURATION = 4, AUGMENT_HUE = 8 };
enum { AUGMENT_SLOT_BRIGHTNESS = 0, AUGMENT_SLOT_CONTRAST = 1, AUGMENT_SLOT_SATURATION = 2, AUGMENT_SLOT_HUE = 3 };

// a blend's float32 value to a level: 0 below, 255 above, truncated between
AUGMENT_HD int augment_clip_trunc(float t) { return t <= 0.0f ? 0 : t >= 255.0f ? 255 : (int)t; }

AUGMENT_HD int augment_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

AUGMENT_HD void augment_brightness(int& r, int& g, int& b, float f) {
  r = augment_clip_trunc(f * (float)r);
  g = augment_clip_trunc(f * (float)g);
  b = augment_clip_trunc(f * (float)b);
}

// ITU-R 601-2 luma as convert("L") rounds it
AUGMENT_HD int augment_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

AUGMENT_HD void augment_saturation(int& r, int& g, int& b, float f) {
  const int L = augment_luma(r, g, b);
  const float Lf = (float)L;
  r = augment_clip_trunc(Lf + f * (float)(r - L));
  g = augment_clip_trunc(Lf + f * (float)(g - L));
  b = augment_clip_trunc(Lf + f * (float)(b - L));
}

// RGB -> (H, S, V) levels.  s, rc, gc, bc are float32; h is evaluated in float64 from them and rounded to float32, and so
// is the wrapped h / 6 + 1: the two roundings are Pillow's (dropping either changes tens of thousands of colours).
AUGMENT_HD void augment_rgb_to_hsv(int r, int g, int b, int& H, int& S, int& V) {
  const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
  V = maxc;
  if (maxc == minc) {
    H = 0, S = 0;
    return;
  }
  const float cr = (float)(maxc - minc);
  const float s = cr / (float)maxc;
  const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
  float h;
  if (r == maxc) h = (float)((double)bc - (double)gc);
  else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
  else h = (float)(4.0 + (double)gc - (double)rc);
  h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
  H = augment_clip8((int)((double)h * 255.0));
  S = augment_clip8((int)((double)s * 255.0));
}

// (H, S, V) levels -> RGB, float64 throughout, rint to nearest even
AUGMENT_HD void augment_hsv_to_rgb(int H, int S, int V, int& r, int& g, int& b) {
  if (S == 0) {
    r = g = b = V;
    return;
  }
  const double fh = (double)H * 6.0 / 255.0, fs = (double)S / 255.0, v = (double)V;
  const double fl = floor(fh), f = fh - fl;
  const int i = (int)fl;                         // 0 ... 6; 6 only at H = 255, where f = 0
  const int p = augment_clip8((int)rint(v * (1.0 - fs)));
  const int q = augment_clip8((int)rint(v * (1.0 - fs * f)));
  const int t = augment_clip8((int)rint(v * (1.0 - fs * (1.0 - f))));
  switch (i % 6) {
    case 0: r = V, g = t, b = p; break;
    case 1: r = q, g = V, b = p; break;
    case 2: r = p, g = V, b = t; break;
    case 3: r = p, g = q, b = V; break;
    case 4: r = t, g = p, b = V; break;
    default: r = V, g = p, b = q; break;
  }
}

// shift in 0 ... 255.  Shift 0 still makes the round trip through HSV, which is lossy, as Pillow's is.
AUGMENT_HD void augment_hue(int& r, int& g, int& b, int shift) {
  int H, S, V;
  augment_rgb_to_hsv(r, g, b, H, S, V);
  augment_hsv_to_rgb((H + shift) & 255, S, V, r, g, b);
}

// The colour steps of one image on one pixel: the four slots in turn, each when its bit of `ops` is set.
AUGMENT_HD void augment_colour(int& r, int& g, int& b, int ops, const int32_t order[4], float brightness, float saturation,
                               int hue_shift) {
  for (int k = 0; k < 4; ++k) {
    const int slot = order[k];
    if (slot == AUGMENT_SLOT_BRIGHTNESS && (ops & AUGMENT_BRIGHTNESS)) augment_brightness(r, g, b, brightness);
    else if (slot == AUGMENT_SLOT_SATURATION && (ops & AUGMENT_SATURATION)) augment_saturation(r, g, b, saturation);
    else if (slot == AUGMENT_SLOT_HUE && (ops & AUGMENT_HUE)) augment_hue(r, g, b, hue_shift);
  }
}

// ToTensor: the level over 255 in float32, correctly rounded
AUGMENT_HD float augment_to_float(int level) { return (float)level / 255.0f; }
