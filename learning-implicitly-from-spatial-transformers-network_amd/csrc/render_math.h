// Every per-vertex, per-face and per-pixel rule of the z-buffer rasteriser (include/list_render.h), written once for
// render_kernels.hip and for tests/csrc/render_host.cpp; render.py restates the same rules in numpy.  Plain C++ (IEEE
// float32 / float64 arithmetic, fmaf, floor and sqrtf only); build with -ffp-contract=off: apart from the explicit fmaf
// chain of the projection no product is fused into a sum.
//
// The rules, in the order a face meets them:
//   vertex   p = 2 * (v[2], v[1], v[0]) (models.py:91-92); X, Y, Z by the fma chain of point_math.h: project(), in k order.
//            LIST camera: den = Z + 1e-8f, pixel x = (X / den) * (W-1)/(map_size-1), y likewise with H, both in float64
//            from the float32 X, Y, den and WITHOUT the reference's clamp; depth value 1 / den in float64 (larger is
//            nearer).  Orthographic camera: x = X, y = Y, depth value Z (smaller is nearer).
//   snap     sub-pixel coordinate = floor(x * 16 + 0.5) in float64: 1/16 pixel, round half up; pixel centres lie at the
//            multiples of 16.
//   drop     a face is dropped whole for the FIRST of: a vertex index outside [0, V); a non-finite X, Y or Z (den) of any
//            vertex; LIST camera and any den <= z_near; any |snapped coordinate| > 2^24; zero area after snapping.
//   cover    integer edge functions (int64) with the top-left fill rule, after the face has been given positive
//            orientation (both windings are drawn): a centre on an edge belongs to the face iff the edge is a top edge
//            (horizontal, interior below) or a left edge (interior to its right).
//   depth    ((e0 * d0 + e1 * d1) + e2 * d2) / area in float64 with the integer edge values as weights, rounded to float32.
//   winner   one 64-bit key per pixel: the depth's bits made monotone (and inverted for the LIST camera) above the face
//            index; the smallest key wins, so the nearest fragment and, among equal float32 depths, the lowest face.
//   shade    face normal (b - a) x (c - a) in float32 in mesh coordinates (array axis order); normal map or head-light grey.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RENDER_HD __host__ __device__ __forceinline__
#else
#define RENDER_HD inline
#endif

enum { RENDER_ORTHO = 0, RENDER_LIST = 1 };
// what became of a face: the index of its counter in the stats record (include/list_render.h)
enum {
  RENDER_BAD_INDEX = 0, RENDER_NON_FINITE = 1, RENDER_BEHIND_NEAR = 2, RENDER_GUARD_BAND = 3, RENDER_ZERO_AREA = 4,
  RENDER_OFFSCREEN = 5, RENDER_SMALL = 6, RENDER_LARGE = 7, RENDER_N_STATS = 8
};
enum { RENDER_SUBPIXEL = 16, RENDER_SUBPIXEL_BITS = 4, RENDER_CAP = 8 };

#define RENDER_GUARD 16777216.0                         /* 2^24 sub-pixels */
#define RENDER_BACKGROUND_KEY 0xFFFFFFFFFFFFFFFFull

RENDER_HD uint32_t render_bits(float x) { return __builtin_bit_cast(uint32_t, x); }
RENDER_HD float render_from_bits(uint32_t b) { return __builtin_bit_cast(float, b); }
RENDER_HD bool render_finite(float x) { return (render_bits(x) & 0x7f800000u) != 0x7f800000u; }

RENDER_HD float render_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}

RENDER_HD float render_sqrt(float a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fsqrt_rn(a);
#else
  return sqrtf(a);
#endif
}

// ---- vertex ---------------------------------------------------------------------------------------------------------
// X, Y, Z of mesh vertex v (array axis order) under the 4x3 matrix T (row-major, as trans_mat[b])
RENDER_HD void render_chain(const float* T, const float* v, float& X, float& Y, float& Z) {
  const float px = v[2] * 2.f, py = v[1] * 2.f, pz = v[0] * 2.f;
  X = px * T[0]; Y = px * T[1]; Z = px * T[2];
  X = fmaf(py, T[3], X); Y = fmaf(py, T[4], Y); Z = fmaf(py, T[5], Z);
  X = fmaf(pz, T[6], X); Y = fmaf(pz, T[7], Y); Z = fmaf(pz, T[8], Z);
  X = X + T[9]; Y = Y + T[10]; Z = Z + T[11];
}

struct RenderVert {
  int64_t sx, sy;      // snapped, in sub-pixels (0 when the vertex is flagged)
  double d;            // depth value: 1 / den (LIST) or Z (orthographic)
  int flags;           // bit RENDER_NON_FINITE / RENDER_BEHIND_NEAR / RENDER_GUARD_BAND
};

RENDER_HD RenderVert render_vertex(const float* T, int mode, int map_size, int W, int H, float z_near, const float* v) {
  float X, Y, Z;
  render_chain(T, v, X, Y, Z);
  RenderVert o;
  o.sx = 0; o.sy = 0; o.d = 0.0; o.flags = 0;
  double xs, ys;
  if (mode == RENDER_LIST) {
    const float den = Z + 1e-8f;
    if (!(render_finite(X) && render_finite(Y) && render_finite(den))) { o.flags = 1 << RENDER_NON_FINITE; return o; }
    if (den <= z_near) { o.flags = 1 << RENDER_BEHIND_NEAR; return o; }
    const double dd = (double)den;
    xs = ((double)X / dd) * ((double)(W - 1) / (double)(map_size - 1));
    ys = ((double)Y / dd) * ((double)(H - 1) / (double)(map_size - 1));
    o.d = 1.0 / dd;
  } else {
    if (!(render_finite(X) && render_finite(Y) && render_finite(Z))) { o.flags = 1 << RENDER_NON_FINITE; return o; }
    xs = (double)X;
    ys = (double)Y;
    o.d = (double)Z;
  }
  const double fx = floor(xs * 16.0 + 0.5), fy = floor(ys * 16.0 + 0.5);
  if (!(fabs(fx) <= RENDER_GUARD && fabs(fy) <= RENDER_GUARD)) { o.flags = 1 << RENDER_GUARD_BAND; return o; }
  o.sx = (int64_t)fx;
  o.sy = (int64_t)fy;
  return o;
}

// ---- face -----------------------------------------------------------------------------------------------------------
struct RenderFace {
  int64_t x0, y0, x1, y1, x2, y2;      // positive orientation: area > 0
  double d0, d1, d2;
  int64_t area;
  int ix0, ix1, iy0, iy1;              // the pixel centres inside the bounding box, clamped to the image (inclusive)
};

RENDER_HD int64_t render_min3(int64_t a, int64_t b, int64_t c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
RENDER_HD int64_t render_max3(int64_t a, int64_t b, int64_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// What becomes of the face with the projected vertices a, b, c (its indices were valid) -> its counter, and f when that
// is RENDER_SMALL or RENDER_LARGE.
RENDER_HD int render_face(const RenderVert& a, const RenderVert& b, const RenderVert& c, int W, int H, RenderFace& f) {
  const int flags = a.flags | b.flags | c.flags;
  if (flags & (1 << RENDER_NON_FINITE)) return RENDER_NON_FINITE;
  if (flags & (1 << RENDER_BEHIND_NEAR)) return RENDER_BEHIND_NEAR;
  if (flags & (1 << RENDER_GUARD_BAND)) return RENDER_GUARD_BAND;
  const int64_t area = (b.sx - a.sx) * (c.sy - a.sy) - (b.sy - a.sy) * (c.sx - a.sx);
  if (area == 0) return RENDER_ZERO_AREA;
  f.x0 = a.sx; f.y0 = a.sy; f.d0 = a.d;
  if (area > 0) {
    f.x1 = b.sx; f.y1 = b.sy; f.d1 = b.d; f.x2 = c.sx; f.y2 = c.sy; f.d2 = c.d; f.area = area;
  } else {
    f.x1 = c.sx; f.y1 = c.sy; f.d1 = c.d; f.x2 = b.sx; f.y2 = b.sy; f.d2 = b.d; f.area = -area;
  }
  const int64_t lo_x = render_min3(f.x0, f.x1, f.x2), hi_x = render_max3(f.x0, f.x1, f.x2);
  const int64_t lo_y = render_min3(f.y0, f.y1, f.y2), hi_y = render_max3(f.y0, f.y1, f.y2);
  // first centre at or after lo, last centre at or before hi (>> of a negative int64 is arithmetic: a floor)
  const int64_t cx0 = (lo_x + (RENDER_SUBPIXEL - 1)) >> RENDER_SUBPIXEL_BITS, cx1 = hi_x >> RENDER_SUBPIXEL_BITS;
  const int64_t cy0 = (lo_y + (RENDER_SUBPIXEL - 1)) >> RENDER_SUBPIXEL_BITS, cy1 = hi_y >> RENDER_SUBPIXEL_BITS;
  f.ix0 = (int)(cx0 < 0 ? 0 : cx0);
  f.ix1 = (int)(cx1 > W - 1 ? W - 1 : cx1);
  f.iy0 = (int)(cy0 < 0 ? 0 : cy0);
  f.iy1 = (int)(cy1 > H - 1 ? H - 1 : cy1);
  if (cx0 > W - 1 || cx1 < 0 || cy0 > H - 1 || cy1 < 0 || f.ix1 < f.ix0 || f.iy1 < f.iy0) return RENDER_OFFSCREEN;
  return (f.ix1 - f.ix0 + 1 <= RENDER_CAP && f.iy1 - f.iy0 + 1 <= RENDER_CAP) ? RENDER_SMALL : RENDER_LARGE;
}

// ---- pixel ----------------------------------------------------------------------------------------------------------
// edge from (xa, ya) to (xb, yb) at the sub-pixel point (px, py): > 0 inside a face of positive orientation
RENDER_HD int64_t render_edge(int64_t xa, int64_t ya, int64_t xb, int64_t yb, int64_t px, int64_t py) {
  return (xb - xa) * (py - ya) - (yb - ya) * (px - xa);
}

// top edge: horizontal with the interior below (y grows downwards); left edge: the interior to its right
RENDER_HD bool render_top_left(int64_t xa, int64_t ya, int64_t xb, int64_t yb) {
  const int64_t dx = xb - xa, dy = yb - ya;
  return dy < 0 || (dy == 0 && dx > 0);
}

RENDER_HD bool render_inside(int64_t e, bool top_left) { return e > 0 || (e == 0 && top_left); }

// Does the face cover the centre of pixel (ix, iy)?  e0, e1, e2: the weights of its three vertices (their sum is area).
RENDER_HD bool render_covers(const RenderFace& f, int ix, int iy, int64_t& e0, int64_t& e1, int64_t& e2) {
  const int64_t px = (int64_t)ix * RENDER_SUBPIXEL, py = (int64_t)iy * RENDER_SUBPIXEL;
  e0 = render_edge(f.x1, f.y1, f.x2, f.y2, px, py);
  e1 = render_edge(f.x2, f.y2, f.x0, f.y0, px, py);
  e2 = render_edge(f.x0, f.y0, f.x1, f.y1, px, py);
  return render_inside(e0, render_top_left(f.x1, f.y1, f.x2, f.y2)) &&
         render_inside(e1, render_top_left(f.x2, f.y2, f.x0, f.y0)) &&
         render_inside(e2, render_top_left(f.x0, f.y0, f.x1, f.y1));
}

RENDER_HD float render_depth(const RenderFace& f, int64_t e0, int64_t e1, int64_t e2) {
  const double s = ((double)e0 * f.d0 + (double)e1 * f.d1) + (double)e2 * f.d2;
  return (float)(s / (double)f.area);
}

// float32 bits in an order that unsigned comparison keeps: negative values below positive ones
RENDER_HD uint32_t render_monotone(float q) {
  const uint32_t b = render_bits(q);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

RENDER_HD uint64_t render_key(float q, int32_t face, int mode) {
  uint32_t m = render_monotone(q);
  if (mode == RENDER_LIST) m = ~m;                    // 1 / den: the larger value is the nearer one
  return ((uint64_t)m << 32) | (uint32_t)face;
}

RENDER_HD int32_t render_key_face(uint64_t key) { return key == RENDER_BACKGROUND_KEY ? -1 : (int32_t)(uint32_t)key; }

// the output depth of a pixel: Z (orthographic) or den = 1 / (1 / den) (LIST); +inf on background
RENDER_HD float render_key_depth(uint64_t key, int mode) {
  if (key == RENDER_BACKGROUND_KEY) return render_from_bits(0x7f800000u);
  uint32_t m = (uint32_t)(key >> 32);
  if (mode == RENDER_LIST) m = ~m;
  const float q = render_from_bits((m & 0x80000000u) ? (m & 0x7fffffffu) : ~m);
  return mode == RENDER_LIST ? (float)(1.0 / (double)q) : q;
}

// ---- shading --------------------------------------------------------------------------------------------------------
RENDER_HD int render_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// (b - a) x (c - a), in mesh coordinates
RENDER_HD void render_normal(const float* a, const float* b, const float* c, float* n) {
  const float u0 = b[0] - a[0], u1 = b[1] - a[1], u2 = b[2] - a[2];
  const float w0 = c[0] - a[0], w1 = c[1] - a[1], w2 = c[2] - a[2];
  n[0] = u1 * w2 - u2 * w1;
  n[1] = u2 * w0 - u0 * w2;
  n[2] = u0 * w1 - u1 * w0;
}

RENDER_HD float render_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// a unit component t in [-1, 1] -> round((t * 0.5 + 0.5) * 255), half up
RENDER_HD int render_unit_byte(float t) { return render_clip8((int)floorf((t * 0.5f + 0.5f) * 255.f + 0.5f)); }

// normal map: the unit normal's components as bytes; a face without a normal (zero or non-finite length) is mid grey
RENDER_HD void render_shade_normal(const float* n, int* rgb) {
  const float len = render_sqrt(render_dot(n, n));
  if (!(len > 0.f) || !render_finite(len)) { rgb[0] = rgb[1] = rgb[2] = 128; return; }
  for (int k = 0; k < 3; ++k) rgb[k] = render_unit_byte(render_div(n[k], len));
}

// head-light grey: |cos| of the angle between the normal and the line from the face's first vertex a to the camera's
// centre eye (homogeneous, mesh coordinates: eye[3] = 0 is a direction, the orthographic camera's)
RENDER_HD int render_shade_lambert(const float* n, const float* a, const float* eye) {
  float d[3];
  for (int k = 0; k < 3; ++k) d[k] = eye[k] - eye[3] * a[k];
  const float len = render_sqrt(render_dot(n, n)) * render_sqrt(render_dot(d, d));
  if (!(len > 0.f) || !render_finite(len)) return 0;
  float c = render_div(fabsf(render_dot(n, d)), len);
  if (!(c == c)) return 0;
  if (c > 1.f) c = 1.f;                               // rounding, or a dot product that overflowed
  return render_clip8((int)floorf(c * 255.f + 0.5f));
}

// alpha in 1/256 steps, 0 ... 256: 0 gives bg back, 256 gives fg
RENDER_HD int render_blend(int fg, int bg, int alpha256) { return (alpha256 * fg + (256 - alpha256) * bg + 128) >> 8; }
