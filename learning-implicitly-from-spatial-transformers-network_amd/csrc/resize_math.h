// Pillow 12's bilinear resample of 8-bit pixels (include/list_resize.h is the text), written once for resize_kernels.hip,
// for the host-only list_resize_plan / list_resize_host and for tests/csrc/resize_host.cpp.  Plain C++ (IEEE float64
// arithmetic and ceil only); build with -ffp-contract=off: every operation rounds on its own.
//
// The coefficients of an axis are made in float64 and turned into 22-bit fixed point (the host does that, where the plan
// is made); a pass is then integer multiply-adds and one clip per output (host and device alike).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RESIZE_HD __host__ __device__ __forceinline__
#else
#define RESIZE_HD inline
#endif

enum { RESIZE_PRECISION_BITS = 22 };
enum { RESIZE_COPY = 0, RESIZE_HORIZONTAL = 1, RESIZE_VERTICAL = 2 };      // what a stage does

RESIZE_HD double resize_triangle(double t) {
  if (t < 0.0) t = -t;
  return t < 1.0 ? 1.0 - t : 0.0;
}

// taps per output of the axis n_in -> n_out: (int)ceil(support) * 2 + 1, support = max(n_in / n_out, 1)
RESIZE_HD int resize_ksize(int n_in, int n_out) {
  double fs = (double)n_in / (double)n_out;
  if (fs < 1.0) fs = 1.0;
  const double support = 1.0 * fs;
  return (int)ceil(support) * 2 + 1;
}

// Output xx of the axis n_in -> n_out: first source index, tap count (<= ksize) and the fixed-point weights K[0 ... ksize)
// (zero beyond the count).  `w` is scratch of ksize doubles.  Returns the weights' sum.
RESIZE_HD int64_t resize_coeffs(int n_in, int n_out, int xx, int ksize, int32_t* first, int32_t* count, int32_t* K, double* w) {
  const double scale = (double)n_in / (double)n_out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * fs;
  const double center = ((double)xx + 0.5) * scale;
  const double ss = 1.0 / fs;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > n_in) xmax = n_in;
  xmax -= xmin;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) {
    w[x] = resize_triangle(((double)(x + xmin) - center + 0.5) * ss);
    ww += w[x];
  }
  int64_t sum = 0;
  for (int x = 0; x < ksize; ++x) {
    double k = 0.0;
    if (x < xmax) k = ww != 0.0 ? w[x] / ww : w[x];
    K[x] = k < 0.0 ? (int32_t)(-0.5 + k * (double)(1 << RESIZE_PRECISION_BITS))
                   : (int32_t)(0.5 + k * (double)(1 << RESIZE_PRECISION_BITS));
    sum += K[x];
  }
  *first = xmin, *count = xmax;
  return sum;
}

// An accumulator starts at one half and ends as a level: clip(acc >> 22, 0, 255)
RESIZE_HD int resize_acc0() { return 1 << (RESIZE_PRECISION_BITS - 1); }
RESIZE_HD int resize_level(int acc) {
  const int v = acc >> RESIZE_PRECISION_BITS;
  return v < 0 ? 0 : v > 255 ? 255 : v;
}

// The two stages of H x W -> out_h x out_w: stage[0] from the source to the intermediate (mid_h x mid_w), stage[1] from
// there to the output.  Equal sizes copy twice; Pillow's tall-image rule runs the vertical pass first; a pass whose axis
// already has its size is a copy (and moves to the second stage, so that the intermediate is the small one).
RESIZE_HD void resize_stages(int H, int W, int out_h, int out_w, int32_t stage[2], int32_t* mid_h, int32_t* mid_w) {
  const bool need_h = W != out_w, need_v = H != out_h;
  const bool vertical_first = (int64_t)H > 100 * (int64_t)W && out_h < H;
  if (need_h && need_v) {
    stage[0] = vertical_first ? RESIZE_VERTICAL : RESIZE_HORIZONTAL;
    stage[1] = vertical_first ? RESIZE_HORIZONTAL : RESIZE_VERTICAL;
  } else {
    stage[0] = need_h ? RESIZE_HORIZONTAL : need_v ? RESIZE_VERTICAL : RESIZE_COPY;
    stage[1] = RESIZE_COPY;
  }
  *mid_h = stage[0] == RESIZE_HORIZONTAL ? H : out_h;
  *mid_w = stage[0] == RESIZE_VERTICAL ? W : out_w;
  if (stage[0] == RESIZE_COPY) *mid_h = H, *mid_w = W;
}

// One pass over uint8 pixels [in_h][in_w][3] -> [o_h][o_w][3] with the axis' tables: bounds [n_out][2] = (first, count),
// weights [n_out][ksize].
inline void resize_pass_host(const uint8_t* in, int in_w, uint8_t* out, int o_h, int o_w, int axis, const int32_t* bounds,
                             const int32_t* weights, int ksize) {
  for (int y = 0; y < o_h; ++y)
    for (int x = 0; x < o_w; ++x)
      for (int c = 0; c < 3; ++c) {
        int level;
        if (axis == RESIZE_COPY) {
          level = in[((int64_t)y * in_w + x) * 3 + c];
        } else {
          const int o = axis == RESIZE_HORIZONTAL ? x : y;
          const int first = bounds[2 * o], count = bounds[2 * o + 1];
          const int32_t* K = weights + (int64_t)o * ksize;
          int acc = resize_acc0();
          for (int k = 0; k < count; ++k) {
            const int64_t at = axis == RESIZE_HORIZONTAL ? (int64_t)y * in_w + first + k : (int64_t)(first + k) * in_w + x;
            acc += (int)in[at * 3 + c] * K[k];
          }
          level = resize_level(acc);
        }
        out[((int64_t)y * o_w + x) * 3 + c] = (uint8_t)level;
      }
}
