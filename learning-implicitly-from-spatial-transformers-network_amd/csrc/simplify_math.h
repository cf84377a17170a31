// Every per-vertex and per-cluster rule of the vertex-clustering simplifier (include/list_simplify.h), written once for
// simplify_kernels.hip and for tests/csrc/simplify_host.cpp; simplify.py restates the same rules in numpy.  Plain C++
// (IEEE float64 arithmetic, floor and llrint only); build with -ffp-contract=off: every operation is rounded on its
// own, no product is fused into a sum.
//
// The rule.  The box [lo, hi) is cut into R0 x R1 x R2 cells; the host computes inv[a] = Ra / (hi[a] - lo[a]) and
// cell[a] = (hi[a] - lo[a]) / Ra in float64 and hands the doubles over, so both sides hold the same bits.
//   vertex   per axis, in float64: t = (double)v - lo; u = clamp(t * inv, 0, R) (a vertex outside the box goes onto
//            the box face); i = min((int64)floor(u), R - 1); q = llrint((u - i) * 2^30), ties to even, 0 <= q <= 2^30.
//            key = (i0 * R1 + i1) * R2 + i2 < 2^30.  A vertex with a non-finite coordinate is invalid: in no cluster.
//   cluster  the valid vertices of one key, numbered in ascending key; per axis S = sum of q (int64, at most
//            2^31 * 2^30) and n = their count.
//   point    a = S / n, r = S % n (integers); m = ((double)a + (double)r / (double)n) * 2^-30;
//            p = (float)(lo + ((double)i + m) * cell).  Every integer-to-double conversion is exact.
//   face     invalid with an index outside [0, V) or an invalid corner; degenerate (dropped) unless its three corners
//            lie in three different clusters; else kept in its order and orientation with cluster numbers for corners.
//            Duplicate faces and opposite pairs are ordinary faces and stay.
//   output   clusters that no kept face uses are dropped, the rest renumbered in ascending key.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SIMP_HD __host__ __device__ __forceinline__
#else
#define SIMP_HD inline
#endif

enum { SIMP_MAX_CELLS = 1024, SIMP_Q_BITS = 30 };
// the totals record (include/list_simplify.h)
enum {
  SIMP_OUT_VERTS = 0, SIMP_OUT_FACES = 1, SIMP_CLUSTERS = 2, SIMP_INVALID_VERTS = 3, SIMP_INVALID_FACES = 4,
  SIMP_DEGENERATE_FACES = 5, SIMP_N_TOTALS = 6
};

#define SIMP_Q_ONE 1073741824.0                        /* 2^30 */
#define SIMP_Q_INV 9.31322574615478515625e-10          /* 2^-30 */

SIMP_HD bool simp_finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }

SIMP_HD bool simp_valid_vertex(const float* v) { return simp_finite(v[0]) && simp_finite(v[1]) && simp_finite(v[2]); }

SIMP_HD double simp_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ddiv_rn(a, b);
#else
  return a / b;
#endif
}

// One finite coordinate on one axis -> its cell i in [0, R) and its offset q in [0, 2^30] inside that cell
SIMP_HD void simp_axis(float v, double lo, double inv, int32_t R, int32_t* i, int32_t* q) {
  const double t = (double)v - lo;
  double u = t * inv;
  u = u < 0.0 ? 0.0 : u;
  u = u > (double)R ? (double)R : u;
  int64_t c = (int64_t)floor(u);
  c = c < R - 1 ? c : R - 1;
  *i = (int32_t)c;
  *q = (int32_t)llrint((u - (double)c) * SIMP_Q_ONE);
}

SIMP_HD uint32_t simp_key(int32_t i0, int32_t i1, int32_t i2, int32_t R1, int32_t R2) {
  return ((uint32_t)i0 * (uint32_t)R1 + (uint32_t)i1) * (uint32_t)R2 + (uint32_t)i2;
}

SIMP_HD void simp_key_cell(uint32_t key, int32_t R1, int32_t R2, int32_t i[3]) {
  i[2] = (int32_t)(key % (uint32_t)R2);
  const uint32_t k = key / (uint32_t)R2;
  i[1] = (int32_t)(k % (uint32_t)R1);
  i[0] = (int32_t)(k / (uint32_t)R1);
}

// A cluster's representative on one axis from the integer sum S of its n >= 1 offsets in cell i
SIMP_HD float simp_point(int64_t S, int64_t n, int32_t i, double lo, double cell) {
  const int64_t a = S / n, r = S % n;
  const double m = ((double)a + simp_div((double)r, (double)n)) * SIMP_Q_INV;
  return (float)(lo + ((double)i + m) * cell);
}
