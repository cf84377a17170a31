// The float64 logarithm of s2loss_kernels.hip.  Plain C++ (frexp, fma and IEEE division only), so the same text compiles
// for the host, where tests/csrc/s2loss_log_host.cpp holds it against libm's log over float32 arguments.
//
// The library's log(double) is built for every double and for a last-bit result: about 170 float64 instructions per call
// on gfx950, which made the occupancy sum compute-bound at five times its byte floor.  The arguments here are float32
// values widened to float64 (occ + 1e-8f and its mirror), so there are no float64 subnormals and nothing to gain from the
// last bit: the sum is rounded to float32 at the end.
//
//   x = 2^e m,  m in [sqrt(1/2), sqrt(2)),   s = (m - 1) / (m + 1),   z = s^2 <= 0.02944
//   log m = 2 atanh s = 2 s (1 + z/3 + z^2/5 + ... + z^9/19),   the first term left out is z^10/21 < 2.4e-17
//   log x = e ln 2 + log m
// Rounding: the division, z, nine fma, two products and the last fma with e ln 2 (|e ln 2| >= 0.69 > 2 |log m| whenever
// e != 0, so nothing cancels) -- within 4 ulps of float64 (2^-50 relative) for every finite x > 0.  log(+-0) = -inf,
// log(x < 0) = NaN, log(NaN) = NaN, log(+inf) = +inf, as libm has them.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define S2LOSS_HD __host__ __device__ __forceinline__
#else
#define S2LOSS_HD inline
#endif

S2LOSS_HD double s2loss_log(double x) {
  if (!(x > 0.0 && x < INFINITY)) return x == 0.0 ? -INFINITY : (x > 0.0 ? x : NAN);
  int e;
  double m = frexp(x, &e);                       // m in [1/2, 1)
  if (m < 0.70710678118654752440) {
    m *= 2.0;
    e -= 1;
  }
  const double s = (m - 1.0) / (m + 1.0), z = s * s;
  double p = 1.0 / 19.0;
  p = fma(p, z, 1.0 / 17.0);
  p = fma(p, z, 1.0 / 15.0);
  p = fma(p, z, 1.0 / 13.0);
  p = fma(p, z, 1.0 / 11.0);
  p = fma(p, z, 1.0 / 9.0);
  p = fma(p, z, 1.0 / 7.0);
  p = fma(p, z, 1.0 / 5.0);
  p = fma(p, z, 1.0 / 3.0);
  p = fma(p, z, 1.0);
  return fma((double)e, 0.69314718055994530942, (2.0 * s) * p);
}
