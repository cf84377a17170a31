// Host check of csrc/s2loss_math.h (built and run by tests/test_s2loss_cpu.py): s2loss_log against libm's log on float32
// arguments widened to float64 -- every 29th float32 in [2^-31, 4), which holds every occ + 1e-8f of a valid occupancy, and
// every 8191st of the other positive ones, subnormals included.  Prints the worst error in float64 ulps of the result
// and the non-finite cases.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "s2loss_math.h"

int main() {
  double worst = 0.0;
  float at = 0.0f;
  long n = 0;
  for (uint32_t b = 1u; b < 0x7f800000u; b += (b >= 0x30000000u && b < 0x40800000u) ? 29u : 8191u) {
    float f;
    memcpy(&f, &b, 4);
    const double x = (double)f, want = log(x), got = s2loss_log(x);
    const double err = want == 0.0 ? (got == 0.0 ? 0.0 : INFINITY) : fabs(got - want) / ldexp(1.0, ilogb(want) - 52);
    if (!(err <= worst)) worst = err, at = f;
    ++n;
  }
  printf("values %ld\nworst_ulps %.3f\nat %.9g\n", n, worst, at);
  printf("specials %g %g %g %g %g %g\n", s2loss_log(0.0), s2loss_log(-0.0), s2loss_log(-1e-3), s2loss_log(NAN),
         s2loss_log(INFINITY), s2loss_log(1.0));
  return 0;
}
