// The text of a Wavefront .obj line (include/list_objtext.h), written once for objtext_kernels.hip, for
// list_objtext_host and for tests/csrc/objtext_host.cpp; objtext.py restates the same integer arithmetic in numpy.
// Integer arithmetic on the bit pattern only: no float operation, no double, no printf, no library call, so no
// rounding or denormal mode can change a byte.
//
// The rule (what utils.write_obj's f-strings print).
//   vertex   "v " s(x) " " s(y) " " s(z) "\n"
//   face     "f " d(a+1) " " d(b+1) " " d(c+1) "\n",  d = the decimal of the index + 1 computed in int64
//   s(x)     what an f-string makes of a numpy.float32: format(x, "") hands the value to Python's float, so the text is
//            repr(float(x)), the shortest digits of the WIDENED value as a float64 -- 0.1f prints 0.10000000149011612.
//            nan (either sign, any payload), inf, -inf, 0.0, -0.0; else the shortest digits d1..dn (1 <= n <= 17) and
//            exponent that lie in the float64's rounding interval: it ends at the midpoints to the neighbouring
//            float64s (the lower half is half as wide when the float64's significand field is 0, i.e. x is a power of
//            two), ends included iff the 53-bit significand is even, which it always is for a widened float32 with 29
//            zero bits behind it; among the shortest the closest to x (Ryu, Adams 2018, float64).
//   layout   on the digits: with x = d1.d2..dn * 10^e, -4 <= e < 16 is positional, at least one digit on each side of
//            the point, zeros up to the point and then ".0"; else d1[.d2..dn]e+XX / e-XX with two exponent digits
//            (a float32's exponent never needs three).
//   bounds   a token is at most 23 bytes, a vertex line at most 74, a face line at most 38.
//
// Bytes leave through a sink (`void put(uint8_t)`): the kernel's writes into LDS, the host's into memory.  Digits
// travel as packed BCD in two words (the low eight digits, the rest): no indexed local array, so nothing of this goes to
// scratch memory on the device.
#pragma once

#include <stdint.h>

#include "objtext_tables.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OBJTEXT_HD __host__ __device__ __forceinline__
#else
#define OBJTEXT_HD inline
#endif

enum { OBJTEXT_MAX_TOKEN = 23, OBJTEXT_MAX_VERTEX_LINE = 74, OBJTEXT_MAX_FACE_LINE = 38 };

// A finite non-zero value as decimal: value = digits * 10^exp10, digits has n decimal digits
struct ObjtextDecimal {
  uint64_t digits;
  int32_t exp10;
  int32_t n;
};

OBJTEXT_HD int32_t objtext_pow5bits(int32_t e) { return (int32_t)(((uint32_t)e * 1217359u) >> 19) + 1; }     // 0 <= e <= 3528
OBJTEXT_HD int32_t objtext_log10pow2(int32_t e) { return (int32_t)(((uint32_t)e * 78913u) >> 18); }           // 0 <= e <= 1650
OBJTEXT_HD int32_t objtext_log10pow5(int32_t e) { return (int32_t)(((uint32_t)e * 732923u) >> 20); }          // 0 <= e <= 2620

// 5^p divides v (v > 0)
OBJTEXT_HD bool objtext_multiple_of_pow5(uint64_t v, int32_t p) {
  int32_t c = 0;
  while (v % 5u == 0u) {
    v /= 5u;
    ++c;
  }
  return c >= p;
}

// a * b as (high, low) 64-bit words, from 32-bit halves
OBJTEXT_HD uint64_t objtext_mul64(uint64_t a, uint64_t b, uint64_t* high) {
  const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
  *high = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
  return (uint64_t)(uint32_t)p00 | (mid << 32);
}

// floor(m * f / 2^shift) for the 128-bit f = {low, high}, 64 < shift < 128, the result below 2^64
OBJTEXT_HD uint64_t objtext_mulshift(uint64_t m, const uint64_t* f, int32_t shift) {
  uint64_t h0, h1;
  objtext_mul64(m, f[0], &h0);
  const uint64_t l1 = objtext_mul64(m, f[1], &h1);
  const uint64_t sum = h0 + l1;
  h1 += sum < h0 ? 1u : 0u;
  const int32_t d = shift - 64;
  return (h1 << (64 - d)) | (sum >> d);
}

OBJTEXT_HD int32_t objtext_ndigits(uint64_t v) {       // v < 10^19
  int32_t n = 1;
  for (uint64_t p = 10u; n < 19 && v >= p; p *= 10u) ++n;
  return n;
}

// bits of a finite non-zero float32 (the sign ignored) -> the shortest decimal of the float64 of the same value
OBJTEXT_HD ObjtextDecimal objtext_shortest(uint32_t bits) {
  // widen: the float64's exponent and significand fields (a float32 subnormal is a normal float64)
  uint32_t mant = bits & 0x7fffffu;
  int32_t expo = (int32_t)((bits >> 23) & 0xffu);
  if (expo == 0) {
    expo = 1;
    while ((mant & 0x800000u) == 0u) {
      mant <<= 1;
      --expo;
    }
    mant &= 0x7fffffu;
  }
  const uint64_t field = (uint64_t)mant << 29;
  const int32_t e2 = expo + 896 - 1023 - 52 - 2;                    // -203 .. 73
  const uint64_t m2 = field | ((uint64_t)1 << 52);                  // even: the interval's ends are always included
  const uint64_t mm_shift = field != 0u ? 1u : 0u;
  const uint64_t mv = 4u * m2, mp = mv + 2u, mm = mv - 1u - mm_shift;

  uint64_t vr, vp, vm;
  int32_t e10;
  bool vm_zeros = false, vr_zeros = false;
  if (e2 >= 0) {
    const int32_t q = objtext_log10pow2(e2) - (e2 > 3 ? 1 : 0);
    e10 = q;
    const int32_t shift = -e2 + q + OBJTEXT_POW5_BITS + objtext_pow5bits(q) - 1;
    const uint64_t* f = kObjtextPow5Inv[q];
    vr = objtext_mulshift(mv, f, shift);
    vp = objtext_mulshift(mp, f, shift);
    vm = objtext_mulshift(mm, f, shift);
    if (q <= 21) {
      if (mv % 5u == 0u) vr_zeros = objtext_multiple_of_pow5(mv, q);
      else vm_zeros = objtext_multiple_of_pow5(mm, q);
    }
  } else {
    const int32_t q = objtext_log10pow5(-e2) - (-e2 > 1 ? 1 : 0);
    e10 = q + e2;
    const int32_t i = -e2 - q;
    const int32_t shift = q - (objtext_pow5bits(i) - OBJTEXT_POW5_BITS);
    const uint64_t* f = kObjtextPow5[i];
    vr = objtext_mulshift(mv, f, shift);
    vp = objtext_mulshift(mp, f, shift);
    vm = objtext_mulshift(mm, f, shift);
    if (q <= 1) {
      vr_zeros = true;                              // mv = 4 * m2 has at least q trailing zero bits
      vm_zeros = mm_shift == 1u;
    } else if (q < 63) {
      vr_zeros = (mv & (((uint64_t)1 << q) - 1u)) == 0u;
    }
  }

  int32_t removed = 0;
  uint32_t last = 0u;
  while (vp / 10u > vm / 10u) {
    vm_zeros &= vm % 10u == 0u;
    vr_zeros &= last == 0u;
    last = (uint32_t)(vr % 10u);
    vr /= 10u;
    vp /= 10u;
    vm /= 10u;
    ++removed;
  }
  if (vm_zeros) {                                   // the interval's lower end is itself a short decimal, and included
    while (vm % 10u == 0u) {
      vr_zeros &= last == 0u;
      last = (uint32_t)(vr % 10u);
      vr /= 10u;
      vp /= 10u;
      vm /= 10u;
      ++removed;
    }
  }
  if (vr_zeros && last == 5u && vr % 2u == 0u) last = 4u;             // exactly half: to even
  ObjtextDecimal d;
  d.digits = vr + (((vr == vm && !vm_zeros) || last >= 5u) ? 1u : 0u);
  d.exp10 = e10 + removed;
  d.n = objtext_ndigits(d.digits);
  return d;
}

// Decimal digits as packed BCD: lo holds the low eight digits, hi the (up to eleven) digits above them
struct ObjtextBcd {
  uint64_t hi;
  uint32_t lo;
};

OBJTEXT_HD ObjtextBcd objtext_bcd(uint64_t v) {          // v < 10^19
  uint32_t low = (uint32_t)(v % 100000000u);
  uint64_t high = v / 100000000u;
  ObjtextBcd b = {0u, 0u};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    b.lo |= (low % 10u) << (4 * i);
    low /= 10u;
  }
#pragma unroll
  for (int i = 0; i < 11; ++i) {
    b.hi |= (high % 10u) << (4 * i);
    high /= 10u;
  }
  return b;
}

// The character of the digit r places from the right
OBJTEXT_HD uint8_t objtext_digit(ObjtextBcd b, int32_t r) {
  const uint32_t d = r >= 8 ? (uint32_t)(b.hi >> (4 * (r - 8))) : b.lo >> (4 * r);
  return (uint8_t)('0' + (d & 15u));
}

// What a token is
enum { OBJTEXT_NAN = 0, OBJTEXT_INF = 1, OBJTEXT_ZERO = 2, OBJTEXT_NUMBER = 3 };

OBJTEXT_HD int32_t objtext_class(uint32_t bits) {
  const uint32_t a = bits & 0x7fffffffu;
  if (a > 0x7f800000u) return OBJTEXT_NAN;
  if (a == 0x7f800000u) return OBJTEXT_INF;
  return a == 0u ? OBJTEXT_ZERO : OBJTEXT_NUMBER;
}

// d1.d2..dn * 10^e is written positionally iff -4 <= e < 16
OBJTEXT_HD bool objtext_positional(ObjtextDecimal d) {
  const int32_t e = d.exp10 + d.n - 1;
  return e >= -4 && e < 16;
}

// Byte length of s(x)
OBJTEXT_HD int32_t objtext_f32_len(uint32_t bits) {
  const int32_t cls = objtext_class(bits), sign = (int32_t)(bits >> 31);
  if (cls != OBJTEXT_NUMBER) return cls == OBJTEXT_NAN ? 3 : 3 + sign;
  const ObjtextDecimal d = objtext_shortest(bits);
  if (!objtext_positional(d)) return sign + (d.n > 1 ? d.n + 1 : 1) + 4;
  if (d.exp10 >= 0) return sign + d.n + d.exp10 + 2;
  return sign + (d.exp10 > -d.n ? d.n + 1 : 2 - d.exp10);
}

// s(x) into the sink, byte by byte
template <class Sink> OBJTEXT_HD void objtext_f32_put(uint32_t bits, Sink& o) {
  const int32_t cls = objtext_class(bits);
  if (cls == OBJTEXT_NAN) {
    o.put('n'), o.put('a'), o.put('n');
    return;
  }
  if (bits >> 31) o.put('-');
  if (cls == OBJTEXT_INF) {
    o.put('i'), o.put('n'), o.put('f');
    return;
  }
  if (cls == OBJTEXT_ZERO) {
    o.put('0'), o.put('.'), o.put('0');
    return;
  }
  const ObjtextDecimal d = objtext_shortest(bits);
  const ObjtextBcd bcd = objtext_bcd(d.digits);
  const int32_t n = d.n;
  int32_t r = n - 1;                                // the next digit, counted from the right
  if (!objtext_positional(d)) {
    o.put(objtext_digit(bcd, r));
    if (n > 1) {
      o.put('.');
      for (--r; r >= 0; --r) o.put(objtext_digit(bcd, r));
    }
    int32_t e = d.exp10 + n - 1;                    // 16 <= |e| <= 45
    o.put('e');
    o.put(e < 0 ? '-' : '+');
    e = e < 0 ? -e : e;
    o.put((uint8_t)('0' + e / 10));
    o.put((uint8_t)('0' + e % 10));
    return;
  }
  if (d.exp10 >= 0) {                               // an integer: digits, zeros, ".0"
    for (; r >= 0; --r) o.put(objtext_digit(bcd, r));
    for (int32_t z = 0; z < d.exp10; ++z) o.put('0');
    o.put('.'), o.put('0');
  } else if (d.exp10 > -n) {                        // the point inside the digits, before the last -exp10 of them
    for (; r >= 0; --r) {
      o.put(objtext_digit(bcd, r));
      if (r == -d.exp10) o.put('.');
    }
  } else {                                          // "0." zeros digits
    o.put('0'), o.put('.');
    for (int32_t z = -d.exp10 - n; z > 0; --z) o.put('0');
    for (; r >= 0; --r) o.put(objtext_digit(bcd, r));
  }
}

// d(a + 1): the index plus one in int64, so INT32_MAX gives 2147483648 (the Python loop's own int32 sum overflows there)
OBJTEXT_HD int32_t objtext_index_len(int32_t a) {
  const int64_t v = (int64_t)a + 1;
  return (v < 0 ? 1 : 0) + objtext_ndigits((uint64_t)(v < 0 ? -v : v));
}

template <class Sink> OBJTEXT_HD void objtext_index_put(int32_t a, Sink& o) {
  const int64_t v = (int64_t)a + 1;
  const uint64_t u = (uint64_t)(v < 0 ? -v : v);
  if (v < 0) o.put('-');
  const ObjtextBcd bcd = objtext_bcd(u);
  for (int32_t r = objtext_ndigits(u) - 1; r >= 0; --r) o.put(objtext_digit(bcd, r));
}

// Whole lines.  v: the three coordinates' bits; f: the three indices.
OBJTEXT_HD int32_t objtext_vertex_len(const uint32_t* v) {
  return 5 + objtext_f32_len(v[0]) + objtext_f32_len(v[1]) + objtext_f32_len(v[2]);
}

OBJTEXT_HD int32_t objtext_face_len(const int32_t* f) {
  return 5 + objtext_index_len(f[0]) + objtext_index_len(f[1]) + objtext_index_len(f[2]);
}

template <class Sink> OBJTEXT_HD void objtext_vertex_put(const uint32_t* v, Sink& o) {
  o.put('v');
  for (int a = 0; a < 3; ++a) {
    o.put(' ');
    objtext_f32_put(v[a], o);
  }
  o.put('\n');
}

template <class Sink> OBJTEXT_HD void objtext_face_put(const int32_t* f, Sink& o) {
  o.put('f');
  for (int a = 0; a < 3; ++a) {
    o.put(' ');
    objtext_index_put(f[a], o);
  }
  o.put('\n');
}

// The whole file on the host: at most `cap` bytes go to out, the file's full length comes back.  list_objtext_host and
// tests/csrc/objtext_host.cpp are this function.
struct ObjtextHostSink {
  uint8_t* out;
  int64_t cap, pos;
  void put(uint8_t c) {
    if (pos < cap) out[pos] = c;
    ++pos;
  }
};

inline int64_t objtext_host_file(const float* verts, const int32_t* faces, int64_t V, int64_t F, uint8_t* out, int64_t cap) {
  ObjtextHostSink sink = {out, cap, 0};
  for (int64_t v = 0; v < V; ++v) {
    uint32_t w[3];
    __builtin_memcpy(w, verts + 3 * v, sizeof(w));
    objtext_vertex_put(w, sink);
  }
  for (int64_t f = 0; f < F; ++f) objtext_face_put(faces + 3 * f, sink);
  return sink.pos;
}
