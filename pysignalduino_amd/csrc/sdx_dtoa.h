// sdx_dtoa.h -- Python's repr(float) / json.dumps(float), one text for the host and for gfx950
// (plain C++17, no HIP intrinsics).  The forward half of sdx_strtod.h.
//
//   int sdxf::py_repr(double x, bool json_form, uint8_t* out)     <= 24 bytes, returns the length
//   int sdxf::py_repr_to(double x, bool json_form, Sink& o)       the same bytes through o.put(c)
//
// Digits: the shortest decimal (1..17 digits) that float() converts back to x; of several, the one
// closest to x; a tie goes to the even digit (what CPython's float_repr_style 'short' prints).
// Found the Schubfach way (R. Giulietti, "The Schubfach way to render doubles", 2020): with
// x = c * 2^q and k = floor(log10(2^q)), the rounding interval of x and x itself are scaled by
// 10^-k with one 64 x 128-bit multiplication each, rounded to odd, which keeps every comparison
// with an even integer exact.  All of it lives in registers; the powers of ten come from the
// generated table sdx_dtoa_pow10.h (tools/gen_dtoa_pow10.py, which also proves that 128 bits
// decide every rounding).
//
// Format (CPython format_float_short, 'r'): the value is 0.d1...dn * 10^decpt;
// -4 < decpt <= 16 prints positionally (".0" appended to an integer), anything else as
// d1[.d2...dn]e[+-]XX with at least two exponent digits.
#pragma once

#include <cstdint>

#include "sdx_dtoa_pow10.h"

#if defined(__HIPCC__)
#define SDXD_HD __host__ __device__
#else
#define SDXD_HD
#endif
#define SDXD_FN SDXD_HD inline __attribute__((always_inline))

namespace sdxf {

struct Pow10 {
  uint64_t hi, lo;
};

// floor(log2(10^e)), |e| <= 400; floor(log10(2^e)) and floor(log10(3/4 * 2^e)), |e| <= 1100
// (compared with exact arithmetic by tools/gen_dtoa_pow10.py check())
SDXD_FN int floor_log2_pow10(int e) { return (e * 1741647) >> 19; }
SDXD_FN int floor_log10_pow2(int e) { return (e * 1262611) >> 22; }
SDXD_FN int floor_log10_34_pow2(int e) { return (e * 1262611 - 524031) >> 22; }

// floor(cp * g / 2^128), with bit 0 set when the product has anything at or above 2^60 below that
// (round to odd).  g is 10^K scaled into [2^127, 2^128) and rounded up, cp < 2^60: an exact product
// that is an integer leaves less than 2^60 behind, and no other comes within 2^-68 of an integer.
SDXD_FN uint64_t round_to_odd(const Pow10& g, uint64_t cp) {
  const unsigned __int128 x = (unsigned __int128)g.lo * cp;
  const unsigned __int128 y = (unsigned __int128)g.hi * cp + (uint64_t)(x >> 64);
  const uint64_t y0 = (uint64_t)y, x0 = (uint64_t)x;
  return (uint64_t)(y >> 64) | (uint64_t)(y0 != 0 || (x0 >> 60) != 0);
}

struct Dec17 {
  uint64_t digits;  // 1..17 digits, may end in zeros
  int exp10;        // value = digits * 10^exp10
};

// the shortest decimal of the finite non-zero double with the fraction field f and the exponent field e
SDXD_FN Dec17 shortest_decimal(uint64_t f, int e) {
  static constexpr Pow10 kPow10[SDXF_POW10_MAX - SDXF_POW10_MIN + 1] = {SDXF_POW10_TABLE};
  uint64_t c;
  int q;
  if (e != 0) {
    c = f | (1ull << 52);
    q = e - 1075;
  } else {
    c = f;
    q = -1074;
  }
  const bool even = (c & 1) == 0;
  const bool lower_closer = f == 0 && e > 1;  // a power of two: the lower neighbour is half as far
  const uint64_t cbl = 4 * c - 2 + (lower_closer ? 1 : 0), cb = 4 * c, cbr = 4 * c + 2;
  const int k = lower_closer ? floor_log10_34_pow2(q) : floor_log10_pow2(q);
  const int h = q + floor_log2_pow10(-k) + 1;  // 1..4
  const Pow10 g = kPow10[-k - SDXF_POW10_MIN];
  const uint64_t vbl = round_to_odd(g, cbl << h);
  const uint64_t vb = round_to_odd(g, cb << h);
  const uint64_t vbr = round_to_odd(g, cbr << h);
  // the interval's ends belong to it when c is even (float() rounds a tie to even)
  const uint64_t lower = vbl + (even ? 0 : 1), upper = vbr - (even ? 0 : 1);
  const uint64_t s = vb / 4;  // floor(x * 10^-k)
  if (s >= 10) {              // one digit fewer: 10 sp or 10 sp + 10 inside the interval?
    const uint64_t sp = s / 10;
    const bool up_in = lower <= 40 * sp, wp_in = 40 * sp + 40 <= upper;
    if (up_in != wp_in) return Dec17{sp + (wp_in ? 1 : 0), k + 1};
  }
  const bool u_in = lower <= 4 * s, w_in = 4 * s + 4 <= upper;
  if (u_in != w_in) return Dec17{s + (w_in ? 1 : 0), k};
  // both or neither: the closer of s and s + 1, a tie to the even one
  const uint64_t mid = 4 * s + 2;
  const bool up = vb > mid || (vb == mid && (s & 1));
  return Dec17{s + (up ? 1 : 0), k};
}

template <class S>
SDXD_FN int py_repr_to(double x, bool json_form, S& o) {
  uint64_t b;
  __builtin_memcpy(&b, &x, 8);
  const bool neg = (b >> 63) != 0;
  const int e = (int)((b >> 52) & 0x7FF);
  const uint64_t f = b & ((1ull << 52) - 1);
  int n = 0;
  auto put = [&](uint8_t ch) {
    o.put(ch);
    ++n;
  };
  auto lit = [&](const char* s) {
    while (*s) put((uint8_t)*s++);
  };
  if (e == 0x7FF) {
    if (f) {
      lit(json_form ? "NaN" : "nan");
    } else {
      if (neg) put('-');
      lit(json_form ? "Infinity" : "inf");
    }
    return n;
  }
  if (neg) put('-');
  if (e == 0 && f == 0) {
    lit("0.0");
    return n;
  }
  Dec17 d = shortest_decimal(f, e);
  while (d.digits % 10 == 0) {
    d.digits /= 10;
    ++d.exp10;
  }
  int nd = 1;
  uint64_t p = 1;  // 10^(nd - 1)
  while (d.digits / 10 >= p) {
    p *= 10;
    ++nd;
  }
  const int decpt = nd + d.exp10;
  uint64_t rest = d.digits;
  auto next_digit = [&]() {  // the digits from the top, without an array
    uint8_t dg = '0';
    while (rest >= p) {
      rest -= p;
      ++dg;
    }
    p /= 10;
    put(dg);
  };
  if (decpt > -4 && decpt <= 16) {
    if (decpt <= 0) {
      lit("0.");
      for (int i = decpt; i < 0; ++i) put('0');
      for (int i = 0; i < nd; ++i) next_digit();
    } else {
      for (int i = 0; i < decpt; ++i) {
        if (i < nd) next_digit();
        else put('0');
      }
      put('.');
      if (decpt >= nd) put('0');
      for (int i = decpt; i < nd; ++i) next_digit();
    }
  } else {
    next_digit();
    if (nd > 1) {
      put('.');
      for (int i = 1; i < nd; ++i) next_digit();
    }
    put('e');
    int ex = decpt - 1;
    put(ex < 0 ? '-' : '+');
    if (ex < 0) ex = -ex;
    if (ex >= 100) put((uint8_t)('0' + ex / 100));
    put((uint8_t)('0' + ex / 10 % 10));
    put((uint8_t)('0' + ex % 10));
  }
  return n;
}

struct PtrSink {
  uint8_t* p;
  SDXD_FN void put(uint8_t c) { *p++ = c; }
};

SDXD_FN int py_repr(double x, bool json_form, uint8_t* out) {
  PtrSink s{out};
  return py_repr_to(x, json_form, s);
}

}  // namespace sdxf
