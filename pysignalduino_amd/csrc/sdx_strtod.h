// sdx_strtod.h -- Python's float(str) for ASCII text, correctly rounded, one text for the host and
// for gfx950 (plain C++17, no HIP intrinsics).
//
//   int sdxf::py_float(p, n, scratch, &bits)
//     0  float() raises ValueError
//     1  bits = the binary64 pattern float() returns (round half to even; subnormals, +-0, +-inf,
//        nan with the sign CPython gives it)
//     2  a byte >= 0x80 (Python's Unicode digit / space handling is not modelled)
//
// Syntax (CPython float_from_string + _Py_string_to_number_with_underscores): ' ' and \t\n\v\f\r
// stripped (not \x1c-\x1f), '_' only between two digits,
//   [+-]? (digits [. digits] | . digits) ([eE] [+-]? digits)?   or   [+-]? (inf | infinity | nan).
//
// Step 1 is Clinger's fast path, as sdx_lines.hip's parse_pyfloat has it: at most 19 significant
// digits forming M < 2^53 and |exp10| <= 22, so M * 10^e (or M / 10^-e) is one IEEE operation on
// exact operands.  Everything else goes to the digit-array fallback below, which is exact for any
// number of digits and any exponent.  The caller provides the fallback's scratch (kScratch bytes);
// only the fallback touches it.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SDXF_HD __host__ __device__
#else
#define SDXF_HD
#endif
#define SDXF_FN SDXF_HD inline __attribute__((always_inline))

namespace sdxf {

// 768 significant digits and a sticky flag decide every rounding: the decimal expansion of a
// midpoint between two adjacent doubles, (2m + 1) * 2^t with t >= -1075, has at most 768
// significant digits, so a value whose first 768 digits are T and that has something non-zero
// behind them lies strictly between T and the next 768-digit number, and no midpoint does.
constexpr int kMaxDigits = 768;
// bytes of scratch per conversion: 201 words -- an odd number of 4-byte words, so that the lanes
// of a wave working at the same digit index of their own LDS column hit different banks
constexpr int kScratch = 804;
static_assert(kScratch >= kMaxDigits && kScratch % 4 == 0 && (kScratch / 4) % 2 == 1, "scratch layout");

// 0.d[0] d[1] ... d[nd-1] * 10^dp (d[0] != 0, d[nd-1] != 0) plus, when sticky, something positive
// below the last stored digit's place
struct Dec {
  uint8_t* d;
  int nd;
  int dp;
  bool sticky;
};

SDXF_FN void dec_trim(Dec& a) {
  while (a.nd > 0 && a.d[a.nd - 1] == 0) --a.nd;
}

// a *= 2^k, 1 <= k <= 60 (digit * 2^k + carry < 10 * 2^60 < 2^64).  Digits pushed past the buffer
// go into sticky.
SDXF_FN void dec_mul_pow2(Dec& a, int k) {
  uint64_t carry = 0;
  for (int i = a.nd - 1; i >= 0; --i) {
    const uint64_t x = ((uint64_t)a.d[i] << k) + carry;
    carry = x / 10;
    a.d[i] = (uint8_t)(x - carry * 10);
  }
  int c = 0;
  for (uint64_t t = carry; t; t /= 10) ++c;
  if (c) {
    int nn = a.nd + c;
    if (nn > kMaxDigits) {
      for (int i = kMaxDigits - c; i < a.nd; ++i)
        if (a.d[i]) a.sticky = true;
      nn = kMaxDigits;
    }
    for (int i = nn - 1; i >= c; --i) a.d[i] = a.d[i - c];
    for (int i = c - 1; i >= 0; --i) {
      a.d[i] = (uint8_t)(carry % 10);
      carry /= 10;
    }
    a.nd = nn;
    a.dp += c;
  }
  dec_trim(a);
}

// a /= 2^k, 1 <= k <= 60 (long division from the top; remainder * 10 + 9 < 10 * 2^60).  The
// quotient's digits that do not fit, or a remainder left when the buffer is full, go into sticky.
SDXF_FN void dec_div_pow2(Dec& a, int k) {
  const uint64_t mask = (1ull << k) - 1;
  uint64_t rem = 0;
  int w = 0, dp = a.dp;
  for (int r = 0; r < a.nd; ++r) {
    rem = rem * 10 + a.d[r];
    const uint64_t q = rem >> k;
    rem &= mask;
    if (w == 0 && q == 0) {  // a leading zero of the quotient
      --dp;
      continue;
    }
    a.d[w++] = (uint8_t)q;  // w <= r: in place
  }
  while (rem) {
    rem *= 10;
    const uint64_t q = rem >> k;
    rem &= mask;
    if (w == 0 && q == 0) {
      --dp;
      continue;
    }
    if (w == kMaxDigits) {  // q or the remainder behind it is non-zero
      a.sticky = true;
      break;
    }
    a.d[w++] = (uint8_t)q;
  }
  a.nd = w;
  a.dp = dp;
  dec_trim(a);
}

SDXF_FN uint64_t dec_int_part(const Dec& a) {  // floor(a), a < 2^63
  uint64_t v = 0;
  for (int i = 0; i < a.dp; ++i) v = 10 * v + (i < a.nd ? a.d[i] : 0);
  return v;
}

// the binary64 magnitude bits of a non-zero Dec, round half to even
SDXF_FN uint64_t dec_to_bits(Dec& a) {
  constexpr uint64_t kInf = 0x7FF0000000000000ull;
  if (a.dp > 310) return kInf;  // >= 10^309
  if (a.dp < -330) return 0;    // < 10^-330 < 2^-1075
  // value = a * 2^e2 throughout; every step multiplies or divides the digits by a power of two
  int e2 = 0;
  while (a.dp > 18) {  // a >= 10^18
    dec_div_pow2(a, 60);
    e2 += 60;
  }
  while (a.dp < 1) {  // a < 1
    dec_mul_pow2(a, 60);
    e2 -= 60;
  }
  // 1 <= a < 2^60: scale the integer part to exactly 53 bits
  {
    const uint64_t ip = dec_int_part(a);
    int len = 0;
    for (uint64_t t = ip; t; t >>= 1) ++len;
    const int s = 53 - len;
    if (s > 0) dec_mul_pow2(a, s);
    else if (s < 0) dec_div_pow2(a, -s);
    e2 -= s;
  }
  // 2^52 <= a < 2^53.  Below the normal range the last place is 2^-1074.
  if (e2 < -1074) {
    const int s = -1074 - e2;
    if (s > 60) return 0;  // a / 2^s < 2^-7: rounds to zero
    dec_div_pow2(a, s);
    e2 = -1074;
  }
  uint64_t m = a.dp > 0 ? dec_int_part(a) : 0;
  if (a.dp >= 0 && a.dp < a.nd) {  // the fraction's first digit (dp < 0: the fraction is < 0.1)
    const int f = a.d[a.dp];
    bool rest = a.sticky;
    for (int i = a.dp + 1; i < a.nd; ++i) rest = rest || a.d[i] != 0;
    if (f > 5 || (f == 5 && (rest || (m & 1)))) ++m;
  }
  if (m == (1ull << 53)) {
    m >>= 1;
    ++e2;
  }
  if (m < (1ull << 52)) return m;  // subnormal (e2 == -1074) or zero
  const int biased = e2 + 1075;    // m * 2^e2 = 1.f * 2^(e2 + 52)
  if (biased >= 2047) return kInf;
  return ((uint64_t)biased << 52) | (m & ((1ull << 52) - 1));
}

SDXF_FN bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
SDXF_FN bool is_ws(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }
SDXF_FN bool word_is(const uint8_t* p, const char* w, int n) {
  for (int k = 0; k < n; ++k) {
    uint8_t c = p[k];
    if (c >= 'A' && c <= 'Z') c = (uint8_t)(c + 32);
    if (c != (uint8_t)w[k]) return false;
  }
  return true;
}
SDXF_FN uint64_t double_bits(double x) {
  uint64_t b;
  __builtin_memcpy(&b, &x, 8);
  return b;
}

SDXF_FN int py_float(const uint8_t* p, int n, uint8_t* scratch, uint64_t* bits) {
  constexpr uint64_t kSign = 0x8000000000000000ull, kInf = 0x7FF0000000000000ull, kNan = 0x7FF8000000000000ull;
  constexpr int64_t kExpCap = 100000000000000000ll;  // exponent digits saturate past 10^17 (decides like any larger one)
  {
    uint8_t any = 0;
    for (int i = 0; i < n; ++i) any |= p[i];
    if (any & 0x80) return 2;
  }
  int s = 0, e = n;
  while (s < e && is_ws(p[s])) ++s;
  while (e > s && is_ws(p[e - 1])) --e;
  if (s == e) return 0;
  for (int i = s; i < e; ++i)
    if (p[i] == '_' && (i == s || i + 1 >= e || !is_digit(p[i - 1]) || !is_digit(p[i + 1]))) return 0;
  int i = s;
  bool neg = false;
  if (p[i] == '-' || p[i] == '+') {
    neg = p[i] == '-';
    ++i;
  }
  const uint64_t sign = neg ? kSign : 0;
  const int rem = e - i;
  if ((rem == 3 && word_is(p + i, "inf", 3)) || (rem == 8 && word_is(p + i, "infinity", 8))) {
    *bits = sign | kInf;
    return 1;
  }
  if (rem == 3 && word_is(p + i, "nan", 3)) {
    *bits = sign | kNan;
    return 1;
  }
  // ---- one pass over the text: the syntax, the first 19 significant digits, the exponent
  const int m0 = i;  // the mantissa's first character
  uint64_t M = 0;
  int sig = 0;
  int64_t e10 = 0;
  bool anyd = false, lost = false;
  bool frac = false;
  for (; i < e; ++i) {
    const uint8_t c = p[i];
    if (c == '.' && !frac) {
      frac = true;
      continue;
    }
    if (c == '_') continue;  // placed between two digits (checked above)
    if (!is_digit(c)) break;
    const int d = c - '0';
    anyd = true;
    if (M == 0 && d == 0) {
      if (frac) --e10;
    } else if (sig < 19) {
      M = 10 * M + (uint64_t)d;
      ++sig;
      if (frac) --e10;
    } else {
      if (d) lost = true;
      if (!frac) ++e10;
    }
  }
  if (!anyd) return 0;
  const int m1 = i;  // past the mantissa
  int64_t x10 = 0;
  if (i < e && (p[i] == 'e' || p[i] == 'E')) {
    int j = i + 1;
    bool eneg = false;
    if (j < e && (p[j] == '+' || p[j] == '-')) {
      eneg = p[j] == '-';
      ++j;
    }
    if (j < e && is_digit(p[j])) {  // otherwise the number ends before the 'e': trailing junk
      for (; j < e && (is_digit(p[j]) || p[j] == '_'); ++j)
        if (p[j] != '_' && x10 < kExpCap) x10 = 10 * x10 + (p[j] - '0');
      if (eneg) x10 = -x10;
      i = j;
    }
  }
  if (i != e) return 0;
  if (M == 0) {
    *bits = sign;
    return 1;
  }
  // ---- step 1: one exact IEEE operation
  if (!lost) {
    uint64_t Mt = M;
    int64_t et = e10 + x10;
    while (Mt % 10 == 0) {
      Mt /= 10;
      ++et;
    }
    if (Mt < (1ull << 53) && et >= -22 && et <= 22) {
      static constexpr double kPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
      const double v = et >= 0 ? (double)Mt * kPow10[et] : (double)Mt / kPow10[-et];
      *bits = sign | double_bits(v);
      return 1;
    }
  }
  // ---- step 2: the digits into the scratch (leading zeros dropped, 768 kept, the rest sticky)
  Dec a{scratch, 0, 0, false};
  int64_t dp = 0;  // grows by at most one per character
  frac = false;
  for (int k = m0; k < m1; ++k) {
    const uint8_t c = p[k];
    if (c == '.') {
      frac = true;
      continue;
    }
    if (c == '_') continue;
    const int d = c - '0';
    if (a.nd == 0 && d == 0) {
      if (frac) --dp;
      continue;
    }
    if (a.nd < kMaxDigits) a.d[a.nd++] = (uint8_t)d;
    else if (d) a.sticky = true;
    if (!frac) ++dp;
  }
  dec_trim(a);
  dp += x10;  // |dp| < 2^31 + 10^18 + 10: no overflow
  a.dp = dp > 1000 ? 1000 : dp < -1000 ? -1000 : (int)dp;
  *bits = sign | dec_to_bits(a);
  return 1;
}

}  // namespace sdxf
