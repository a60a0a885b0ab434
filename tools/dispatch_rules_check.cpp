// dispatch_rules_check.cpp -- the validator of sdx_dispatch_rules
// (pysignalduino_amd/csrc/sdx_dispatch_layout.h) under the address and UB sanitizers, stand-alone:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/dispatch_rules_check.cpp -o dispatch_rules_check && ./dispatch_rules_check rules.bin 129 66 12 19
//
// rules.bin: the 152 bytes of a struct pysignalduino_amd.dispatch.DispatchRules.struct filled; then the bank's
// four class counts (MU MS MC MN).  Every candidate is copied into a heap block of exactly sizeof(struct) bytes,
// so a validator that read past it trips the sanitizer.  The good struct must pass; every damaged one must be
// refused: for every kind and every mask word the first bit at or above the class count and the word's last
// bit, the class count of a smaller bank under a set bit, a negative cap, a non-zero reserved word, class
// counts above 256, null arguments.  What must stay legal: every bit below the class count, caps 0 and
// INT32_MAX, any drop_equal.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../pysignalduino_amd/csrc/sdx_dispatch_layout.h"

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                      \
    }                                                                \
  } while (0)

// validate a copy of r that owns exactly sizeof r bytes, with counts that own exactly 16
static const char* verdict(const sdx_dispatch_rules& r, const uint32_t (&n_class)[4]) {
  sdx_dispatch_rules* p = static_cast<sdx_dispatch_rules*>(std::malloc(sizeof r));
  uint32_t* c = static_cast<uint32_t*>(std::malloc(sizeof n_class));
  if (!p || !c) std::abort();
  std::memcpy(p, &r, sizeof r);
  std::memcpy(c, n_class, sizeof n_class);
  const char* why = sdx_dispatch_validate(p, c);
  std::free(p);
  std::free(c);
  return why;
}

int main(int argc, char** argv) {
  static_assert(sizeof(sdx_dispatch_rules) == 152, "the struct's size");
  CHECK(argc == 6);
  std::FILE* fh = std::fopen(argv[1], "rb");
  CHECK(fh != nullptr);
  sdx_dispatch_rules good;
  const size_t got = std::fread(&good, 1, sizeof good, fh);
  const bool at_end = std::fgetc(fh) == EOF;
  std::fclose(fh);
  CHECK(got == sizeof good && at_end);
  uint32_t nc[4];
  for (int kd = 0; kd < 4; ++kd) nc[kd] = (uint32_t)std::strtoul(argv[2 + kd], nullptr, 10);
  const char* why = verdict(good, nc);
  if (why) std::fprintf(stderr, "the good struct: %s\n", why);
  CHECK(why == nullptr);
  CHECK(sdx_dispatch_validate(nullptr, nc) != nullptr);
  CHECK(sdx_dispatch_validate(&good, nullptr) != nullptr);

  int refused = 0, legal = 0;
  for (int kd = 0; kd < 4; ++kd) {
    const uint32_t c = nc[kd];
    CHECK(c <= SDX_DISPATCH_CLASS_MAX);
    for (uint32_t b = 0; b < 256; ++b) {  // every single bit: legal below the class count, refused from it on
      sdx_dispatch_rules r = good;
      r.keep_equal[kd][b >> 6] |= 1ull << (b & 63);
      CHECK((verdict(r, nc) == nullptr) == (b < c));
      b < c ? ++legal : ++refused;
    }
    if (c > 0) {  // the last legal bit is refused by the class count of a smaller bank
      sdx_dispatch_rules r = good;
      r.keep_equal[kd][(c - 1) >> 6] |= 1ull << ((c - 1) & 63);
      uint32_t smaller[4] = {nc[0], nc[1], nc[2], nc[3]};
      smaller[kd] = c - 1;
      CHECK(verdict(r, nc) == nullptr && verdict(r, smaller) != nullptr);
      ++refused;
    }
    {  // all four words full: legal only for a kind of 256 classes
      sdx_dispatch_rules r = good;
      for (int w = 0; w < 4; ++w) r.keep_equal[kd][w] = ~0ull;
      CHECK((verdict(r, nc) == nullptr) == (c == 256));
      uint32_t full[4] = {nc[0], nc[1], nc[2], nc[3]};
      full[kd] = 256;
      CHECK(verdict(r, full) == nullptr);
      full[kd] = 257;
      CHECK(verdict(good, full) != nullptr);  // a class count above 256
      full[kd] = 0xFFFFFFFFu;
      CHECK(verdict(good, full) != nullptr);
      refused += 2;
    }
    for (int32_t cap : {-1, INT_MIN, -4}) {
      sdx_dispatch_rules r = good;
      r.max_repeat[kd] = cap;
      CHECK(verdict(r, nc) != nullptr);
      ++refused;
    }
    for (int32_t cap : {0, 1, 4, INT_MAX}) {
      sdx_dispatch_rules r = good;
      r.max_repeat[kd] = cap;
      CHECK(verdict(r, nc) == nullptr);
      ++legal;
    }
  }
  for (int32_t x : {1, -1, INT_MIN, 0x100}) {
    sdx_dispatch_rules r = good;
    r.res = x;
    CHECK(verdict(r, nc) != nullptr);
    ++refused;
  }
  for (int32_t x : {0, 1, -1, INT_MAX}) {
    sdx_dispatch_rules r = good;
    r.drop_equal = x;
    CHECK(verdict(r, nc) == nullptr);
    ++legal;
  }
  {  // an empty bank: no bit is legal, the empty masks are
    sdx_dispatch_rules r{};
    const uint32_t none[4] = {0, 0, 0, 0};
    CHECK(verdict(r, none) == nullptr);
    r.keep_equal[2][0] = 1;
    CHECK(verdict(r, none) != nullptr);
  }
  std::printf("dispatch_rules_check: ok (sizeof %zu, %d damaged structs refused, %d legal ones passed)\n", sizeof good,
              refused, legal);
  return 0;
}
