// Host driver of pysignalduino_amd/csrc/sdx_strtod.h for tests/test_strtod_host.py: one hex-encoded
// string per input line; prints "<class> <16 hex digits of the value>" per line.  Every string and
// the scratch live in exact-size heap blocks, so AddressSanitizer sees any access outside them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "../pysignalduino_amd/csrc/sdx_strtod.h"

static int hexv(char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    const size_t n = line.size() / 2;
    uint8_t* s = static_cast<uint8_t*>(std::malloc(n ? n : 1));
    uint8_t* scratch = static_cast<uint8_t*>(std::malloc(sdxf::kScratch));
    if (!s || !scratch) return 2;
    for (size_t k = 0; k < n; ++k) s[k] = static_cast<uint8_t>(16 * hexv(line[2 * k]) + hexv(line[2 * k + 1]));
    std::memset(scratch, 0xEE, sdxf::kScratch);  // no digit: stale scratch must never be read as one
    uint64_t bits = 0;
    const int cls = sdxf::py_float(s, static_cast<int>(n), scratch, &bits);
    std::printf("%d %016llx\n", cls, cls == 1 ? static_cast<unsigned long long>(bits) : 0ull);
    std::free(scratch);
    std::free(s);
  }
  return 0;
}
