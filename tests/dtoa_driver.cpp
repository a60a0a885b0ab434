// Host driver of pysignalduino_amd/csrc/sdx_dtoa.h for tests/test_dtoa_host.py: one binary64 bit
// pattern (16 hex digits) per input line; prints "<repr> <json>" per line.  Each text is written into
// an exact-size 24-byte heap block, so AddressSanitizer sees any byte past the promised length.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "../pysignalduino_amd/csrc/sdx_dtoa.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    const uint64_t bits = std::strtoull(line.c_str(), nullptr, 16);
    double x;
    std::memcpy(&x, &bits, 8);
    for (int form = 0; form < 2; ++form) {
      uint8_t* out = static_cast<uint8_t*>(std::malloc(24));
      if (!out) return 2;
      const int n = sdxf::py_repr(x, form != 0, out);
      if (n < 1 || n > 24) return 3;
      std::fwrite(out, 1, static_cast<size_t>(n), stdout);
      std::fputc(form ? '\n' : ' ', stdout);
      std::free(out);
    }
  }
  return 0;
}
