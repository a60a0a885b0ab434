// repeat_layout_check.cpp -- the host-side size / offset helpers of sdx_mark_repeats
// (pysignalduino_amd/csrc/sdx_repeat_layout.h) under the address and UB sanitizers, stand-alone:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/repeat_layout_check.cpp -o repeat_layout_check && ./repeat_layout_check
//
// For a range of n it allocates exactly sdx_repeat_scratch_size(n) / sdx_repeat_state_size() bytes on
// the heap and writes every section through the offsets the library uses, first to last byte: a section
// that overlapped another, or reached past the size handed to the caller, trips the sanitizer or a check.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../pysignalduino_amd/csrc/sdx_repeat_layout.h"

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                      \
    }                                                                \
  } while (0)

static int check_n(int64_t n) {
  const size_t size = sdx_repeat_scratch_size(n);
  const int64_t nt = sdx_repeat_tiles(n);
  CHECK(size % 16 == 0 && size >= 16);
  CHECK(nt * SDX_REPEAT_TILE >= n && (nt == 0 || (nt - 1) * SDX_REPEAT_TILE < n));
  CHECK(sdx_repeat_keys_off() == 16 && sdx_repeat_keys_off() % 16 == 0);
  CHECK(sdx_repeat_tile_last_off(n) % 4 == 0 && sdx_repeat_tile_prev_off(n) % 4 == 0);
  CHECK(sdx_repeat_tile_prev_off(n) + 4 * (size_t)nt <= size);
  unsigned char* s = static_cast<unsigned char*>(std::malloc(size));
  CHECK(s != nullptr);
  std::memset(s, 0, size);
  int32_t* head = reinterpret_cast<int32_t*>(s);
  for (int i = 0; i < 4; ++i) head[i] += 1;
  sdx_repeat_key* keys = reinterpret_cast<sdx_repeat_key*>(s + sdx_repeat_keys_off());
  for (int64_t i = 0; i < (n > 0 ? n : 0); ++i) keys[i].kind += 1, keys[i].proto += 1, keys[i].len += 1, keys[i].off += 1;
  int32_t* last = reinterpret_cast<int32_t*>(s + sdx_repeat_tile_last_off(n));
  int32_t* prev = reinterpret_cast<int32_t*>(s + sdx_repeat_tile_prev_off(n));
  for (int64_t b = 0; b < nt; ++b) last[b] += 1;
  for (int64_t b = 0; b < nt; ++b) prev[b] += 1;
  // every byte of every section was written exactly once: no section overlaps another
  const size_t used = sdx_repeat_tile_prev_off(n) + 4 * (size_t)nt;
  for (size_t i = 0; i < used; ++i) CHECK(s[i] == (i % 4 == 0 ? 1 : 0));
  std::free(s);
  return 0;
}

int main() {
  static_assert(sizeof(sdx_repeat_key) == 16 && sizeof(sdx_repeat_state_hdr) == 16, "16-byte records");
  const size_t st = sdx_repeat_state_size();
  CHECK(st % 16 == 0 && st >= sizeof(sdx_repeat_state_hdr) + SDX_REPEAT_PAYLOAD_MAX);
  unsigned char* state = static_cast<unsigned char*>(std::malloc(st));
  CHECK(state != nullptr);
  std::memset(state, 0, sizeof(sdx_repeat_state_hdr));
  std::memset(state + sizeof(sdx_repeat_state_hdr), 0xAB, SDX_REPEAT_PAYLOAD_MAX);   // the longest payload fits
  std::free(state);
  const int64_t T = SDX_REPEAT_TILE;
  const int64_t ns[] = {-5, 0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T, 2 * T + 1, 1000, 250000, 1000003, (1 << 22) + 7};
  for (int64_t n : ns)
    if (check_n(n)) return 1;
  CHECK(sdx_repeat_scratch_size(INT32_MAX) > 16ull * INT32_MAX);   // no 32-bit wrap at the ABI's largest n
  std::puts("repeat_layout_check: ok");
  return 0;
}
