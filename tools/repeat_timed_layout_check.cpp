// repeat_timed_layout_check.cpp -- the host-side size / offset helpers of sdx_mark_repeats_timed
// (pysignalduino_amd/csrc/sdx_repeat_layout.h) under the address and UB sanitizers, stand-alone:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/repeat_timed_layout_check.cpp -o repeat_timed_layout_check && ./repeat_timed_layout_check
//
// For a range of n it allocates exactly sdx_repeat_timed_scratch_size(n) / sdx_repeat_timed_state_size()
// bytes on the heap and writes every section through the offsets the library uses, first to last byte,
// with the element type the kernels use: a section that overlapped another, was misaligned for its type,
// or reached past the size handed to the caller trips the sanitizer or a check.
#include <cstddef>
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

template <class T>
static int bump(unsigned char* s, size_t off, size_t count) {
  CHECK(off % alignof(T) == 0);
  T* p = reinterpret_cast<T*>(s + off);
  for (size_t i = 0; i < count; ++i) p[i] += 1;
  return 0;
}

static int check_n(int64_t n) {
  const size_t size = sdx_repeat_timed_scratch_size(n);
  const size_t lines = sdx_rt_lines(n);
  const size_t nt = (size_t)sdx_repeat_tiles(n);
  CHECK(size % 16 == 0 && size >= 16);
  CHECK(sdx_rt_keys_off() == 16 && sdx_rt_te_off(n) % 8 == 0);
  CHECK(sdx_rt_flags_off(n) + lines <= size);
  unsigned char* s = static_cast<unsigned char*>(std::malloc(size));
  CHECK(s != nullptr);
  std::memset(s, 0, size);
  if (bump<int32_t>(s, 0, 4)) return 1;
  sdx_repeat_key* keys = reinterpret_cast<sdx_repeat_key*>(s + sdx_rt_keys_off());
  for (size_t i = 0; i < lines; ++i) keys[i].kind += 1, keys[i].proto += 1, keys[i].len += 1, keys[i].off += 1;
  if (bump<int64_t>(s, sdx_rt_te_off(n), lines)) return 1;
  if (bump<int32_t>(s, sdx_rt_seg_off(n), lines)) return 1;
  if (bump<int32_t>(s, sdx_rt_succ_off(n), lines)) return 1;
  if (bump<int32_t>(s, sdx_rt_exit_off(n), lines)) return 1;
  if (bump<int32_t>(s, sdx_rt_last_off(n), lines)) return 1;
  for (int t = 0; t < 5; ++t)
    if (bump<int32_t>(s, sdx_rt_tile_off(n, t), nt)) return 1;
  if (bump<uint8_t>(s, sdx_rt_flags_off(n), lines)) return 1;
  // every byte of every section was written exactly once: no section overlaps another
  size_t ones = 0;
  for (size_t i = 0; i < size; ++i) {
    CHECK(s[i] <= 1);
    ones += s[i];
  }
  CHECK(ones == 4 + 4 * lines + lines + 4 * lines + 5 * nt + lines);
  CHECK(sdx_rt_flags_off(n) + lines + 15 >= size);   // nothing but the rounding behind the last section
  std::free(s);
  return 0;
}

int main() {
  static_assert(sizeof(sdx_repeat_timed_state_hdr) == 24, "header + T");
  static_assert(offsetof(sdx_repeat_timed_state_hdr, t) == 16, "T behind the untimed header's fields");
  const size_t st = sdx_repeat_timed_state_size();
  CHECK(st % 16 == 0 && st >= sizeof(sdx_repeat_timed_state_hdr) + SDX_REPEAT_PAYLOAD_MAX);
  CHECK(sdx_repeat_state_size() == 16 + 65536);       // the untimed layout is what it was
  unsigned char* state = static_cast<unsigned char*>(std::malloc(st));
  CHECK(state != nullptr);
  std::memset(state, 0, sizeof(sdx_repeat_timed_state_hdr));
  reinterpret_cast<sdx_repeat_timed_state_hdr*>(state)->t = INT64_MIN;
  std::memset(state + sizeof(sdx_repeat_timed_state_hdr), 0xAB, SDX_REPEAT_PAYLOAD_MAX);   // the longest payload fits
  std::free(state);
  const int64_t T = SDX_REPEAT_TILE;
  const int64_t ns[] = {-5, 0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T, 2 * T + 1, 1000, 250000, 1000003, (1 << 22) + 7};
  for (int64_t n : ns)
    if (check_n(n)) return 1;
  CHECK(sdx_repeat_timed_scratch_size(INT32_MAX) > 41ull * INT32_MAX);   // no 32-bit wrap at the ABI's largest n
  std::puts("repeat_timed_layout_check: ok");
  return 0;
}
