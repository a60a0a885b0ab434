// repeat_sources_layout_check.cpp -- the host-side size / offset helpers of sdx_mark_repeats_by_source
// (pysignalduino_amd/csrc/sdx_repeat_layout.h) under the address and UB sanitizers, stand-alone:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/repeat_sources_layout_check.cpp -o repeat_sources_layout_check && ./repeat_sources_layout_check
//
// For a range of (n, S) it allocates exactly sdx_repeat_sources_scratch_size(n, S) bytes on the heap and
// writes every part through the offsets the library uses, first to last byte, with the element type the
// kernels use: a part that overlapped another, was misaligned for its type, or reached past the size
// handed to the caller trips the sanitizer or a check.  The state's slots are written the same way.
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
static int bump(unsigned char* s, size_t off, size_t bytes) {
  CHECK(off % alignof(T) == 0 && off % 16 == 0 && bytes % sizeof(T) == 0);
  T* p = reinterpret_cast<T*>(s + off);
  const T zero{};
  for (size_t i = 0; i < bytes / sizeof(T); ++i) {
    CHECK(std::memcmp(&p[i], &zero, sizeof(T)) == 0);   // not written by an earlier part
    T one;
    std::memset(&one, 1, sizeof(T));
    p[i] = one;                                         // through the element type
  }
  return 0;
}

static int check(int64_t n, int64_t S) {
  const size_t size = sdx_repeat_sources_scratch_size(n, S);
  CHECK(size % 16 == 0 && size >= 16);
  CHECK(sdx_rs_off(n, S, SDX_RS_HEAD) == 0 && sdx_rs_off(n, S, SDX_RS_TABLE) == 16);   // the table: independent of n
  unsigned char* s = static_cast<unsigned char*>(std::malloc(size));
  CHECK(s != nullptr);
  std::memset(s, 0, size);
  size_t sum = 0;
  for (int p = 0; p < SDX_RS_END; ++p) {
    const size_t off = sdx_rs_off(n, S, p), bytes = sdx_rs_part_bytes(n, S, p);
    CHECK(off + bytes <= size);
    sum += bytes;
    int r;
    switch (p) {
      case SDX_RS_TABLE: r = bump<sdx_repeat_source_entry>(s, off, bytes); break;
      case SDX_RS_LKEYS: case SDX_RS_KEYS: r = bump<sdx_repeat_key>(s, off, bytes); break;
      case SDX_RS_TE: case SDX_RS_PTIMES: r = bump<int64_t>(s, off, bytes); break;
      case SDX_RS_FLAGS: r = bump<uint8_t>(s, off, bytes); break;
      default: r = bump<int32_t>(s, off, bytes);
    }
    if (r) return 1;
  }
  size_t ones = 0;
  for (size_t i = 0; i < size; ++i) ones += s[i] == 1;
  CHECK(ones == sum);                                         // no part overlaps another
  CHECK(size - sum < 16 * (size_t)SDX_RS_END);                // nothing but the roundings between them
  CHECK(sdx_rs_off(n, S, SDX_RS_END) == size);
  std::free(s);
  return 0;
}

int main() {
  static_assert(sizeof(sdx_repeat_source_entry) == 32, "the compact table's entry");
  static_assert(offsetof(sdx_repeat_source_entry, t) == 16 && offsetof(sdx_repeat_source_entry, last) == 24, "entry");
  static_assert(offsetof(sdx_repeat_source_entry, len) == offsetof(sdx_repeat_timed_state_hdr, len), "entry = header + last");
  const size_t slot = sdx_repeat_timed_state_size();
  CHECK(slot % 16 == 0);
  CHECK(sdx_repeat_sources_state_size(0) == 0 && sdx_repeat_sources_state_size(SDX_REPEAT_SOURCES_MAX + 1) == 0);
  CHECK(sdx_repeat_sources_state_size(-3) == 0 && sdx_repeat_sources_scratch_size(100, 0) == 0);
  CHECK(sdx_repeat_sources_scratch_size(100, SDX_REPEAT_SOURCES_MAX + 1) == 0);
  CHECK(sdx_repeat_sources_state_size(1) == slot);            // S = 1: the timed entry's state buffer
  CHECK(sdx_repeat_sources_state_size(SDX_REPEAT_SOURCES_MAX) == (size_t)SDX_REPEAT_SOURCES_MAX * slot);
  CHECK(sdx_rs_passes(1) == 1 && sdx_rs_passes(256) == 1 && sdx_rs_passes(257) == 2 && sdx_rs_passes(4096) == 2);
  {   // every slot: header and the longest payload, the last slot's last byte is the buffer's
    const int64_t S = 5;
    const size_t st = sdx_repeat_sources_state_size(S);
    unsigned char* state = static_cast<unsigned char*>(std::malloc(st));
    CHECK(state != nullptr);
    for (int64_t i = 0; i < S; ++i) {
      unsigned char* sl = state + (size_t)i * slot;
      std::memset(sl, 0, sizeof(sdx_repeat_timed_state_hdr));
      reinterpret_cast<sdx_repeat_timed_state_hdr*>(sl)->t = INT64_MIN;
      std::memset(sl + sizeof(sdx_repeat_timed_state_hdr), 0xAB, SDX_REPEAT_PAYLOAD_MAX);
    }
    std::free(state);
  }
  const int64_t T = SDX_REPEAT_TILE;
  const int64_t ns[] = {-5, 0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 1000, 250000, (1 << 22) + 7};
  const int64_t ss[] = {1, 2, 3, 255, 256, 257, 4096};
  for (int64_t n : ns)
    for (int64_t S : ss)
      if (check(n, S)) return 1;
  CHECK(sdx_repeat_sources_scratch_size(INT32_MAX, 4096) > 80ull * INT32_MAX);   // no 32-bit wrap at the ABI's largest n
  std::puts("repeat_sources_layout_check: ok");
  return 0;
}
