// profile_blob_check.cpp -- the receiver-profile table's blob validator
// (pysignalduino_amd/csrc/sdx_profile_layout.h) under the address and UB sanitizers, stand-alone:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/profile_blob_check.cpp -o profile_blob_check && ./profile_blob_check table.blob
//
// table.blob: a blob pysignalduino_amd.profiles.ReceiverProfiles wrote.  Every candidate is copied into a
// heap block of exactly its size, so a validator that read past nbytes trips the sanitizer.  The good blob
// must pass (at an odd address too); every damaged one must be refused: truncated at every section boundary
// (with the header's total_bytes left alone and with it patched to the cut), a mask bit at or above its
// kind's class count, an of_source entry = the profile count, wrong magic / version / counts, the class
// counts of another bank where a set bit then lies beyond them, non-zero padding.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../pysignalduino_amd/csrc/sdx_profile_layout.h"

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                      \
    }                                                                \
  } while (0)

// validate a copy of v that owns exactly v.size() bytes
static const char* verdict(const std::vector<uint8_t>& v) {
  uint8_t* p = static_cast<uint8_t*>(std::malloc(v.size() ? v.size() : 1));
  if (!p) std::abort();
  if (!v.empty()) std::memcpy(p, v.data(), v.size());
  const char* why = sdx_profile_validate(p, v.size());
  std::free(p);
  return why;
}
static void put32(std::vector<uint8_t>& v, size_t off, uint32_t x) { std::memcpy(v.data() + off, &x, 4); }

int main(int argc, char** argv) {
  static_assert(sizeof(sdx_profile_hdr) == 48, "the header's size");
  CHECK(argc == 2);
  std::FILE* fh = std::fopen(argv[1], "rb");
  CHECK(fh != nullptr);
  std::vector<uint8_t> good;
  uint8_t buf[4096];
  for (size_t k; (k = std::fread(buf, 1, sizeof buf, fh)) > 0;) good.insert(good.end(), buf, buf + k);
  std::fclose(fh);
  const size_t n = good.size();
  const char* why = verdict(good);
  if (why) std::fprintf(stderr, "the good blob: %s\n", why);
  CHECK(why == nullptr);
  {  // at an odd address: no aligned access is assumed
    uint8_t* p = static_cast<uint8_t*>(std::malloc(n + 1));
    CHECK(p != nullptr);
    std::memcpy(p + 1, good.data(), n);
    CHECK(sdx_profile_validate(p + 1, n) == nullptr);
    std::free(p);
  }
  CHECK(sdx_profile_validate(nullptr, 0) != nullptr);
  sdx_profile_hdr h;
  std::memcpy(&h, good.data(), sizeof h);
  const size_t total_at = offsetof(sdx_profile_hdr, total_bytes), np_at = offsetof(sdx_profile_hdr, n_profiles),
               ns_at = offsetof(sdx_profile_hdr, n_sources), nc_at = offsetof(sdx_profile_hdr, n_class);
  const size_t so = sdx_profile_src_off(h.n_profiles);

  // ---- truncation at every section boundary (and a byte / a word to either side) ----------------------
  int refused = 0;
  for (size_t c : {(size_t)0, (size_t)1, (size_t)16, (size_t)47, (size_t)48, (size_t)49, (size_t)56, (size_t)48 + 127,
                   (size_t)48 + 128, so - 8, so - 1, so, so + 1, so + h.n_sources - 1, so + h.n_sources, n - 16, n - 1}) {
    if (c >= n) continue;
    std::vector<uint8_t> v(good.begin(), good.begin() + c);
    CHECK(verdict(v) != nullptr);  // total_bytes names the old size
    if (c >= sizeof(sdx_profile_hdr)) {
      put32(v, total_at, (uint32_t)c);  // the header agrees with the cut: the counts decide
      CHECK(verdict(v) != nullptr);
    }
    ++refused;
  }
  CHECK(refused > 8);
  {  // longer than its counts say
    std::vector<uint8_t> v = good;
    v.resize(n + 16, 0);
    CHECK(verdict(v) != nullptr);
    put32(v, total_at, (uint32_t)n + 16);
    CHECK(verdict(v) != nullptr);
  }

  // ---- contents out of range --------------------------------------------------------------------------
  auto damaged = [&](size_t off, uint32_t x, int bytes) {
    std::vector<uint8_t> v = good;
    std::memcpy(v.data() + off, &x, bytes);
    return verdict(v);
  };
  CHECK(damaged(0, SDX_PROFILE_MAGIC ^ 1u, 4) != nullptr);
  CHECK(damaged(4, SDX_PROFILE_VERSION + 1, 4) != nullptr);
  CHECK(damaged(total_at, (uint32_t)n + 16, 4) != nullptr);
  CHECK(damaged(np_at, 0, 4) != nullptr && damaged(np_at, SDX_PROFILE_MAX + 1, 4) != nullptr);
  CHECK(damaged(np_at, h.n_profiles + 1, 4) != nullptr && damaged(np_at, 0xFFFFFFFFu, 4) != nullptr);
  CHECK(damaged(ns_at, 0, 4) != nullptr && damaged(ns_at, SDX_PROFILE_SOURCES_MAX + 1, 4) != nullptr);
  CHECK(damaged(ns_at, h.n_sources + 16, 4) != nullptr && damaged(ns_at, 0xFFFFFFFFu, 4) != nullptr);
  CHECK(damaged(offsetof(sdx_profile_hdr, res), 1, 4) != nullptr);
  int bits = 0;
  for (int kd = 0; kd < 4; ++kd) {
    CHECK(damaged(nc_at + 4 * kd, SDX_PROFILE_CLASS_MAX + 1, 4) != nullptr);  // a class count above 256
    for (uint32_t p : {0u, h.n_profiles - 1}) {
      const size_t m = SDX_PROFILE_MASK_OFF + (size_t)SDX_PROFILE_MASK_BYTES * p + 32u * kd;
      const uint32_t c = h.n_class[kd];
      if (c < 256) {  // the first bit beyond the class count, and the mask's last bit
        std::vector<uint8_t> v = good;
        v[m + c / 8] |= (uint8_t)(1u << (c % 8));
        CHECK(verdict(v) != nullptr);
        v = good;
        v[m + 31] |= 0x80;
        CHECK(verdict(v) != nullptr);
        bits += 2;
      }
      if (c > 0) {  // the last legal bit is legal
        std::vector<uint8_t> v = good;
        v[m + (c - 1) / 8] |= (uint8_t)(1u << ((c - 1) % 8));
        CHECK(verdict(v) == nullptr);
        // ... and is refused by the class count of a smaller bank
        put32(v, nc_at + 4 * kd, c - 1);
        CHECK(verdict(v) != nullptr);
      }
    }
  }
  CHECK(damaged(so, h.n_profiles, 1) != nullptr);                    // of_source[0], of_source[S - 1]
  CHECK(damaged(so + h.n_sources - 1, 255, 1) != nullptr);
  if (so + h.n_sources < n) CHECK(damaged(n - 1, 1, 1) != nullptr);  // padding
  std::printf("profile_blob_check: ok (%u profiles, %u sources, %d truncations and %d mask bits refused)\n", h.n_profiles,
              h.n_sources, refused, bits);
  return 0;
}
