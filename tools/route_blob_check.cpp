// route_blob_check.cpp -- the route table's blob validator (pysignalduino_amd/csrc/sdx_route_layout.h)
// under the address and UB sanitizers, stand-alone:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/route_blob_check.cpp -o route_blob_check && ./route_blob_check table.blob
//
// table.blob: a blob pysignalduino_amd.routes.RouteTable wrote.  Every candidate is copied into a heap
// block of exactly its size, so a validator that read past nbytes trips the sanitizer.  The good blob
// must pass (at an odd address too); every damaged one must be refused: truncated at every section
// boundary (with the header's total_bytes left alone and with it patched to the cut), an out-of-range
// transition, class and start state, table offsets outside the blob, wrong magic / version / counts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../pysignalduino_amd/csrc/sdx_route_layout.h"

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
  const char* why = sdx_route_validate(p, v.size());
  std::free(p);
  return why;
}
static void put32(std::vector<uint8_t>& v, size_t off, uint32_t x) { std::memcpy(v.data() + off, &x, 4); }

int main(int argc, char** argv) {
  static_assert(sizeof(sdx_route_hdr) == 32 && sizeof(sdx_route_dfa) == 16, "the records' sizes");
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
    CHECK(sdx_route_validate(p + 1, n) == nullptr);
    std::free(p);
  }
  sdx_route_hdr h;
  std::memcpy(&h, good.data(), sizeof h);
  std::vector<sdx_route_dfa> d(h.n_routes);
  std::memcpy(d.data(), good.data() + SDX_ROUTE_DFA_OFF, sizeof(sdx_route_dfa) * h.n_routes);
  const size_t total_at = offsetof(sdx_route_hdr, total_bytes);

  // ---- truncation at every section boundary (and one byte / one word to either side) ----------------
  std::vector<size_t> cuts = {0, 1, 16, 31, 32, 33, SDX_ROUTE_DFA_OFF - 1, SDX_ROUTE_DFA_OFF, SDX_ROUTE_DFA_OFF + 16,
                              sdx_route_tables_off(h.n_routes) - 4, sdx_route_tables_off(h.n_routes), n - 4, n - 1};
  for (const sdx_route_dfa& r : d) {
    const size_t tend = (size_t)r.trans_off + (size_t)r.n_states * h.n_class * h.trans_width;
    for (size_t c : {(size_t)r.flags_off, (size_t)r.flags_off + r.n_states - 1, (size_t)r.flags_off + r.n_states,
                     (size_t)r.trans_off, (size_t)r.trans_off + 4, tend - 4, tend - 1})
      cuts.push_back(c);
  }
  int refused = 0;
  for (size_t c : cuts) {
    if (c >= n) continue;
    std::vector<uint8_t> v(good.begin(), good.begin() + c);
    CHECK(verdict(v) != nullptr);  // total_bytes names the old size
    if (c >= sizeof(sdx_route_hdr)) {
      put32(v, total_at, (uint32_t)c);  // the header agrees with the cut: the sections' own checks decide
      CHECK(verdict(v) != nullptr);
    }
    ++refused;
  }
  CHECK(refused > 10);

  // ---- contents out of range --------------------------------------------------------------------------
  auto damaged = [&](size_t off, uint32_t x, int bytes) {
    std::vector<uint8_t> v = good;
    std::memcpy(v.data() + off, &x, bytes);
    return verdict(v);
  };
  CHECK(damaged(0, SDX_ROUTE_MAGIC ^ 1u, 4) != nullptr);                      // magic
  CHECK(damaged(4, SDX_ROUTE_VERSION + 1, 4) != nullptr);                     // version
  CHECK(damaged(8, 0, 4) != nullptr && damaged(8, SDX_ROUTE_MAX + 1, 4) != nullptr);   // route count
  CHECK(damaged(12, 0, 4) != nullptr && damaged(12, 257, 4) != nullptr);      // class count
  CHECK(damaged(16, 3, 4) != nullptr && damaged(16, 0, 4) != nullptr);        // width
  CHECK(damaged(total_at, (uint32_t)n + 4, 4) != nullptr);
  if (h.n_class < 256) {
    CHECK(damaged(SDX_ROUTE_CLS_OFF, h.n_class, 1) != nullptr);               // cls_of[0], cls_of[255]
    CHECK(damaged(SDX_ROUTE_CLS_OFF + 255, 255, 1) != nullptr);
  }
  for (uint32_t r = 0; r < h.n_routes; ++r) {
    const size_t rec = SDX_ROUTE_DFA_OFF + sizeof(sdx_route_dfa) * r;
    const size_t cells = (size_t)d[r].n_states * h.n_class;
    CHECK(damaged(rec + 4, d[r].n_states, 4) != nullptr);                     // start state
    CHECK(damaged(rec, 0, 4) != nullptr && damaged(rec, SDX_ROUTE_STATES_MAX + 1, 4) != nullptr);
    CHECK(damaged(rec + 8, (uint32_t)n, 4) != nullptr);                       // flags table at the blob's end
    CHECK(damaged(rec + 8, d[r].flags_off + 2, 4) != nullptr);                // misaligned
    CHECK(damaged(rec + 12, (uint32_t)n - 4, 4) != nullptr || cells * h.trans_width <= 4);
    CHECK(damaged(rec + 12, 0xFFFFFFFCu, 4) != nullptr);                      // no wrap-around
    CHECK(damaged(rec + 12, 0, 4) != nullptr);                                // inside the header
    if (h.trans_width == 1 && d[r].n_states < 256) {                          // first and last transition
      CHECK(damaged(d[r].trans_off, d[r].n_states, 1) != nullptr);
      CHECK(damaged(d[r].trans_off + cells - 1, 255, 1) != nullptr);
    } else if (h.trans_width == 2) {
      CHECK(damaged(d[r].trans_off, d[r].n_states, 2) != nullptr);
      CHECK(damaged(d[r].trans_off + 2 * (cells - 1), 0xFFFF, 2) != nullptr);
    }
    CHECK(damaged(d[r].flags_off, 8, 1) != nullptr);                          // an unknown flag
  }

  // ---- the LDS split: whole routes, whole words, inside the budget and the blob -----------------------
  for (uint32_t budget : {1312u, 2048u, 4096u, SDX_ROUTE_LDS_BYTES, 1u << 20}) {
    uint32_t bytes = 0;
    const uint32_t k = sdx_route_lds_routes(good.data(), budget, &bytes);
    CHECK(k <= h.n_routes && bytes % 4 == 0 && bytes <= budget && bytes + sizeof(sdx_route_hdr) <= n);
    CHECK(bytes + sizeof(sdx_route_hdr) >= sdx_route_tables_off(h.n_routes));
    for (uint32_t r = 0; r < k; ++r)
      CHECK((size_t)d[r].trans_off + (size_t)d[r].n_states * h.n_class * h.trans_width <= bytes + sizeof(sdx_route_hdr));
    if (budget == 1u << 20) CHECK(k == h.n_routes);
  }
  std::printf("route_blob_check: ok (%u routes, %d truncations refused)\n", h.n_routes, refused);
  return 0;
}
