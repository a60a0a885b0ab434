// sdx_profile.hip -- receiver profiles (sdx_filter_records), hand-written HIP for gfx950.
//
// A stream merges up to 4,096 receivers; every line carries its source id.  A PROFILE is a set of enabled
// protocol classes per kind, a PROFILE TABLE maps every source id to one of up to 64 profiles (the blob:
// sdx_profile_layout.h, compiled by pysignalduino_amd/profiles.py).  The pass rewrites each kind's launch
// output -- descriptors, records, cursor -- so that every line keeps only the records whose class its
// source's profile enables, in list order, compacted into a dense record array in LINE order
// (DESIGN.md §4n).  Payloads stay where they are: a kept record is copied with all its 16 bytes.
//
// The skeleton -- count -> scan -> write, the scan, the slots, the common argument checks -- is sdx_compact.h;
// this file is the pass's policy, the table's functions and the entries.
// Table contents are never range-checked here: sdx_profile_validate passed the whole blob before it was
// uploaded.  What is checked are the values that come from the launch: proto and the source id.
#include <cstring>

#include "sdx_compact.h"
#include "sdx_profile_layout.h"

struct sdx_profile_table {
  int device;
  uint8_t* dev;  // the blob
  sdx_profile_hdr hdr;
};

namespace sdxp {

using namespace sdxc;
static_assert(SDX_PROFILE_TILE == T, "the layout header's tile is the skeleton's");
constexpr uint32_t HDR = sizeof(sdx_profile_hdr);

struct Policy {
  struct Args {
    const uint8_t* blob;
    uint32_t P, S;
    const int32_t* source;
  };

  // The table's part one kind's block needs, in LDS: masks[p] = the kind's four words of profile p, then
  // of_source.  8 B-aligned words first, bytes behind them.
  struct Staged {
    uint64_t mask[SDX_PROFILE_MAX][4];
    uint8_t of_source[SDX_PROFILE_SOURCES_MAX];
  };
  static __device__ __forceinline__ void stage(Staged& L, const Args& a, const Slot& k) {
    const uint64_t* m = reinterpret_cast<const uint64_t*>(a.blob + HDR);  // the blob is 16-byte aligned, HDR = 48
    for (uint32_t i = threadIdx.x; i < 4 * a.P; i += T) L.mask[i >> 2][i & 3] = m[(i >> 2) * 16 + k.kind * 4 + (i & 3)];
    const uint32_t* s = reinterpret_cast<const uint32_t*>(a.blob + HDR + SDX_PROFILE_MASK_BYTES * a.P);  // padded to 16 bytes
    uint32_t* d = reinterpret_cast<uint32_t*>(L.of_source);
    for (uint32_t i = threadIdx.x; i < (a.S + 3) / 4; i += T) d[i] = s[i];
    __syncthreads();
  }

  // One lane's line: its profile index; a source id outside [0, S) keeps nothing (-1).
  struct Line {
    const Staged& L;
    int p;
    uint32_t n_class;
    __device__ __forceinline__ Line(const Staged& L_, const Args& a, const Slot& k, int g) : L(L_), n_class(k.n_class) {
      const int32_t src = a.source ? a.source[g] : 0;
      p = src >= 0 && (uint32_t)src < a.S ? (int)L.of_source[src] : -1;
    }
    // One 8-byte LDS read per record: the mask word of its class.  (The line's four words held in registers and
    // picked by a chain of selects were compiled into a private array indexed by proto >> 6: 48 bytes of scratch
    // memory a lane.)
    __device__ __forceinline__ bool keep(const uint4& v) const {
      const uint32_t proto = v.y >> 16;                                 // the high half of word 1
      const uint64_t word = L.mask[p < 0 ? 0 : p][(proto >> 6) & 3];    // always inside the staged masks
      return p >= 0 && proto < n_class && ((word >> (proto & 63)) & 1);  // n_class <= 256
    }
  };
};

}  // namespace sdxp

extern "C" int sdx_profile_table_create(const void* blob, size_t nbytes, int device, sdx_profile_table** out) {
  using namespace sdxp;
  static const char FN[] = "sdx_profile_table_create";
  if (!blob || !out) return bad_arg(FN, "null argument");
  const uint8_t* b = static_cast<const uint8_t*>(blob);
  if (const char* why = sdx_profile_validate(b, nbytes)) return bad_arg(FN, why);  // nothing is uploaded
  sdx_profile_hdr h;
  memcpy(&h, b, sizeof h);
  hipError_t e = hipSetDevice(device);
  void* d = nullptr;
  if (e == hipSuccess) e = hipMalloc(&d, nbytes);
  if (e == hipSuccess) e = hipMemcpy(d, blob, nbytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (d) (void)hipFree(d);
    return sdx::set_error(SDX_EHIP, std::string(FN) + ": " + hipGetErrorString(e));
  }
  *out = new sdx_profile_table{device, static_cast<uint8_t*>(d), h};
  return SDX_OK;
}

extern "C" const char* sdx_profile_check(const void* blob, size_t nbytes) {
  return sdx_profile_validate(static_cast<const uint8_t*>(blob), nbytes);
}

extern "C" int sdx_profile_table_destroy(sdx_profile_table* table) {
  if (!table) return SDX_OK;
  if (table->dev) (void)hipFree(table->dev);
  delete table;
  return SDX_OK;
}

extern "C" size_t sdx_profile_scratch_bytes(int k, int32_t n) { return sdxc::scratch_bytes(k, n); }

extern "C" int sdx_filter_records(const sdx_bank* bank, const sdx_profile_table* table, const sdx_json_in* kinds, int k,
                                  int32_t n, const int32_t* source_dev, sdx_desc* const* desc_out,
                                  sdx_result* const* rec_out, const uint32_t* rec_cap, uint32_t* const* cursor_out,
                                  void* scratch_dev, void* hip_stream) {
  using namespace sdxp;
  static const char FN[] = "sdx_filter_records";
  if (!bank) return bad_arg(FN, "null bank");
  if (!table || !table->dev) return bad_arg(FN, "null table");
  const sdx_bank_hdr* bh = sdx::bank_hdr(bank);
  const uint32_t counts[4] = {bh->n_mu, bh->n_ms, bh->n_mc, bh->n_mn};
  const char* why = nullptr;
  for (int kd = 0; kd < 4; ++kd)
    if (table->hdr.n_class[kd] != counts[kd]) why = "the table was compiled for another bank";
  Slots in{};
  if (const int rc = fill_slots(FN, counts, why, kinds, k, n, source_dev, false, desc_out, rec_out, rec_cap, cursor_out,
                                scratch_dev, &in))
    return rc;
  return launch<Policy>(FN, in, k, n, {table->dev, table->hdr.n_profiles, table->hdr.n_sources, source_dev}, hip_stream);
}
