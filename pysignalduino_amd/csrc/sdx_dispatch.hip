// sdx_dispatch.hip -- dispatch rules (sdx_dispatch_records), hand-written HIP for gfx950.
//
// FHEM dispatches every message a line demodulates to, but stops after maxMuMsgRepeat messages of one protocol
// and drops a message equal to the one just dispatched, unless its protocol carries dispatchequals.  The pass
// rewrites each kind's launch output -- descriptors, records, cursor -- so that every line keeps only the
// records those two rules keep (the definition: include/sdx.h), in list order, compacted into a
// dense record array in LINE order, exactly as sdx_filter_records leaves its outputs: every
// consumer of a launch's outputs runs on them unchanged.  Payloads stay where they are.
//
// The skeleton -- count -> scan -> write, the scan, the slots, the common argument checks -- is sdx_compact.h;
// this file is the pass's policy and the entries.  Both kernels make the decisions: no flag per input record is stored.
// The rules are never range-checked here: sdx_dispatch_validate passed them before anything was launched.  What
// is checked is the value that comes from the launch: proto.
#include "sdx_compact.h"
#include "sdx_dispatch_layout.h"

namespace sdxd {

using namespace sdxc;
static_assert(SDX_DISPATCH_TILE == T, "the layout header's tile is the skeleton's");
constexpr uint32_t NONE = 0xFFFFFFFFu;  // no protocol: sdx_result.proto has 16 bits

// Byte by byte, as sdx_repeat.hip's same_bytes: the heap has no slack behind its last payload, and payloads
// stand at any alignment.  Nothing outside [a, a + len) and [b, b + len) is read.
__device__ __forceinline__ bool same_bytes(const uint8_t* a, const uint8_t* b, uint32_t len) {
  if (a == b) return true;  // two records of one payload
  for (uint32_t i = 0; i < len; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

struct Policy {
  using Args = sdx_dispatch_rules;

  // The kind's four mask words go through LDS: a lane picks its word by proto >> 6, and a per-lane index into
  // values held in registers would become a private array.
  struct Staged {
    uint64_t mask[4];
  };
  static __device__ __forceinline__ void stage(Staged& L, const Args& rules, const Slot& k) {
    if (threadIdx.x < 4) L.mask[threadIdx.x] = rules.keep_equal[k.kind][threadIdx.x];
    __syncthreads();
  }

  // One lane's state along its line's records -- run, prev_proto and the last dispatched record's {off, len,
  // proto}, all in registers -- beside the kind's part of the rules, out of the kernel arguments.
  struct Line {
    const Staged& L;
    const uint8_t* heap;
    uint32_t cap, drop_equal, n_class;
    uint32_t run = 0, prev_proto = NONE;
    uint32_t l_off = 0, l_len = 0, l_proto = NONE;  // the last record that passed the cap ("last")
    __device__ __forceinline__ Line(const Staged& L_, const Args& rules, const Slot& k, int)
        : L(L_), heap(k.heap), cap((uint32_t)rules.max_repeat[k.kind]), drop_equal((uint32_t)rules.drop_equal),
          n_class(k.n_class) {}

    // the definition's loop body for the record {off, len | proto << 16, ..}: is it kept?
    __device__ __forceinline__ bool keep(const uint4& v) {
      const uint32_t off = v.x, proto = v.y >> 16, len = v.y & 0xFFFFu;
      run = proto == prev_proto ? run + 1 : 1;
      prev_proto = proto;
      if (cap && run > cap) return false;
      // no payload byte is read unless the rule is on and proto and length agree
      const bool eq = drop_equal && proto == l_proto && len == l_len && same_bytes(heap + off, heap + l_off, len);
      l_off = off, l_len = len, l_proto = proto;
      if (!eq) return true;
      return proto < n_class && ((L.mask[(proto >> 6) & 3] >> (proto & 63)) & 1);  // n_class <= 256
    }
  };
};

}  // namespace sdxd

extern "C" size_t sdx_dispatch_scratch_bytes(int k, int32_t n) { return sdxc::scratch_bytes(k, n); }

extern "C" int sdx_dispatch_records(const sdx_bank* bank, const sdx_dispatch_rules* rules, const sdx_json_in* kinds, int k,
                                    int32_t n, sdx_desc* const* desc_out, sdx_result* const* rec_out,
                                    const uint32_t* rec_cap, uint32_t* const* cursor_out, void* scratch_dev,
                                    void* hip_stream) {
  using namespace sdxd;
  static const char FN[] = "sdx_dispatch_records";
  if (!bank) return bad_arg(FN, "null bank");
  if (!rules) return bad_arg(FN, "null rules");
  const sdx_bank_hdr* bh = sdx::bank_hdr(bank);
  const uint32_t counts[4] = {bh->n_mu, bh->n_ms, bh->n_mc, bh->n_mn};
  Slots in{};
  if (const int rc = fill_slots(FN, counts, sdx_dispatch_validate(rules, counts), kinds, k, n, nullptr, true, desc_out,
                                rec_out, rec_cap, cursor_out, scratch_dev, &in))
    return rc;
  return launch<Policy>(FN, in, k, n, *rules, hip_stream);
}
