// sdx_dispatch.hip -- dispatch rules (sdx_dispatch_records), hand-written HIP for gfx950.
//
// FHEM dispatches every message a line demodulates to, but stops after maxMuMsgRepeat messages of one protocol
// and drops a message equal to the one just dispatched, unless its protocol carries dispatchequals.  The pass
// rewrites each kind's launch output -- descriptors, records, cursor -- so that every line keeps only the
// records those two rules keep (the definition: include/sdx.h), in list order, compacted into a
// dense record array in LINE order, exactly as sdx_filter_records leaves its outputs: every
// consumer of a launch's outputs runs on them unchanged.  Payloads stay where they are.
//
// The file in the order it is written:
//   device   block_excl32 / block_scan_array32: the scan idiom of sdx_profile.hip, this file's own copy
//   device   Walk: one lane's state along its line's records -- run, prev_proto and the last dispatched
//            record's {off, len, proto}, all in registers -- and the decision for the next record
//   kernel   k_dp_count  lane = line, blockIdx.y = kind: the line's kept count, its block-local exclusive
//            prefix (scratch) and the block's total
//   kernel   k_dp_scan   one block per kind: exclusive scan of the block totals, the output cursor
//   kernel   k_dp_write  lane = line, blockIdx.y = kind: the decisions again (no flag per input record is
//            stored), the descriptor, and the kept records copied 16 bytes a piece
//   host     sdx_dispatch_scratch_bytes, sdx_dispatch_records
// Count -> scan -> write through kernel boundaries: no global atomics, no spinning, the same bytes every run.
// The rules are never range-checked here: sdx_dispatch_validate passed them before anything was launched.  What
// is checked is the value that comes from the launch: proto.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/sdx.h"
#include "../../include/sdx_bank.h"
#include "sdx_dispatch_layout.h"

namespace sdx {
int set_error(int code, const std::string& msg);  // sdx_kernels.hip
const sdx_bank_hdr* bank_hdr(const sdx_bank* b);
}  // namespace sdx

namespace sdxd {

constexpr int T = SDX_DISPATCH_TILE;
constexpr uint32_t NONE = 0xFFFFFFFFu;  // no protocol: sdx_result.proto has 16 bits
static_assert(sizeof(sdx_result) == 16 && sizeof(sdx_desc) == 8, "record layout");

struct Slot {  // one kind of the call
  const sdx_desc* desc;
  const sdx_result* rec;
  const uint32_t* cursor;
  const uint8_t* heap;
  sdx_desc* desc_out;
  sdx_result* rec_out;
  uint32_t* cursor_out;
  uint2* pre;     // scratch: [n] (block-local exclusive prefix of the kept counts, the line's kept count)
  uint32_t* blk;  // scratch: [blocks] block totals, then their exclusive scan
  uint32_t rec_cap, kind, n_class, res;
};
struct Slots {
  Slot s[4];  // in the caller's order
};

__device__ __forceinline__ uint32_t wave_incl32(uint32_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(v, o);
    if (lane >= o) v += y;
  }
  return v;
}

// exclusive block scan of one count per thread; *total = the block's sum
__device__ inline uint32_t block_excl32(uint32_t v, uint32_t* total) {
  __shared__ uint32_t wsum[T / 64];
  const uint32_t inc = wave_incl32(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t base = 0, all = 0;
#pragma unroll
  for (int i = 0; i < T / 64; ++i) {
    const uint32_t s = wsum[i];
    base += i < w ? s : 0;
    all += s;
  }
  __syncthreads();  // wsum is reused by the next call
  *total = all;
  return base + inc - v;
}

// in-place exclusive scan of blk[0, nb) by one block; returns the sum
__device__ inline uint32_t block_scan_array32(uint32_t* blk, uint32_t nb) {
  uint32_t carry = 0;
  for (uint32_t c = 0; c < nb; c += T) {
    const uint32_t i = c + threadIdx.x;
    const uint32_t v = i < nb ? blk[i] : 0;
    uint32_t tot;
    const uint32_t ex = block_excl32(v, &tot);
    if (i < nb) blk[i] = carry + ex;
    carry += tot;
  }
  return carry;
}

// The kind's part of the rules, out of the kernel arguments.  The four mask words go through LDS: a lane picks
// its word by proto >> 6, and a per-lane index into values held in registers would become a private array.
struct Kind {
  uint32_t cap, drop_equal, n_class;
};
__device__ __forceinline__ Kind stage(uint64_t (&mask)[4], const sdx_dispatch_rules& rules, const Slot& k) {
  if (threadIdx.x < 4) mask[threadIdx.x] = rules.keep_equal[k.kind][threadIdx.x];
  __syncthreads();
  return Kind{(uint32_t)rules.max_repeat[k.kind], (uint32_t)rules.drop_equal, k.n_class};
}

// Byte by byte, as sdx_repeat.hip's same_bytes: the heap has no slack behind its last payload, and payloads
// stand at any alignment.  Nothing outside [a, a + len) and [b, b + len) is read.
__device__ __forceinline__ bool same_bytes(const uint8_t* a, const uint8_t* b, uint32_t len) {
  if (a == b) return true;  // two records of one payload
  for (uint32_t i = 0; i < len; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

struct Walk {
  uint32_t run = 0, prev_proto = NONE;
  uint32_t l_off = 0, l_len = 0, l_proto = NONE;  // the last record that passed the cap ("last")

  // the definition's loop body for the record {off, len | proto << 16, ..}: is it kept?
  __device__ __forceinline__ bool step(uint32_t off, uint32_t len_proto, const uint8_t* __restrict__ heap,
                                       const uint64_t (&mask)[4], const Kind& kd) {
    const uint32_t proto = len_proto >> 16, len = len_proto & 0xFFFFu;
    run = proto == prev_proto ? run + 1 : 1;
    prev_proto = proto;
    if (kd.cap && run > kd.cap) return false;
    // no payload byte is read unless the rule is on and proto and length agree
    const bool eq = kd.drop_equal && proto == l_proto && len == l_len && same_bytes(heap + off, heap + l_off, len);
    l_off = off, l_len = len, l_proto = proto;
    if (!eq) return true;
    return proto < kd.n_class && ((mask[(proto >> 6) & 3] >> (proto & 63)) & 1);  // n_class <= 256
  }
};

__global__ __launch_bounds__(T) void k_dp_count(Slots in, int n, sdx_dispatch_rules rules) {
  __shared__ uint64_t mask[4];
  const Slot& k = in.s[blockIdx.y];
  const Kind kd = stage(mask, rules, k);
  const int g = blockIdx.x * T + threadIdx.x;
  uint32_t kept = 0;
  if (g < n) {
    const sdx_desc d = k.desc[g];
    if (d.status == SDX_ST_OK && d.n_rec) {
      const uint2* r = reinterpret_cast<const uint2*>(k.rec + d.rec_begin);  // {payload_off, len | proto << 16}
      Walk w;
      for (uint32_t j = 0; j < d.n_rec; ++j) {
        const uint2 v = r[2 * j];
        kept += w.step(v.x, v.y, k.heap, mask, kd) ? 1u : 0u;
      }
    }
  }
  uint32_t tot;
  const uint32_t pre = block_excl32(kept, &tot);  // every thread of the block takes part
  if (g < n) k.pre[g] = make_uint2(pre, kept);
  if (threadIdx.x == 0) k.blk[blockIdx.x] = tot;
}

__global__ __launch_bounds__(T) void k_dp_scan(Slots in, uint32_t nb) {
  const Slot& k = in.s[blockIdx.x];
  const uint32_t total = block_scan_array32(k.blk, nb);
  if (threadIdx.x == 0) {
    k.cursor_out[0] = total;  // the demand, placed or not
    k.cursor_out[1] = k.cursor[1];
    k.cursor_out[2] = k.cursor[2] | (total > k.rec_cap ? 1u : 0u);
    k.cursor_out[3] = k.cursor[3];
  }
}

__global__ __launch_bounds__(T) void k_dp_write(Slots in, int n, sdx_dispatch_rules rules) {
  __shared__ uint64_t mask[4];
  const Slot& k = in.s[blockIdx.y];
  const Kind kd = stage(mask, rules, k);
  const int g = blockIdx.x * T + threadIdx.x;
  if (g >= n) return;
  sdx_desc d = k.desc[g];
  if (d.status == SDX_ST_OK) {  // every other status: the input's 8 bytes
    const uint2 pc = k.pre[g];
    const uint32_t begin = k.blk[blockIdx.x] + pc.x, cnt = pc.y;
    uint32_t kept = 0;
    if (cnt) {
      const uint4* r = reinterpret_cast<const uint4*>(k.rec + d.rec_begin);
      uint4* o = reinterpret_cast<uint4*>(k.rec_out);
      // a list that does not fit as a whole stores nothing: the count pass's number decides before the first store
      const bool fits = (uint64_t)begin + cnt <= k.rec_cap;
      if (fits) {
        Walk w;
        for (uint32_t j = 0; j < d.n_rec; ++j) {
          const uint4 v = r[j];
          if (w.step(v.x, v.y, k.heap, mask, kd) && kept < cnt) o[begin + kept++] = v;
        }
      }
      d = fits ? sdx_desc{begin, (uint16_t)kept, SDX_ST_OK, 0} : sdx_desc{begin, 0, SDX_ST_OVF_OUT, 0};
    } else {
      d = sdx_desc{begin, 0, SDX_ST_OK, 0};
    }
  }
  k.desc_out[g] = d;
}

static int bad_arg(const char* fn, const char* what) { return sdx::set_error(SDX_EINVAL, std::string(fn) + ": " + what); }

static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
static inline size_t blocks_of(int32_t n) { return ((size_t)n + T - 1) / T; }
static inline size_t kind_scratch(int32_t n) { return up16(8 * (size_t)n) + up16(4 * blocks_of(n)); }

}  // namespace sdxd

extern "C" size_t sdx_dispatch_scratch_bytes(int k, int32_t n) {
  if (k < 1 || k > 4 || n < 0) return 0;
  return 16 + (size_t)k * sdxd::kind_scratch(n);  // never 0
}

extern "C" int sdx_dispatch_records(const sdx_bank* bank, const sdx_dispatch_rules* rules, const sdx_json_in* kinds, int k,
                                    int32_t n, sdx_desc* const* desc_out, sdx_result* const* rec_out,
                                    const uint32_t* rec_cap, uint32_t* const* cursor_out, void* scratch_dev,
                                    void* hip_stream) {
  using namespace sdxd;
  static const char FN[] = "sdx_dispatch_records";
  if (!bank) return bad_arg(FN, "null bank");
  if (!rules) return bad_arg(FN, "null rules");
  if (!kinds || k < 1 || k > 4) return bad_arg(FN, "1 to 4 kinds");
  if (n < 0) return bad_arg(FN, "n < 0");
  if (!desc_out || !rec_out || !rec_cap || !cursor_out || !scratch_dev) return bad_arg(FN, "null output or scratch");
  if ((uintptr_t)scratch_dev & 15) return bad_arg(FN, "scratch_dev must be 16-byte aligned");
  const sdx_bank_hdr* bh = sdx::bank_hdr(bank);
  const uint32_t counts[4] = {bh->n_mu, bh->n_ms, bh->n_mc, bh->n_mn};
  if (const char* why = sdx_dispatch_validate(rules, counts)) return bad_arg(FN, why);
  Slots in{};
  bool seen[4] = {};
  uint8_t* sc = static_cast<uint8_t*>(scratch_dev);
  for (int i = 0; i < k; ++i) {
    const sdx_json_in& j = kinds[i];
    if (j.kind < SDX_KIND_MU || j.kind > SDX_KIND_MN) return bad_arg(FN, "bad kind");
    if (seen[j.kind]) return bad_arg(FN, "a kind given twice");
    seen[j.kind] = true;
    if (!j.desc_dev || !j.rec_dev || !j.cursor_dev || !j.heap_dev) return bad_arg(FN, "null buffer");
    if (j.n != n) return bad_arg(FN, "every kind's n must be the chunk's n");
    if (!desc_out[i] || !rec_out[i] || !cursor_out[i]) return bad_arg(FN, "a null output");
    if (((uintptr_t)desc_out[i] & 3) || ((uintptr_t)cursor_out[i] & 3) || ((uintptr_t)rec_out[i] & 15) ||
        ((uintptr_t)j.rec_dev & 15))
      return bad_arg(FN, "descriptors and cursors must be 4-byte, records 16-byte aligned");
    Slot& s = in.s[i];
    s = Slot{j.desc_dev, j.rec_dev, j.cursor_dev, j.heap_dev, desc_out[i], rec_out[i], cursor_out[i],
             reinterpret_cast<uint2*>(sc), reinterpret_cast<uint32_t*>(sc + up16(8 * (size_t)n)),
             rec_cap[i], (uint32_t)j.kind, counts[j.kind], 0};
    sc += kind_scratch(n);
  }
  hipStream_t st = (hipStream_t)hip_stream;
  const uint32_t nb = (uint32_t)blocks_of(n);
  if (nb) hipLaunchKernelGGL(k_dp_count, dim3(nb, k), dim3(T), 0, st, in, (int)n, *rules);
  hipLaunchKernelGGL(k_dp_scan, dim3(k), dim3(T), 0, st, in, nb);
  if (nb) hipLaunchKernelGGL(k_dp_write, dim3(nb, k), dim3(T), 0, st, in, (int)n, *rules);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SDX_OK : sdx::set_error(SDX_EHIP, std::string(FN) + ": " + hipGetErrorString(e));
}
