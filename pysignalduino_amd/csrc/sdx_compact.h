// sdx_compact.h -- the record-compaction skeleton of sdx_filter_records and sdx_dispatch_records.
//
// Both passes rewrite each kind's launch output -- descriptors, records, cursor -- so that every line keeps a
// subset of its records, in list order, compacted into a dense record array in LINE order.  Payloads stay
// where they are: a kept record is copied with all its 16 bytes.  Count -> scan -> write through kernel
// boundaries: no global atomics, no spinning, the same bytes every run.
//   kernel   k_count<P>  lane = line, blockIdx.y = kind: the line's kept count, its block-local exclusive
//            prefix (scratch) and the block's total
//   kernel   k_scan      one block per kind: exclusive scan of the block totals, the output cursor
//   kernel   k_write<P>  lane = line, blockIdx.y = kind: the decisions again (no flag per input record is
//            stored), the descriptor, and the kept records copied 16 bytes a piece to [block offset + prefix, ...)
//   host     scratch_bytes, fill_slots (the common argument checks), launch<P>
// What a pass keeps is its policy P:
//   P::Args    the by-value kernel arguments
//   P::Staged  what a block holds in LDS, filled by  static void P::stage(Staged&, const Args&, const Slot&)
//              (every thread of the block calls it; it ends with a barrier)
//   P::Line    one lane's state along its line's records: Line(const Staged&, const Args&, const Slot&, int line)
//              and  bool keep(const uint4& record), called once per record in list order.  A Line reads what it
//              picks per record (a mask word by proto >> 6) from Staged: a per-lane index into values held in
//              registers becomes a private array in scratch memory.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/sdx.h"
#include "../../include/sdx_bank.h"

namespace sdx {
int set_error(int code, const std::string& msg);  // sdx_kernels.hip
const sdx_bank_hdr* bank_hdr(const sdx_bank* b);
}  // namespace sdx

namespace sdxc {

constexpr int T = 256;  // lines per workgroup
static_assert(sizeof(sdx_result) == 16 && sizeof(sdx_desc) == 8, "record layout");

struct Slot {  // one kind of the call
  const sdx_desc* desc;
  const sdx_result* rec;
  const uint32_t* cursor;
  const uint8_t* heap;  // payloads; only a policy reads them
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

// exclusive block scan of one count per thread; *total = the block's sum (sdx_exchange.hip's idiom on 32-bit counts)
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

template <class P>
__global__ __launch_bounds__(T) void k_count(Slots in, int n, typename P::Args a) {
  __shared__ typename P::Staged L;
  const Slot& k = in.s[blockIdx.y];
  P::stage(L, a, k);
  const int g = blockIdx.x * T + threadIdx.x;
  uint32_t kept = 0;
  if (g < n) {
    const sdx_desc d = k.desc[g];
    if (d.status == SDX_ST_OK && d.n_rec) {
      const uint4* r = reinterpret_cast<const uint4*>(k.rec + d.rec_begin);
      typename P::Line line(L, a, k, g);
      for (uint32_t j = 0; j < d.n_rec; ++j) kept += line.keep(r[j]) ? 1u : 0u;  // only the words P reads are loaded
    }
  }
  uint32_t tot;
  const uint32_t pre = block_excl32(kept, &tot);  // every thread of the block takes part
  if (g < n) k.pre[g] = make_uint2(pre, kept);
  if (threadIdx.x == 0) k.blk[blockIdx.x] = tot;
}

// static: one copy per unit that includes this file
static __global__ __launch_bounds__(T) void k_scan(Slots in, uint32_t nb) {
  const Slot& k = in.s[blockIdx.x];
  const uint32_t total = block_scan_array32(k.blk, nb);
  if (threadIdx.x == 0) {
    k.cursor_out[0] = total;  // the demand, placed or not
    k.cursor_out[1] = k.cursor[1];
    k.cursor_out[2] = k.cursor[2] | (total > k.rec_cap ? 1u : 0u);
    k.cursor_out[3] = k.cursor[3];
  }
}

template <class P>
__global__ __launch_bounds__(T) void k_write(Slots in, int n, typename P::Args a) {
  __shared__ typename P::Staged L;
  const Slot& k = in.s[blockIdx.y];
  P::stage(L, a, k);
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
        typename P::Line line(L, a, k, g);
        for (uint32_t j = 0; j < d.n_rec; ++j) {
          const uint4 v = r[j];
          if (line.keep(v) && kept < cnt) o[begin + kept++] = v;
        }
      }
      d = fits ? sdx_desc{begin, (uint16_t)kept, SDX_ST_OK, 0} : sdx_desc{begin, 0, SDX_ST_OVF_OUT, 0};
    } else {
      d = sdx_desc{begin, 0, SDX_ST_OK, 0};
    }
  }
  k.desc_out[g] = d;
}

inline int bad_arg(const char* fn, const char* what) { return sdx::set_error(SDX_EINVAL, std::string(fn) + ": " + what); }

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
inline size_t blocks_of(int32_t n) { return ((size_t)n + T - 1) / T; }
inline size_t kind_scratch(int32_t n) { return up16(8 * (size_t)n) + up16(4 * blocks_of(n)); }

inline size_t scratch_bytes(int k, int32_t n) {
  if (k < 1 || k > 4 || n < 0) return 0;
  return 16 + (size_t)k * kind_scratch(n);  // never 0
}

// The checks of everything both entries take, in the order both report them, and the slots.  ``source_dev``: null
// where the entry has none.  ``why``: the entry's verdict on its own table or rules against the bank's ``counts``
// (null: fine), reported where it stands among the checks.  ``need_heap``: the policy reads payloads.
inline int fill_slots(const char* fn, const uint32_t (&counts)[4], const char* why, const sdx_json_in* kinds, int k,
                      int32_t n, const void* source_dev, bool need_heap, sdx_desc* const* desc_out,
                      sdx_result* const* rec_out, const uint32_t* rec_cap, uint32_t* const* cursor_out,
                      void* scratch_dev, Slots* in) {
  if (!kinds || k < 1 || k > 4) return bad_arg(fn, "1 to 4 kinds");
  if (n < 0) return bad_arg(fn, "n < 0");
  if (!desc_out || !rec_out || !rec_cap || !cursor_out || !scratch_dev) return bad_arg(fn, "null output or scratch");
  if ((uintptr_t)source_dev & 3) return bad_arg(fn, "source_dev must be 4-byte aligned");
  if ((uintptr_t)scratch_dev & 15) return bad_arg(fn, "scratch_dev must be 16-byte aligned");
  if (why) return bad_arg(fn, why);
  bool seen[4] = {};
  uint8_t* sc = static_cast<uint8_t*>(scratch_dev);
  for (int i = 0; i < k; ++i) {
    const sdx_json_in& j = kinds[i];
    if (j.kind < SDX_KIND_MU || j.kind > SDX_KIND_MN) return bad_arg(fn, "bad kind");
    if (seen[j.kind]) return bad_arg(fn, "a kind given twice");
    seen[j.kind] = true;
    if (!j.desc_dev || !j.rec_dev || !j.cursor_dev || (need_heap && !j.heap_dev)) return bad_arg(fn, "null buffer");
    if (j.n != n) return bad_arg(fn, "every kind's n must be the chunk's n");
    if (!desc_out[i] || !rec_out[i] || !cursor_out[i]) return bad_arg(fn, "a null output");
    if (((uintptr_t)desc_out[i] & 3) || ((uintptr_t)cursor_out[i] & 3) || ((uintptr_t)rec_out[i] & 15) ||
        ((uintptr_t)j.rec_dev & 15))
      return bad_arg(fn, "descriptors and cursors must be 4-byte, records 16-byte aligned");
    in->s[i] = Slot{j.desc_dev, j.rec_dev, j.cursor_dev, j.heap_dev, desc_out[i], rec_out[i], cursor_out[i],
                    reinterpret_cast<uint2*>(sc), reinterpret_cast<uint32_t*>(sc + up16(8 * (size_t)n)),
                    rec_cap[i], (uint32_t)j.kind, counts[j.kind], 0};
    sc += kind_scratch(n);
  }
  return SDX_OK;
}

// the three launches for all k kinds
template <class P>
int launch(const char* fn, const Slots& in, int k, int32_t n, const typename P::Args& a, void* hip_stream) {
  hipStream_t st = (hipStream_t)hip_stream;
  const uint32_t nb = (uint32_t)blocks_of(n);
  if (nb) hipLaunchKernelGGL(k_count<P>, dim3(nb, k), dim3(T), 0, st, in, (int)n, a);
  hipLaunchKernelGGL(k_scan, dim3(k), dim3(T), 0, st, in, nb);
  if (nb) hipLaunchKernelGGL(k_write<P>, dim3(nb, k), dim3(T), 0, st, in, (int)n, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SDX_OK : sdx::set_error(SDX_EHIP, std::string(fn) + ": " + hipGetErrorString(e));
}

}  // namespace sdxc
