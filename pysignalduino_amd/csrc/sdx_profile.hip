// sdx_profile.hip -- receiver profiles (sdx_filter_records), hand-written HIP for gfx950.
//
// A stream merges up to 4,096 receivers; every line carries its source id.  A PROFILE is a set of enabled
// protocol classes per kind, a PROFILE TABLE maps every source id to one of up to 64 profiles (the blob:
// sdx_profile_layout.h, compiled by pysignalduino_amd/profiles.py).  The pass rewrites each kind's launch
// output -- descriptors, records, cursor -- so that every line keeps only the records whose class its
// source's profile enables, in list order, compacted into a dense record array in LINE order
// (DESIGN.md §4n).  Payloads stay where they are: a kept record is copied with all its 16 bytes.
//
// The file in the order it is written:
//   device   block_excl32 / block_scan_array32: sdx_exchange.hip's scan idiom on 32-bit counts
//   kernel   k_pf_count  lane = line, blockIdx.y = kind: the line's kept count, its block-local exclusive
//            prefix (scratch) and the block's total
//   kernel   k_pf_scan   one block per kind: exclusive scan of the block totals, the output cursor
//   kernel   k_pf_write  lane = line, blockIdx.y = kind: descriptor, and the kept records copied 16 bytes
//            a piece to [block offset + prefix, ...)
//   host     sdx_profile_table_create / _destroy, sdx_profile_check, sdx_profile_scratch_bytes, sdx_filter_records
// Count -> scan -> write through kernel boundaries: no global atomics, no spinning, the same bytes every run.
// Table contents are never range-checked here: sdx_profile_validate passed the whole blob before it was
// uploaded.  What is checked are the values that come from the launch: proto and the source id.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/sdx.h"
#include "../../include/sdx_bank.h"
#include "sdx_profile_layout.h"

namespace sdx {
int set_error(int code, const std::string& msg);  // sdx_kernels.hip
const sdx_bank_hdr* bank_hdr(const sdx_bank* b);
}  // namespace sdx

struct sdx_profile_table {
  int device;
  uint8_t* dev;  // the blob
  sdx_profile_hdr hdr;
};

namespace sdxp {

constexpr int T = SDX_PROFILE_TILE;
constexpr uint32_t HDR = sizeof(sdx_profile_hdr);
static_assert(sizeof(sdx_result) == 16 && sizeof(sdx_desc) == 8, "record layout");

struct Slot {  // one kind of the call
  const sdx_desc* desc;
  const sdx_result* rec;
  const uint32_t* cursor;
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

// The table's part one kind's block needs, in LDS: masks[p] = the kind's four words of profile p, then
// of_source.  8 B-aligned words first, bytes behind them.
struct Staged {
  uint64_t mask[SDX_PROFILE_MAX][4];
  uint8_t of_source[SDX_PROFILE_SOURCES_MAX];
};

__device__ __forceinline__ void stage(Staged& L, const uint8_t* __restrict__ blob, uint32_t P, uint32_t S, uint32_t kind) {
  const uint64_t* m = reinterpret_cast<const uint64_t*>(blob + HDR);  // the blob is 16-byte aligned, HDR = 48
  for (uint32_t i = threadIdx.x; i < 4 * P; i += T) L.mask[i >> 2][i & 3] = m[(i >> 2) * 16 + kind * 4 + (i & 3)];
  const uint32_t* s = reinterpret_cast<const uint32_t*>(blob + HDR + SDX_PROFILE_MASK_BYTES * P);  // padded to 16 bytes
  uint32_t* d = reinterpret_cast<uint32_t*>(L.of_source);
  for (uint32_t i = threadIdx.x; i < (S + 3) / 4; i += T) d[i] = s[i];
  __syncthreads();
}

// the line's profile index; a source id outside [0, S) keeps nothing (-1)
__device__ __forceinline__ int line_profile(const Staged& L, const int32_t* __restrict__ source, int g, uint32_t S) {
  const int32_t src = source ? source[g] : 0;
  return src >= 0 && (uint32_t)src < S ? (int)L.of_source[src] : -1;
}

// One 8-byte LDS read per record: the mask word of its class.  (The line's four words held in registers and picked
// by a chain of selects were compiled into a private array indexed by proto >> 6: 48 bytes of scratch memory a lane.)
__device__ __forceinline__ bool enabled(const Staged& L, int p, uint32_t proto, uint32_t n_class) {
  const uint64_t word = L.mask[p < 0 ? 0 : p][(proto >> 6) & 3];  // always inside the staged masks
  return p >= 0 && proto < n_class && ((word >> (proto & 63)) & 1);  // n_class <= 256
}

__global__ __launch_bounds__(T) void k_pf_count(Slots in, int n, const uint8_t* __restrict__ blob, uint32_t P, uint32_t S,
                                                const int32_t* __restrict__ source) {
  __shared__ Staged L;
  const Slot& k = in.s[blockIdx.y];
  stage(L, blob, P, S, k.kind);
  const int g = blockIdx.x * T + threadIdx.x;
  uint32_t kept = 0;
  if (g < n) {
    const sdx_desc d = k.desc[g];
    if (d.status == SDX_ST_OK && d.n_rec) {
      const int m = line_profile(L, source, g, S);
      const sdx_result* r = k.rec + d.rec_begin;
      for (uint32_t j = 0; j < d.n_rec; ++j) kept += enabled(L, m, r[j].proto, k.n_class) ? 1u : 0u;
    }
  }
  uint32_t tot;
  const uint32_t pre = block_excl32(kept, &tot);  // every thread of the block takes part
  if (g < n) k.pre[g] = make_uint2(pre, kept);
  if (threadIdx.x == 0) k.blk[blockIdx.x] = tot;
}

__global__ __launch_bounds__(T) void k_pf_scan(Slots in, uint32_t nb) {
  const Slot& k = in.s[blockIdx.x];
  const uint32_t total = block_scan_array32(k.blk, nb);
  if (threadIdx.x == 0) {
    k.cursor_out[0] = total;  // the demand, placed or not
    k.cursor_out[1] = k.cursor[1];
    k.cursor_out[2] = k.cursor[2] | (total > k.rec_cap ? 1u : 0u);
    k.cursor_out[3] = k.cursor[3];
  }
}

__global__ __launch_bounds__(T) void k_pf_write(Slots in, int n, const uint8_t* __restrict__ blob, uint32_t P, uint32_t S,
                                                const int32_t* __restrict__ source) {
  __shared__ Staged L;
  const Slot& k = in.s[blockIdx.y];
  stage(L, blob, P, S, k.kind);
  const int g = blockIdx.x * T + threadIdx.x;
  if (g >= n) return;
  sdx_desc d = k.desc[g];
  if (d.status == SDX_ST_OK) {  // every other status: the input's 8 bytes
    const uint2 pc = k.pre[g];
    const uint32_t begin = k.blk[blockIdx.x] + pc.x, cnt = pc.y;
    uint32_t kept = 0;
    if (cnt) {
      const int m = line_profile(L, source, g, S);
      const uint4* r = reinterpret_cast<const uint4*>(k.rec + d.rec_begin);
      uint4* o = reinterpret_cast<uint4*>(k.rec_out);
      // a list that does not fit as a whole stores nothing: the count pass's number decides before the first store
      const bool fits = (uint64_t)begin + cnt <= k.rec_cap;
      if (fits) {
        for (uint32_t j = 0; j < d.n_rec; ++j) {
          const uint4 v = r[j];
          if (enabled(L, m, v.y >> 16, k.n_class) && kept < cnt) o[begin + kept++] = v;  // proto: the high half of word 1
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

extern "C" size_t sdx_profile_scratch_bytes(int k, int32_t n) {
  if (k < 1 || k > 4 || n < 0) return 0;
  return 16 + (size_t)k * sdxp::kind_scratch(n);  // never 0
}

extern "C" int sdx_filter_records(const sdx_bank* bank, const sdx_profile_table* table, const sdx_json_in* kinds, int k,
                                  int32_t n, const int32_t* source_dev, sdx_desc* const* desc_out,
                                  sdx_result* const* rec_out, const uint32_t* rec_cap, uint32_t* const* cursor_out,
                                  void* scratch_dev, void* hip_stream) {
  using namespace sdxp;
  static const char FN[] = "sdx_filter_records";
  if (!bank) return bad_arg(FN, "null bank");
  if (!table || !table->dev) return bad_arg(FN, "null table");
  if (!kinds || k < 1 || k > 4) return bad_arg(FN, "1 to 4 kinds");
  if (n < 0) return bad_arg(FN, "n < 0");
  if (!desc_out || !rec_out || !rec_cap || !cursor_out || !scratch_dev) return bad_arg(FN, "null output or scratch");
  if ((uintptr_t)source_dev & 3) return bad_arg(FN, "source_dev must be 4-byte aligned");
  if ((uintptr_t)scratch_dev & 15) return bad_arg(FN, "scratch_dev must be 16-byte aligned");
  const sdx_bank_hdr* bh = sdx::bank_hdr(bank);
  const uint32_t counts[4] = {bh->n_mu, bh->n_ms, bh->n_mc, bh->n_mn};
  for (int kd = 0; kd < 4; ++kd)
    if (table->hdr.n_class[kd] != counts[kd]) return bad_arg(FN, "the table was compiled for another bank");
  Slots in{};
  bool seen[4] = {};
  uint8_t* sc = static_cast<uint8_t*>(scratch_dev);
  for (int i = 0; i < k; ++i) {
    const sdx_json_in& j = kinds[i];
    if (j.kind < SDX_KIND_MU || j.kind > SDX_KIND_MN) return bad_arg(FN, "bad kind");
    if (seen[j.kind]) return bad_arg(FN, "a kind given twice");
    seen[j.kind] = true;
    if (!j.desc_dev || !j.rec_dev || !j.cursor_dev) return bad_arg(FN, "null buffer");
    if (j.n != n) return bad_arg(FN, "every kind's n must be the chunk's n");
    if (!desc_out[i] || !rec_out[i] || !cursor_out[i]) return bad_arg(FN, "a null output");
    if (((uintptr_t)desc_out[i] & 3) || ((uintptr_t)cursor_out[i] & 3) || ((uintptr_t)rec_out[i] & 15) ||
        ((uintptr_t)j.rec_dev & 15))
      return bad_arg(FN, "descriptors and cursors must be 4-byte, records 16-byte aligned");
    Slot& s = in.s[i];
    s = Slot{j.desc_dev, j.rec_dev, j.cursor_dev, desc_out[i], rec_out[i], cursor_out[i],
             reinterpret_cast<uint2*>(sc), reinterpret_cast<uint32_t*>(sc + up16(8 * (size_t)n)),
             rec_cap[i], (uint32_t)j.kind, counts[j.kind], 0};
    sc += kind_scratch(n);
  }
  hipStream_t st = (hipStream_t)hip_stream;
  const uint32_t nb = (uint32_t)blocks_of(n);
  const uint32_t P = table->hdr.n_profiles, S = table->hdr.n_sources;
  if (nb) hipLaunchKernelGGL(k_pf_count, dim3(nb, k), dim3(T), 0, st, in, (int)n, table->dev, P, S, source_dev);
  hipLaunchKernelGGL(k_pf_scan, dim3(k), dim3(T), 0, st, in, nb);
  if (nb) hipLaunchKernelGGL(k_pf_write, dim3(nb, k), dim3(T), 0, st, in, (int)n, table->dev, P, S, source_dev);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SDX_OK : sdx::set_error(SDX_EHIP, std::string(FN) + ": " + hipGetErrorString(e));
}
