// sdx_index.hip -- a chunk's line -> record-range index over all its kinds (sdx_index_records), hand-written HIP
// for gfx950.
//
// Every kind's launch keeps its own record array, so "the texts of line g" has no place of its own in a chunk's
// result: a line's records stand at its kind's [rec_begin, rec_begin + n_rec).  The index gives every line a range
// [first[g], first[g + 1]) of CHUNK record indices, in line order, shared by the kinds -- a line belongs to one of
// them --, which sdx_serialize_json_lines writes its texts' offsets and lengths at: one off / len array and one
// text buffer per chunk, read back with one sized copy.
//
// Count -> scan -> write through kernel boundaries on sdx_compact.h's scan primitives; no global atomics, no
// spinning, the same bytes every run:
//   k_idx_count  lane = line: the line's count (the n_rec of its OK descriptor with records, 0 for a skipped
//                line), its block-local exclusive prefix -> first[g], the block's total -> blk[block]
//   k_idx_scan   one block: exclusive scan of the block totals; first[n] = the chunk's total
//   k_idx_add    lane = line: first[g] += blk[block]
#include "sdx_compact.h"

namespace sdxi {

using namespace sdxc;

struct Kinds {
  const sdx_desc* desc[4];  // in the caller's order; [k, 4): nullptr
};

__global__ __launch_bounds__(T) void k_idx_count(Kinds in, int n, const uint8_t* __restrict__ skip,
                                                 uint32_t* __restrict__ first, uint32_t* __restrict__ blk) {
  const int g = blockIdx.x * T + threadIdx.x;
  uint32_t cnt = 0;
  if (g < n && !(skip && skip[g])) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!in.desc[i]) continue;
      const sdx_desc d = in.desc[i][g];
      cnt += d.status == SDX_ST_OK ? d.n_rec : 0u;  // at most one kind's term is non-zero
    }
  }
  uint32_t tot;
  const uint32_t pre = block_excl32(cnt, &tot);  // every thread of the block takes part
  if (g < n) first[g] = pre;
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

__global__ __launch_bounds__(T) void k_idx_scan(uint32_t* __restrict__ blk, uint32_t nb, uint32_t* __restrict__ total) {
  const uint32_t sum = block_scan_array32(blk, nb);
  if (threadIdx.x == 0) *total = sum;
}

__global__ __launch_bounds__(T) void k_idx_add(int n, const uint32_t* __restrict__ blk, uint32_t* __restrict__ first) {
  const int g = blockIdx.x * T + threadIdx.x;
  if (g < n) first[g] += blk[blockIdx.x];
}

}  // namespace sdxi

extern "C" size_t sdx_index_scratch_bytes(int32_t n) {
  if (n < 0) return 0;
  const size_t b = sdxc::up16(4 * sdxc::blocks_of(n));
  return b ? b : 16;  // never 0
}

extern "C" int sdx_index_records(const sdx_json_in* kinds, int32_t k, int32_t n, const uint8_t* skip_dev,
                                 uint32_t* first_dev, void* scratch_dev, void* hip_stream) {
  using namespace sdxi;
  static const char FN[] = "sdx_index_records";
  // what sdx_mark_repeats refuses, in its order
  if (!kinds || k < 1 || k > 4) return bad_arg(FN, "1 to 4 kinds");
  if (n < 0) return bad_arg(FN, "n < 0");
  Kinds in{};
  bool seen[4] = {};
  for (int i = 0; i < k; ++i) {
    const sdx_json_in& j = kinds[i];
    if (j.kind < SDX_KIND_MU || j.kind > SDX_KIND_MN) return bad_arg(FN, "bad kind");
    if (seen[j.kind]) return bad_arg(FN, "a kind given twice");
    seen[j.kind] = true;
    if (!j.desc_dev || !j.rec_dev || !j.heap_dev) return bad_arg(FN, "null buffer");
    if (j.n != n) return bad_arg(FN, "every kind's n must be the chunk's n");
    if ((uintptr_t)j.desc_dev & 3) return bad_arg(FN, "descriptors must be 4-byte aligned");
    in.desc[i] = j.desc_dev;
  }
  if (!first_dev) return bad_arg(FN, "null first_dev");
  if (n > 0 && !scratch_dev) return bad_arg(FN, "null scratch_dev");
  if (((uintptr_t)first_dev | (uintptr_t)scratch_dev) & 3) return bad_arg(FN, "first_dev and scratch_dev must be 4-byte aligned");
  hipStream_t st = (hipStream_t)hip_stream;
  uint32_t* blk = static_cast<uint32_t*>(scratch_dev);
  const uint32_t nb = (uint32_t)blocks_of(n);
  if (nb) hipLaunchKernelGGL(k_idx_count, dim3(nb), dim3(T), 0, st, in, (int)n, skip_dev, first_dev, blk);
  hipLaunchKernelGGL(k_idx_scan, dim3(1), dim3(T), 0, st, blk, nb, first_dev + n);  // n = 0: first[0] = 0, blk unread
  if (nb) hipLaunchKernelGGL(k_idx_add, dim3(nb), dim3(T), 0, st, (int)n, (const uint32_t*)blk, first_dev);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SDX_OK : sdx::set_error(SDX_EHIP, std::string(FN) + ": " + hipGetErrorString(e));
}
