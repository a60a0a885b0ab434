// sdx_repeat.hip -- repeat suppression (sdx_mark_repeats), hand-written HIP for gfx950.
//
// A stick delivers every telegram several times, each repetition as its own firmware line.  A
// result-bearing line (k_json's condition: descriptor OK with n_rec > 0 in its kind's launch) is a
// REPEAT when (kind, proto index, payload bytes) of its first result equal those of the previous
// result-bearing line of the stream; lines without results neither start nor break a run.
//
// Four launches on the caller's stream, no look-back and no spinning (as sdx_split.hip):
//   k_rep_keys     lane = line: the kinds' descriptors -> one 16-byte key per line, and per tile of
//                  SDX_REPEAT_TILE lines its last result-bearing line
//   k_rep_tiles    one workgroup: running maximum over the tile table -> the last result-bearing line
//                  in front of every tile, and the chunk's last one
//   k_rep_resolve  lane = line: the predecessor from the wave's ballot, the tile's waves (LDS), the tile
//                  table or the carried state; kind / proto / length, then the payload bytes
//   k_rep_state    one workgroup: key + payload of the chunk's last result-bearing line -> state
// Payload bytes are read one at a time, [off, off + len) only: nothing past a payload's end.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/sdx.h"
#include "sdx_repeat_layout.h"

namespace sdx {
int set_error(int code, const std::string& msg);  // sdx_kernels.hip
}

namespace sdxr {

constexpr int T = SDX_REPEAT_TILE;
constexpr int WAVES = T / 64;
constexpr int ST = 1024;  // k_rep_tiles' workgroup
constexpr int SWAVES = ST / 64;

struct KindIn {
  const sdx_desc* desc;  // nullptr: no launch of this kind
  const sdx_result* rec;
  const uint8_t* heap;
};
struct Kinds {
  KindIn k[4];  // by enum sdx_kind
};

__device__ __forceinline__ int last_bit(uint64_t m) { return 63 - __builtin_clzll(m); }  // m != 0

__global__ __launch_bounds__(T) void k_rep_keys(Kinds in, int n, sdx_repeat_key* __restrict__ keys,
                                                int32_t* __restrict__ tile_last) {
  __shared__ int32_t wlast[WAVES];
  const int g = blockIdx.x * T + threadIdx.x;
  sdx_repeat_key key{SDX_REPEAT_NONE, 0, 0, 0};
  if (g < n) {
#pragma unroll
    for (int kd = 3; kd >= 0; --kd) {  // a line belongs to one kind; the lowest kind wins otherwise
      if (!in.k[kd].desc) continue;
      const sdx_desc d = in.k[kd].desc[g];
      if (d.status == SDX_ST_OK && d.n_rec > 0) {
        const sdx_result r = in.k[kd].rec[d.rec_begin];
        key = sdx_repeat_key{(uint32_t)kd, r.proto, r.payload_len, r.payload_off};
      }
    }
    *reinterpret_cast<uint4*>(keys + g) = make_uint4(key.kind, key.proto, key.len, key.off);
  }
  const uint64_t m = __ballot(key.kind != SDX_REPEAT_NONE);
  if ((threadIdx.x & 63) == 0) wlast[threadIdx.x >> 6] = m ? (int)(g + last_bit(m)) : -1;
  __syncthreads();
  if (threadIdx.x == 0) {
    int last = -1;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) last = max(last, wlast[w]);
    tile_last[blockIdx.x] = last;
  }
}

// tile_prev[b] = max(tile_last[0 .. b)) (-1 = none), head[0] = max over all tiles: line indices grow
// with the tile, so the maximum is the nearest one
__global__ __launch_bounds__(ST) void k_rep_tiles(const int32_t* __restrict__ tile_last, int nt,
                                                  int32_t* __restrict__ tile_prev, int32_t* __restrict__ head) {
  __shared__ int32_t wmax[SWAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = -1;
  for (int base = 0; base < nt; base += ST) {
    const int i = base + threadIdx.x;
    const int own = i < nt ? tile_last[i] : -1;
    int incl = own;
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(incl, d);
      if (lane >= d) incl = max(incl, t);
    }
    int excl = __shfl_up(incl, 1);
    if (lane == 0) excl = -1;
    if (lane == 63) wmax[wave] = incl;
    __syncthreads();
    int before = carry, all = carry;
#pragma unroll
    for (int w = 0; w < SWAVES; ++w) {
      if (w < wave) before = max(before, wmax[w]);
      all = max(all, wmax[w]);
    }
    if (i < nt) tile_prev[i] = max(before, excl);
    carry = all;
    __syncthreads();  // wmax is written again in the next round
  }
  if (threadIdx.x == 0) head[0] = carry;
}

__device__ __forceinline__ bool same_bytes(const uint8_t* a, const uint8_t* b, uint32_t len) {
  for (uint32_t i = 0; i < len; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

__global__ __launch_bounds__(T) void k_rep_resolve(Kinds in, int n, const sdx_repeat_key* __restrict__ keys,
                                                   const int32_t* __restrict__ tile_prev,
                                                   const uint8_t* __restrict__ state, uint8_t* __restrict__ repeat) {
  __shared__ int32_t wlast[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.x * T + threadIdx.x;
  sdx_repeat_key key{SDX_REPEAT_NONE, 0, 0, 0};
  if (g < n) {
    const uint4 v = *reinterpret_cast<const uint4*>(keys + g);
    key = sdx_repeat_key{v.x, v.y, v.z, v.w};
  }
  const bool have = key.kind != SDX_REPEAT_NONE;
  const uint64_t m = __ballot(have);
  if (lane == 0) wlast[wave] = m ? (int)(g + last_bit(m)) : -1;
  __syncthreads();
  if (g >= n) return;
  if (!have) {
    repeat[g] = 0;
    return;
  }
  const uint64_t lower = lane ? m & (~0ull >> (64 - lane)) : 0ull;
  int pred = -1;
  if (lower) {
    pred = g - lane + last_bit(lower);
  } else {
    for (int w = wave - 1; w >= 0 && pred < 0; --w) pred = wlast[w];
    if (pred < 0) pred = tile_prev[blockIdx.x];
  }
  const uint8_t* mine = in.k[key.kind].heap + key.off;
  bool eq;
  if (pred >= 0) {
    const uint4 v = *reinterpret_cast<const uint4*>(keys + pred);
    eq = v.x == key.kind && v.y == key.proto && v.z == key.len && same_bytes(mine, in.k[key.kind].heap + v.w, key.len);
  } else {  // no earlier result-bearing line in this chunk: the carried state
    const sdx_repeat_state_hdr h = *reinterpret_cast<const sdx_repeat_state_hdr*>(state);
    eq = h.valid && h.kind == key.kind && h.proto == key.proto && h.len == key.len &&
         same_bytes(mine, state + sizeof(sdx_repeat_state_hdr), key.len);
  }
  repeat[g] = eq ? 1 : 0;
}

__global__ __launch_bounds__(T) void k_rep_state(Kinds in, const sdx_repeat_key* __restrict__ keys,
                                                 const int32_t* __restrict__ head, uint8_t* __restrict__ state) {
  const int last = head[0];
  if (last < 0) return;  // no result-bearing line in this chunk: the state stays
  const uint4 v = *reinterpret_cast<const uint4*>(keys + last);
  if (threadIdx.x == 0) {
    sdx_repeat_state_hdr* h = reinterpret_cast<sdx_repeat_state_hdr*>(state);
    h->valid = 1;
    h->kind = v.x;
    h->proto = v.y;
    h->len = v.z;
  }
  const uint8_t* src = in.k[v.x].heap + v.w;
  uint8_t* dst = state + sizeof(sdx_repeat_state_hdr);
  for (uint32_t i = threadIdx.x; i < v.z; i += T) dst[i] = src[i];
}

}  // namespace sdxr

extern "C" size_t sdx_repeat_state_bytes(void) { return sdx_repeat_state_size(); }
extern "C" size_t sdx_repeat_scratch_bytes(int32_t n) { return sdx_repeat_scratch_size(n); }
extern "C" int sdx_repeat_tile(void) { return SDX_REPEAT_TILE; }

extern "C" int sdx_mark_repeats(const sdx_bank* bank, const sdx_json_in* kinds, int k, int32_t n, uint8_t* repeat_dev,
                                void* key_scratch_dev, void* state_dev, void* hip_stream) {
  (void)bank;  // keys are table indices: no bank record is read
  if (!kinds || k < 1 || k > 4) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats: 1 to 4 kinds");
  if (n < 0) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats: n < 0");
  sdxr::Kinds in{};
  for (int i = 0; i < k; ++i) {
    const sdx_json_in& j = kinds[i];
    if (j.kind < SDX_KIND_MU || j.kind > SDX_KIND_MN) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats: bad kind");
    if (in.k[j.kind].desc) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats: a kind given twice");
    if (!j.desc_dev || !j.rec_dev || !j.heap_dev) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats: null buffer");
    if (j.n != n) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats: every kind's n must be the chunk's n");
    in.k[j.kind] = sdxr::KindIn{j.desc_dev, j.rec_dev, j.heap_dev};
  }
  if (n == 0) return SDX_OK;
  if (!repeat_dev || !key_scratch_dev || !state_dev)
    return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats: null buffer");
  if (((uintptr_t)key_scratch_dev | (uintptr_t)state_dev) & 15)
    return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats: key_scratch_dev and state_dev must be 16-byte aligned");
  uint8_t* s = static_cast<uint8_t*>(key_scratch_dev);
  int32_t* head = reinterpret_cast<int32_t*>(s);
  sdx_repeat_key* keys = reinterpret_cast<sdx_repeat_key*>(s + sdx_repeat_keys_off());
  int32_t* tile_last = reinterpret_cast<int32_t*>(s + sdx_repeat_tile_last_off(n));
  int32_t* tile_prev = reinterpret_cast<int32_t*>(s + sdx_repeat_tile_prev_off(n));
  const int nt = (int)sdx_repeat_tiles(n);
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(sdxr::k_rep_keys, dim3(nt), dim3(sdxr::T), 0, st, in, (int)n, keys, tile_last);
  hipLaunchKernelGGL(sdxr::k_rep_tiles, dim3(1), dim3(sdxr::ST), 0, st, (const int32_t*)tile_last, nt, tile_prev, head);
  hipLaunchKernelGGL(sdxr::k_rep_resolve, dim3(nt), dim3(sdxr::T), 0, st, in, (int)n, (const sdx_repeat_key*)keys,
                     (const int32_t*)tile_prev, (const uint8_t*)state_dev, repeat_dev);
  hipLaunchKernelGGL(sdxr::k_rep_state, dim3(1), dim3(sdxr::T), 0, st, in, (const sdx_repeat_key*)keys,
                     (const int32_t*)head, static_cast<uint8_t*>(state_dev));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return sdx::set_error(SDX_EHIP, std::string("sdx_mark_repeats: ") + hipGetErrorString(e));
  return SDX_OK;
}
