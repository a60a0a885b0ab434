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
// sdx_mark_repeats_timed (a run also ends when its last published line is too old) follows below, with
// kernels of its own behind k_rep_keys and k_rep_tiles; sdx_mark_repeats_by_source (one run per source id of
// a stream that merges several receivers) sorts the lines by id and runs the timed kernels over the result.
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

// ---- sdx_mark_repeats_timed: a run also ends when its anchor is more than W old -----
// A stream carries (K, T): K the key of the previous result-bearing line, T the time of the last one that
// was not marked.  A line is a repeat when its key equals K and t - T <= W; otherwise it is published and
// T = t.  T is the last PUBLISHED line's time, so a decision depends on the decisions before it:
//   segment head  a result-bearing line whose key differs from its predecessor's, or whose gap to it
//                 exceeds W: T is never later than the predecessor's time, so it is published whatever
//                 came before.  Found per line, as eq above.  The chunk's first result-bearing line is
//                 always a head; the carried (K, T) decides whether it is published (SDX_RT_SREP: not).
//   segment       a head and the lines behind it up to the next head: equal keys, every gap <= W
//   orbit         inside a segment the published lines are head, succ(head), succ(succ(head)), ... with
//                 succ(a) = the segment's first line behind a with t > t(a) + W
// Eight launches, the first two those of sdx_mark_repeats:
//   k_rep_keys, k_rep_tiles    keys, the last result-bearing line in front of every tile
//   k_rept_heads   lane = line: predecessor as k_rep_resolve, key compare and gap -> flags, te (a line
//                  without results takes its predecessor's time, so te is non-decreasing and a search
//                  never stops on such a line), the tile's last head
//   k_rep_tiles    over the tiles' last heads -> the last head in front of every tile
//   k_rept_seg     lane = line: the line's segment head
//   k_rept_succ    lane = line: succ by binary search, inside the wave over the lanes' registers
//                  (shuffles), behind it galloping over te / seg in memory; then pointer doubling over
//                  the tile (LDS, 8 rounds): the orbit's last line inside the tile and its first behind it
//   k_rept_chain   one workgroup, thread = tile: an orbit that leaves its head's tile is followed from
//                  tile to tile (one load per tile it enters; orbits of different segments in parallel)
//                  and entered into the tiles it lands in; then the state: K as k_rep_state, T = the
//                  time of the last line of the last head's orbit
//   k_rept_mark    lane = line: the tile's heads and its entry walk their orbit inside the tile (LDS)
// Every search and walk is bounded by indices: on times that decrease the mask is unspecified, but
// nothing leaves its buffer and every loop ends.
namespace sdxt {
using sdxr::Kinds;
using sdxr::last_bit;
using sdxr::same_bytes;
using sdxr::ST;
using sdxr::T;
using sdxr::WAVES;

// t - anchor > w for anchor <= t (the precondition), whatever the two values: no signed overflow
__device__ __forceinline__ bool past(int64_t t, int64_t anchor, int64_t w) {
  return (uint64_t)t - (uint64_t)anchor > (uint64_t)w;
}

// sdx_mark_repeats_by_source runs these passes over POSITIONS (the lines sorted by source id, stable), BS =
// true; the two entries above it instantiate BS = false, where the struct is not read.
struct BySrc {
  const uint32_t* psrc;  // the position's source id, < S
  const int32_t* perm;   // position -> line
  int32_t* ipred;        // out: the last result-bearing position at or in front of the position
  int S;
};
template <bool BS>
__device__ __forceinline__ const uint8_t* slot_of(const uint8_t* state, const BySrc& bs, int g) {
  if constexpr (BS) {
    const uint32_t s = bs.psrc[g];
    return state + (size_t)(s < (uint32_t)bs.S ? s : 0u) * SDX_REPEAT_TIMED_STATE_SIZE;
  } else {
    return state;
  }
}

template <bool BS>
__global__ __launch_bounds__(T) void k_rept_heads(Kinds in, int n, const sdx_repeat_key* __restrict__ keys,
                                                  const int32_t* __restrict__ tile_prev,
                                                  const int64_t* __restrict__ times, int64_t window,
                                                  const uint8_t* __restrict__ state, int64_t* __restrict__ te,
                                                  uint8_t* __restrict__ flags, int32_t* __restrict__ tile_head,
                                                  int32_t* __restrict__ tile_arr, BySrc bs) {
  __shared__ int32_t wlast[WAVES];
  __shared__ int32_t whead[WAVES];
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
  uint32_t f = 0;
  if (g < n) {
    const uint64_t lower = lane ? m & (~0ull >> (64 - lane)) : 0ull;
    int pred = -1;
    if (lower) {
      pred = g - lane + last_bit(lower);
    } else {
      for (int w = wave - 1; w >= 0 && pred < 0; --w) pred = wlast[w];
      if (pred < 0) pred = tile_prev[blockIdx.x];
    }
    int64_t t = 0;
    bool inrun = pred >= 0;  // the predecessor decides; otherwise the carried state
    if constexpr (BS) {
      bs.ipred[g] = have ? g : pred;
      inrun = inrun && bs.psrc[pred] == bs.psrc[g];  // a source's first result-bearing line: its own state
    }
    if (have) {
      t = times[g];
      f = SDX_RT_RB;
      const uint8_t* mine = in.k[key.kind].heap + key.off;
      if (inrun) {
        const uint4 v = *reinterpret_cast<const uint4*>(keys + pred);
        const bool cont = !past(t, times[pred], window) && v.x == key.kind && v.y == key.proto && v.z == key.len &&
                          same_bytes(mine, in.k[key.kind].heap + v.w, key.len);
        if (!cont) f |= SDX_RT_HEAD;
      } else {  // the chunk's first result-bearing line: the carried (K, T)
        const uint8_t* slot = slot_of<BS>(state, bs, g);
        const sdx_repeat_timed_state_hdr h = *reinterpret_cast<const sdx_repeat_timed_state_hdr*>(slot);
        f |= SDX_RT_HEAD;
        if (h.valid && !past(t, h.t, window) && h.kind == key.kind && h.proto == key.proto && h.len == key.len &&
            same_bytes(mine, slot + sizeof(sdx_repeat_timed_state_hdr), key.len))
          f |= SDX_RT_SREP;
      }
    } else if (pred >= 0) {
      t = times[pred];
    }
    te[g] = t;
    flags[g] = (uint8_t)f;
  }
  const uint64_t hm = __ballot((f & SDX_RT_HEAD) != 0);
  if (lane == 0) whead[wave] = hm ? (int)(g + last_bit(hm)) : -1;
  __syncthreads();
  if (threadIdx.x == 0) {
    int last = -1;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) last = max(last, whead[w]);
    tile_head[blockIdx.x] = last;
    tile_arr[blockIdx.x] = -1;
  }
}

__global__ __launch_bounds__(T) void k_rept_seg(int n, const uint8_t* __restrict__ flags,
                                                const int32_t* __restrict__ tile_prevhead, int32_t* __restrict__ seg) {
  __shared__ int32_t whead[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.x * T + threadIdx.x;
  const bool head = g < n && (flags[g] & SDX_RT_HEAD);
  const uint64_t hm = __ballot(head);
  if (lane == 0) whead[wave] = hm ? (int)(g + last_bit(hm)) : -1;
  __syncthreads();
  if (g >= n) return;
  const uint64_t upto = hm & (~0ull >> (63 - lane));
  int s = -1;
  if (upto) {
    s = g - lane + last_bit(upto);
  } else {
    for (int w = wave - 1; w >= 0 && s < 0; --w) s = whead[w];
    if (s < 0) s = tile_prevhead[blockIdx.x];
  }
  seg[g] = s;
}

template <bool BS>
__global__ __launch_bounds__(T) void k_rept_succ(int n, const int64_t* __restrict__ te, const int32_t* __restrict__ seg,
                                                 const uint8_t* __restrict__ flags, int64_t window,
                                                 const uint8_t* __restrict__ state, int32_t* __restrict__ succ,
                                                 int32_t* __restrict__ exitv, int32_t* __restrict__ lastv, BySrc bs) {
  __shared__ int32_t sg[T];
  __shared__ int32_t J[T];
  __shared__ int32_t L[T];
  const int tid = threadIdx.x, lane = tid & 63;
  const int base = blockIdx.x * T;
  const int g = base + tid;
  const long long tv = g < n ? te[g] : 0;
  const int sv = g < n ? seg[g] : -2;  // a lane behind the chunk belongs to no segment: a search stops on it
  const uint32_t f = g < n ? flags[g] : 0u;
  int64_t a = tv;
  if (f & SDX_RT_SREP) a = reinterpret_cast<const sdx_repeat_timed_state_hdr*>(slot_of<BS>(state, bs, g))->t;
  // the first lane behind this one that is past the anchor's window or in another segment
  int lo = lane + 1, hi = 64;
#pragma unroll
  for (int it = 0; it < 7; ++it) {
    const int mid = (lo + hi) >> 1;
    const long long tm = __shfl(tv, mid & 63);
    const int sm = __shfl(sv, mid & 63);
    if (lo < hi) {
      if (sm != sv || past(tm, a, window)) hi = mid;
      else lo = mid + 1;
    }
  }
  int s = -1;
  if (f & SDX_RT_RB) {
    int64_t idx = (int64_t)(g - lane) + lo;
    if (lo >= 64) {  // behind the wave: gallop, then halve; [lo2, hi2) always holds the answer or hi2 = n
      const int64_t a0 = idx;
      int64_t lo2 = a0, hi2 = n;
      for (int64_t off = 1;; off <<= 1) {
        const int64_t p = a0 + off - 1;
        if (p >= n) break;
        if (seg[p] != sv || past(te[p], a, window)) {
          hi2 = p;
          break;
        }
        lo2 = p + 1;
      }
      while (lo2 < hi2) {
        const int64_t mid = (lo2 + hi2) >> 1;
        if (seg[mid] != sv || past(te[mid], a, window)) hi2 = mid;
        else lo2 = mid + 1;
      }
      idx = lo2;
    }
    if (idx < n && seg[idx] == sv) s = (int)idx;
  }
  if (g < n) succ[g] = s;
  // pointer doubling inside the tile: after round r, L = the line 2^r - 1 hops on (or the orbit's last
  // line in the tile), J = the line 2^r hops on (T: it left the tile or ended)
  sg[tid] = s;
  J[tid] = (s >= 0 && s < base + T) ? s - base : T;
  L[tid] = tid;
#pragma unroll 1
  for (int r = 0; r < 8; ++r) {
    __syncthreads();
    const int j = J[tid];
    const int nj = j < T ? J[j] : T;
    const int nl = j < T ? L[j] : L[tid];
    __syncthreads();
    J[tid] = nj;
    L[tid] = nl;
  }
  __syncthreads();
  if (g < n) {
    const int l = L[tid];
    lastv[g] = base + l;
    exitv[g] = sg[l];
  }
}

template <bool BS>
__global__ __launch_bounds__(ST) void k_rept_chain(Kinds in, int n, int nt, const sdx_repeat_key* __restrict__ keys,
                                                   const int32_t* __restrict__ head,
                                                   const int32_t* __restrict__ tile_head,
                                                   const int32_t* __restrict__ exitv, const int32_t* __restrict__ lastv,
                                                   const int64_t* __restrict__ te, const uint8_t* __restrict__ flags,
                                                   int32_t* __restrict__ tile_arr, uint8_t* __restrict__ state) {
  const int last_head = head[1];
  sdx_repeat_timed_state_hdr* sh = reinterpret_cast<sdx_repeat_timed_state_hdr*>(state);
  for (int b = threadIdx.x; b < nt; b += ST) {
    const int h = tile_head[b];
    if (h < 0) continue;
    int x = h;  // only a tile's last head can have an orbit that leaves the tile
    for (int it = 0; it < nt; ++it) {
      const int e = exitv[x];
      if (e < 0 || e >= n) break;
      tile_arr[e / T] = e;
      x = e;
    }
    if (!BS && h == last_head) {  // T: the last published line; it stays when the carried anchor covers them all
      const int l = lastv[x];
      if (!(l == h && (flags[h] & SDX_RT_SREP))) sh->t = te[l];
    }
  }
  if constexpr (BS) return;  // the sources' slots: k_reps_state
  const int last = head[0];
  if (last < 0) return;  // no result-bearing line in this chunk: the state stays
  const uint4 v = *reinterpret_cast<const uint4*>(keys + last);
  if (threadIdx.x == 0) {
    sh->valid = 1;
    sh->kind = v.x;
    sh->proto = v.y;
    sh->len = v.z;
  }
  const uint8_t* src = in.k[v.x].heap + v.w;
  uint8_t* dst = state + sizeof(sdx_repeat_timed_state_hdr);
  for (uint32_t i = threadIdx.x; i < v.z; i += ST) dst[i] = src[i];
}

template <bool BS>
__global__ __launch_bounds__(T) void k_rept_mark(int n, const int32_t* __restrict__ succ,
                                                 const uint8_t* __restrict__ flags, const int32_t* __restrict__ tile_arr,
                                                 uint8_t* __restrict__ repeat, BySrc bs) {
  __shared__ int32_t J[T];
  __shared__ uint8_t on[T];
  const int tid = threadIdx.x;
  const int base = blockIdx.x * T;
  const int g = base + tid;
  const int s = g < n ? succ[g] : -1;
  const uint32_t f = g < n ? flags[g] : 0u;
  J[tid] = (s >= 0 && s < base + T) ? s - base : T;
  on[tid] = 0;
  __syncthreads();
  if ((f & SDX_RT_HEAD) || g == tile_arr[blockIdx.x]) {
    int x = tid;
    for (int it = 0; it < T && x < T; ++it) {
      on[x] = 1;
      x = J[x];
    }
  }
  __syncthreads();
  if (g < n) {
    const uint8_t r = (f & SDX_RT_RB) ? ((on[tid] && !(f & SDX_RT_SREP)) ? 0 : 1) : 0;
    if constexpr (BS) {
      const uint32_t line = (uint32_t)bs.perm[g];  // a permutation of [0, n): every entry is written
      if (line < (uint32_t)n) repeat[line] = r;
    } else {
      repeat[g] = r;
    }
  }
}

}  // namespace sdxt

// ---- sdx_mark_repeats_by_source: one (K, T) per source id ---------------------------
// The lines are sorted by source id, stable, so that every source's lines stand together in stream
// order; the timed passes above then run over positions with BS = true: a source's first result-bearing
// line takes its predecessor from the source's own slot and is always a segment head.  Without times
// every time is 0 and W = 0: no gap ever exceeds the window, which is the untimed definition.
//   k_rep_keys     keys by line, as above
//   k_reps_ids     sort key = the id (an id outside [0, S) sorts as S - 1 and its line loses its key);
//                  the run table is cleared
//   k_reps_hist, k_reps_scan, k_reps_scatter   one 8-bit LSD radix pass (two for S > 256) over tiles of
//                  256 lines: digit counts per tile, their prefix over the tiles (a wave per digit), the
//                  stable scatter.  No look-back, no global atomics (the scheme of sdx_group.hip's sort).
//   k_reps_gather  keys, times and ids by position; every source's run [lo, hi); the tiles' last
//                  result-bearing positions
//   k_rep_tiles, k_rept_heads<1>, k_rep_tiles, k_rept_seg, k_rept_succ<1>, k_rept_chain<1>
//   k_rept_mark<1> writes the mask back in line order
//   k_reps_state   a wave per source: K from the run's last result-bearing line, T from its last head's
//                  orbit end, the payload copied by the wave; the source's entry of the compact table
namespace sdxs {
using sdxt::BySrc;

__global__ __launch_bounds__(T) void k_reps_ids(int n, int S, const int32_t* __restrict__ source,
                                                uint32_t* __restrict__ skey, int32_t* __restrict__ run_lo,
                                                int32_t* __restrict__ run_hi) {
  const int g = blockIdx.x * T + threadIdx.x;
  if (g < n) {
    const uint32_t s = (uint32_t)source[g];
    skey[g] = s < (uint32_t)S ? s : (uint32_t)S - 1u;
  }
  if (g < S) run_lo[g] = run_hi[g] = 0;
}

__global__ __launch_bounds__(T) void k_reps_hist(const uint32_t* __restrict__ kin, int n, int nt, int d,
                                                 uint32_t* __restrict__ hist) {
  __shared__ uint32_t c[256];
  const int g = blockIdx.x * T + threadIdx.x;
  c[threadIdx.x] = 0;
  __syncthreads();
  if (g < n) atomicAdd(&c[(kin[g] >> (8 * d)) & 255u], 1u);  // LDS
  __syncthreads();
  hist[(size_t)threadIdx.x * nt + blockIdx.x] = c[threadIdx.x];
}

// each digit's row: exclusive prefix over the tiles (one wave per row); tot[digit] = the row's total
__global__ __launch_bounds__(T) void k_reps_scan(uint32_t* __restrict__ hist, int nt, uint32_t* __restrict__ tot) {
  const int row = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  uint32_t* h = hist + (size_t)row * nt;
  uint32_t run = 0;
  for (int b0 = 0; b0 < nt; b0 += 64) {
    const int x = b0 + lane;
    const uint32_t v = x < nt ? h[x] : 0u;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(incl, o);
      if (lane >= o) incl += y;
    }
    if (x < nt) h[x] = run + incl - v;
    run += __shfl(incl, 63);
  }
  if (lane == 0) tot[row] = run;
}

// a tile's lines go, in order, to (prefix of the digit totals) + (the tile's row offset) + (rank in the tile)
__global__ __launch_bounds__(T) void k_reps_scatter(const uint32_t* __restrict__ kin, const int32_t* __restrict__ vin,
                                                    int n, int nt, int d, const uint32_t* __restrict__ hist,
                                                    const uint32_t* __restrict__ tot, uint32_t* __restrict__ kout,
                                                    int32_t* __restrict__ vout) {
  __shared__ uint32_t run[256];
  __shared__ uint32_t wc[WAVES][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x * T + tid;
  const uint32_t t = tot[tid];
  run[tid] = t;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) wc[w][tid] = 0;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {  // inclusive scan of the digit totals
    const uint32_t y = tid >= o ? run[tid - o] : 0u;
    __syncthreads();
    run[tid] += y;
    __syncthreads();
  }
  const uint32_t base = run[tid] - t + hist[(size_t)tid * nt + blockIdx.x];
  __syncthreads();
  run[tid] = base;
  const bool valid = g < n;
  const uint32_t k = valid ? kin[g] : 0u;
  const uint32_t dig = (k >> (8 * d)) & 255u;
  uint64_t peers = __ballot(valid);  // the wave's lanes with this lane's digit
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const uint64_t bal = __ballot((dig >> b) & 1u);
    peers &= ((dig >> b) & 1u) ? bal : ~bal;
  }
  if (valid && lane == __ffsll((unsigned long long)peers) - 1) wc[wave][dig] = (uint32_t)__popcll(peers);
  __syncthreads();
  if (valid) {
    uint32_t pos = run[dig] + (uint32_t)__popcll(lane ? peers & (~0ull >> (64 - lane)) : 0ull);
    for (int w = 0; w < wave; ++w) pos += wc[w][dig];
    if (pos < (uint32_t)n) {  // always, the counts sum to n
      kout[pos] = k;
      vout[pos] = vin ? vin[g] : g;
    }
  }
}

__global__ __launch_bounds__(T) void k_reps_gather(int n, int S, const int32_t* __restrict__ perm,
                                                   const uint32_t* __restrict__ psrc, const int32_t* __restrict__ source,
                                                   const sdx_repeat_key* __restrict__ lkeys,
                                                   const int64_t* __restrict__ times, sdx_repeat_key* __restrict__ keys,
                                                   int64_t* __restrict__ ptimes, int32_t* __restrict__ run_lo,
                                                   int32_t* __restrict__ run_hi, int32_t* __restrict__ tile_last) {
  __shared__ int32_t wlast[WAVES];
  const int g = blockIdx.x * T + threadIdx.x;
  bool have = false;
  if (g < n) {
    const uint32_t line = (uint32_t)perm[g];
    uint4 v = make_uint4(SDX_REPEAT_NONE, 0, 0, 0);
    int64_t t = 0;
    if (line < (uint32_t)n) {
      if ((uint32_t)source[line] < (uint32_t)S) v = *reinterpret_cast<const uint4*>(lkeys + line);
      if (times) t = times[line];
    }
    *reinterpret_cast<uint4*>(keys + g) = v;
    ptimes[g] = t;
    have = v.x != SDX_REPEAT_NONE;
    const uint32_t s = psrc[g];
    if (s < (uint32_t)S) {
      if (g == 0 || psrc[g - 1] != s) run_lo[s] = g;
      if (g == n - 1 || psrc[g + 1] != s) run_hi[s] = g + 1;
    }
  }
  const uint64_t m = __ballot(have);
  if ((threadIdx.x & 63) == 0) wlast[threadIdx.x >> 6] = m ? (int)(g - (threadIdx.x & 63) + last_bit(m)) : -1;
  __syncthreads();
  if (threadIdx.x == 0) {
    int last = -1;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) last = max(last, wlast[w]);
    tile_last[blockIdx.x] = last;
  }
}

__global__ __launch_bounds__(T) void k_reps_state(Kinds in, int n, int nt, int S, const sdx_repeat_key* __restrict__ keys,
                                                  const int32_t* __restrict__ run_lo, const int32_t* __restrict__ run_hi,
                                                  const int32_t* __restrict__ ipred, const int32_t* __restrict__ seg,
                                                  const int32_t* __restrict__ exitv, const int32_t* __restrict__ lastv,
                                                  const int64_t* __restrict__ te, const uint8_t* __restrict__ flags,
                                                  const int32_t* __restrict__ perm, uint8_t* __restrict__ state,
                                                  sdx_repeat_source_entry* __restrict__ table) {
  const int s = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= S) return;
  uint8_t* slot = state + (size_t)s * SDX_REPEAT_TIMED_STATE_SIZE;
  sdx_repeat_timed_state_hdr h = *reinterpret_cast<const sdx_repeat_timed_state_hdr*>(slot);
  const int lo = run_lo[s], hi = run_hi[s];
  int last = -1;
  if (lo >= 0 && lo < hi && hi <= n) {
    last = ipred[hi - 1];
    if (last < lo || last >= hi) last = -1;
  }
  int line = -1;
  if (last >= 0) {  // the source has a result-bearing line in this chunk
    const uint4 v = *reinterpret_cast<const uint4*>(keys + last);
    h.valid = 1;
    h.kind = v.x;
    h.proto = v.y;
    h.len = v.z;
    const int hd = seg[hi - 1];  // the run's last head: its first result-bearing line is one
    if (hd >= lo && hd < hi) {
      int x = hd;  // an orbit that leaves its tile is followed from tile to tile, as k_rept_chain does
      for (int it = 0; it < nt; ++it) {
        const int e = exitv[x];
        if (e < 0 || e >= n) break;
        x = e;
      }
      const int l = lastv[x];
      if (l >= 0 && l < n && !(l == hd && (flags[hd] & SDX_RT_SREP))) h.t = te[l];
    }
    const uint32_t pl = (uint32_t)perm[last];
    line = pl < (uint32_t)n ? (int)pl : -1;
    if (v.x <= (uint32_t)SDX_KIND_MN && in.k[v.x].heap) {
      const uint8_t* src = in.k[v.x].heap + v.w;
      uint8_t* dst = slot + sizeof(sdx_repeat_timed_state_hdr);
      for (uint32_t i = lane; i < v.z; i += 64) dst[i] = src[i];
    }
    if (lane == 0) *reinterpret_cast<sdx_repeat_timed_state_hdr*>(slot) = h;
  }
  if (lane == 0) table[s] = sdx_repeat_source_entry{h.valid, h.kind, h.proto, h.len, h.t, line, 0};
}

}  // namespace sdxs
}  // namespace sdxr

extern "C" size_t sdx_repeat_sources_state_bytes(int32_t n_sources) { return sdx_repeat_sources_state_size(n_sources); }
extern "C" size_t sdx_repeat_sources_scratch_bytes(int32_t n, int32_t n_sources) {
  return sdx_repeat_sources_scratch_size(n, n_sources);
}

extern "C" int sdx_mark_repeats_by_source(const sdx_bank* bank, const sdx_json_in* kinds, int k, int32_t n,
                                          const int32_t* source_dev, int32_t n_sources, const int64_t* times_dev,
                                          int64_t window_us, uint8_t* repeat_dev, void* scratch_dev, void* state_dev,
                                          void* hip_stream) {
  namespace sdxt = sdxr::sdxt;
  namespace sdxs = sdxr::sdxs;
  (void)bank;
  if (!kinds || k < 1 || k > 4) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_by_source: 1 to 4 kinds");
  if (n < 0) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_by_source: n < 0");
  if (!sdx_rs_sources_ok(n_sources))
    return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_by_source: n_sources must be 1 .. SDX_REPEAT_SOURCES_MAX");
  if (times_dev && window_us < 0) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_by_source: window_us < 0");
  if (!source_dev || !repeat_dev || !scratch_dev || !state_dev)
    return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_by_source: null buffer");
  if ((((uintptr_t)scratch_dev | (uintptr_t)state_dev) & 15) || ((uintptr_t)times_dev & 7) || ((uintptr_t)source_dev & 3))
    return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_by_source: scratch_dev and state_dev must be 16-byte, "
                                      "times_dev 8-byte, source_dev 4-byte aligned");
  sdxr::Kinds in{};
  for (int i = 0; i < k; ++i) {
    const sdx_json_in& j = kinds[i];
    if (j.kind < SDX_KIND_MU || j.kind > SDX_KIND_MN)
      return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_by_source: bad kind");
    if (in.k[j.kind].desc) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_by_source: a kind given twice");
    if (!j.desc_dev || !j.rec_dev || !j.heap_dev)
      return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_by_source: null buffer");
    if (j.n != n) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_by_source: every kind's n must be the chunk's n");
    in.k[j.kind] = sdxr::KindIn{j.desc_dev, j.rec_dev, j.heap_dev};
  }
  if (n == 0) return SDX_OK;
  const int S = n_sources;
  const int64_t window = times_dev ? window_us : 0;
  uint8_t* s = static_cast<uint8_t*>(scratch_dev);
  auto part = [&](int p) { return s + sdx_rs_off(n, S, p); };
  int32_t* head = reinterpret_cast<int32_t*>(part(SDX_RS_HEAD));
  sdx_repeat_source_entry* table = reinterpret_cast<sdx_repeat_source_entry*>(part(SDX_RS_TABLE));
  int32_t* run_lo = reinterpret_cast<int32_t*>(part(SDX_RS_RUN_LO));
  int32_t* run_hi = reinterpret_cast<int32_t*>(part(SDX_RS_RUN_HI));
  sdx_repeat_key* lkeys = reinterpret_cast<sdx_repeat_key*>(part(SDX_RS_LKEYS));
  sdx_repeat_key* keys = reinterpret_cast<sdx_repeat_key*>(part(SDX_RS_KEYS));
  int64_t* te = reinterpret_cast<int64_t*>(part(SDX_RS_TE));
  int64_t* ptimes = reinterpret_cast<int64_t*>(part(SDX_RS_PTIMES));
  int32_t* seg = reinterpret_cast<int32_t*>(part(SDX_RS_SEG));
  int32_t* succ = reinterpret_cast<int32_t*>(part(SDX_RS_SUCC));
  int32_t* exitv = reinterpret_cast<int32_t*>(part(SDX_RS_EXIT));
  int32_t* lastv = reinterpret_cast<int32_t*>(part(SDX_RS_LAST));
  int32_t* ipred = reinterpret_cast<int32_t*>(part(SDX_RS_IPRED));
  int32_t* perm = reinterpret_cast<int32_t*>(part(SDX_RS_PERM));
  uint32_t* k0 = reinterpret_cast<uint32_t*>(part(SDX_RS_K0));
  uint32_t* k1 = reinterpret_cast<uint32_t*>(part(SDX_RS_K1));
  int32_t* v0 = reinterpret_cast<int32_t*>(part(SDX_RS_V0));
  const int nt = (int)sdx_repeat_tiles(n);
  int32_t* tiles = reinterpret_cast<int32_t*>(part(SDX_RS_TILES));
  int32_t *tile_last = tiles, *tile_prev = tiles + nt, *tile_head = tiles + 2 * nt, *tile_prevhead = tiles + 3 * nt,
          *tile_arr = tiles + 4 * nt, *tile_spare = tiles + 5 * nt;
  uint32_t* hist = reinterpret_cast<uint32_t*>(part(SDX_RS_HIST));
  uint32_t* tot = reinterpret_cast<uint32_t*>(part(SDX_RS_TOT));
  uint8_t* flags = part(SDX_RS_FLAGS);
  uint8_t* state = static_cast<uint8_t*>(state_dev);
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid(nt), blk(sdxr::T);
  hipLaunchKernelGGL(sdxr::k_rep_keys, grid, blk, 0, st, in, (int)n, lkeys, tile_spare);
  const int gi = ((n > S ? n : S) + sdxr::T - 1) / sdxr::T;
  hipLaunchKernelGGL(sdxs::k_reps_ids, dim3(gi), blk, 0, st, (int)n, S, source_dev, k0, run_lo, run_hi);
  const int passes = sdx_rs_passes(S);
  uint32_t* psrc = k1;
  for (int d = 0; d < passes; ++d) {  // (k0, line) -> (k1, v0 or perm) -> (k0, perm)
    uint32_t *kin = d ? k1 : k0, *kout = d ? k0 : k1;
    hipLaunchKernelGGL(sdxs::k_reps_hist, grid, blk, 0, st, (const uint32_t*)kin, (int)n, nt, d, hist);
    hipLaunchKernelGGL(sdxs::k_reps_scan, dim3(256 / sdxr::WAVES), blk, 0, st, hist, nt, tot);
    hipLaunchKernelGGL(sdxs::k_reps_scatter, grid, blk, 0, st, (const uint32_t*)kin, (const int32_t*)(d ? v0 : nullptr),
                       (int)n, nt, d, (const uint32_t*)hist, (const uint32_t*)tot, kout, d == passes - 1 ? perm : v0);
    psrc = kout;
  }
  hipLaunchKernelGGL(sdxs::k_reps_gather, grid, blk, 0, st, (int)n, S, (const int32_t*)perm, (const uint32_t*)psrc,
                     source_dev, (const sdx_repeat_key*)lkeys, times_dev, keys, ptimes, run_lo, run_hi, tile_last);
  const sdxt::BySrc bs{psrc, perm, ipred, S};
  hipLaunchKernelGGL(sdxr::k_rep_tiles, dim3(1), dim3(sdxr::ST), 0, st, (const int32_t*)tile_last, nt, tile_prev, head);
  hipLaunchKernelGGL(sdxt::k_rept_heads<true>, grid, blk, 0, st, in, (int)n, (const sdx_repeat_key*)keys,
                     (const int32_t*)tile_prev, (const int64_t*)ptimes, window, (const uint8_t*)state, te, flags, tile_head,
                     tile_arr, bs);
  hipLaunchKernelGGL(sdxr::k_rep_tiles, dim3(1), dim3(sdxr::ST), 0, st, (const int32_t*)tile_head, nt, tile_prevhead,
                     head + 1);
  hipLaunchKernelGGL(sdxt::k_rept_seg, grid, blk, 0, st, (int)n, (const uint8_t*)flags, (const int32_t*)tile_prevhead, seg);
  hipLaunchKernelGGL(sdxt::k_rept_succ<true>, grid, blk, 0, st, (int)n, (const int64_t*)te, (const int32_t*)seg,
                     (const uint8_t*)flags, window, (const uint8_t*)state, succ, exitv, lastv, bs);
  hipLaunchKernelGGL(sdxt::k_rept_chain<true>, dim3(1), dim3(sdxr::ST), 0, st, in, (int)n, nt, (const sdx_repeat_key*)keys,
                     (const int32_t*)head, (const int32_t*)tile_head, (const int32_t*)exitv, (const int32_t*)lastv,
                     (const int64_t*)te, (const uint8_t*)flags, tile_arr, state);
  hipLaunchKernelGGL(sdxt::k_rept_mark<true>, grid, blk, 0, st, (int)n, (const int32_t*)succ, (const uint8_t*)flags,
                     (const int32_t*)tile_arr, repeat_dev, bs);
  hipLaunchKernelGGL(sdxs::k_reps_state, dim3((S + sdxr::WAVES - 1) / sdxr::WAVES), blk, 0, st, in, (int)n, nt, S,
                     (const sdx_repeat_key*)keys, (const int32_t*)run_lo, (const int32_t*)run_hi, (const int32_t*)ipred,
                     (const int32_t*)seg, (const int32_t*)exitv, (const int32_t*)lastv, (const int64_t*)te,
                     (const uint8_t*)flags, (const int32_t*)perm, state, table);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return sdx::set_error(SDX_EHIP, std::string("sdx_mark_repeats_by_source: ") + hipGetErrorString(e));
  return SDX_OK;
}

extern "C" size_t sdx_repeat_timed_state_bytes(void) { return sdx_repeat_timed_state_size(); }
extern "C" size_t sdx_repeat_timed_scratch_bytes(int32_t n) { return sdx_repeat_timed_scratch_size(n); }

extern "C" int sdx_mark_repeats_timed(const sdx_bank* bank, const sdx_json_in* kinds, int k, int32_t n,
                                      const int64_t* times_dev, int64_t window_us, uint8_t* repeat_dev,
                                      void* scratch_dev, void* state_dev, void* hip_stream) {
  namespace sdxt = sdxr::sdxt;
  (void)bank;
  if (!kinds || k < 1 || k > 4) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_timed: 1 to 4 kinds");
  if (n < 0) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_timed: n < 0");
  if (window_us < 0) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_timed: window_us < 0");
  if (!times_dev || !repeat_dev || !scratch_dev || !state_dev)
    return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_timed: null buffer");
  if ((((uintptr_t)scratch_dev | (uintptr_t)state_dev) & 15) || ((uintptr_t)times_dev & 7))
    return sdx::set_error(SDX_EINVAL,
                          "sdx_mark_repeats_timed: scratch_dev and state_dev must be 16-byte, times_dev 8-byte aligned");
  sdxr::Kinds in{};
  for (int i = 0; i < k; ++i) {
    const sdx_json_in& j = kinds[i];
    if (j.kind < SDX_KIND_MU || j.kind > SDX_KIND_MN)
      return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_timed: bad kind");
    if (in.k[j.kind].desc) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_timed: a kind given twice");
    if (!j.desc_dev || !j.rec_dev || !j.heap_dev)
      return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_timed: null buffer");
    if (j.n != n) return sdx::set_error(SDX_EINVAL, "sdx_mark_repeats_timed: every kind's n must be the chunk's n");
    in.k[j.kind] = sdxr::KindIn{j.desc_dev, j.rec_dev, j.heap_dev};
  }
  if (n == 0) return SDX_OK;
  uint8_t* s = static_cast<uint8_t*>(scratch_dev);
  int32_t* head = reinterpret_cast<int32_t*>(s);
  sdx_repeat_key* keys = reinterpret_cast<sdx_repeat_key*>(s + sdx_rt_keys_off());
  int64_t* te = reinterpret_cast<int64_t*>(s + sdx_rt_te_off(n));
  int32_t* seg = reinterpret_cast<int32_t*>(s + sdx_rt_seg_off(n));
  int32_t* succ = reinterpret_cast<int32_t*>(s + sdx_rt_succ_off(n));
  int32_t* exitv = reinterpret_cast<int32_t*>(s + sdx_rt_exit_off(n));
  int32_t* lastv = reinterpret_cast<int32_t*>(s + sdx_rt_last_off(n));
  int32_t* tile_last = reinterpret_cast<int32_t*>(s + sdx_rt_tile_off(n, 0));
  int32_t* tile_prev = reinterpret_cast<int32_t*>(s + sdx_rt_tile_off(n, 1));
  int32_t* tile_head = reinterpret_cast<int32_t*>(s + sdx_rt_tile_off(n, 2));
  int32_t* tile_prevhead = reinterpret_cast<int32_t*>(s + sdx_rt_tile_off(n, 3));
  int32_t* tile_arr = reinterpret_cast<int32_t*>(s + sdx_rt_tile_off(n, 4));
  uint8_t* flags = s + sdx_rt_flags_off(n);
  uint8_t* state = static_cast<uint8_t*>(state_dev);
  const int nt = (int)sdx_repeat_tiles(n);
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(sdxr::k_rep_keys, dim3(nt), dim3(sdxr::T), 0, st, in, (int)n, keys, tile_last);
  hipLaunchKernelGGL(sdxr::k_rep_tiles, dim3(1), dim3(sdxr::ST), 0, st, (const int32_t*)tile_last, nt, tile_prev, head);
  hipLaunchKernelGGL(sdxt::k_rept_heads<false>, dim3(nt), dim3(sdxr::T), 0, st, in, (int)n, (const sdx_repeat_key*)keys,
                     (const int32_t*)tile_prev, times_dev, window_us, (const uint8_t*)state, te, flags, tile_head,
                     tile_arr, sdxt::BySrc{});
  hipLaunchKernelGGL(sdxr::k_rep_tiles, dim3(1), dim3(sdxr::ST), 0, st, (const int32_t*)tile_head, nt, tile_prevhead,
                     head + 1);
  hipLaunchKernelGGL(sdxt::k_rept_seg, dim3(nt), dim3(sdxr::T), 0, st, (int)n, (const uint8_t*)flags,
                     (const int32_t*)tile_prevhead, seg);
  hipLaunchKernelGGL(sdxt::k_rept_succ<false>, dim3(nt), dim3(sdxr::T), 0, st, (int)n, (const int64_t*)te, (const int32_t*)seg,
                     (const uint8_t*)flags, window_us, (const uint8_t*)state, succ, exitv, lastv, sdxt::BySrc{});
  hipLaunchKernelGGL(sdxt::k_rept_chain<false>, dim3(1), dim3(sdxr::ST), 0, st, in, (int)n, nt, (const sdx_repeat_key*)keys,
                     (const int32_t*)head, (const int32_t*)tile_head, (const int32_t*)exitv, (const int32_t*)lastv,
                     (const int64_t*)te, (const uint8_t*)flags, tile_arr, state);
  hipLaunchKernelGGL(sdxt::k_rept_mark<false>, dim3(nt), dim3(sdxr::T), 0, st, (int)n, (const int32_t*)succ,
                     (const uint8_t*)flags, (const int32_t*)tile_arr, repeat_dev, sdxt::BySrc{});
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return sdx::set_error(SDX_EHIP, std::string("sdx_mark_repeats_timed: ") + hipGetErrorString(e));
  return SDX_OK;
}

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
