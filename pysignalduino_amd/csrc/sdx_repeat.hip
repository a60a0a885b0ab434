// sdx_repeat.hip -- repeat suppression (sdx_mark_repeats), hand-written HIP for gfx950.
//
// A stick delivers every telegram several times, each repetition as its own firmware line.  A
// result-bearing line (k_json's condition: descriptor OK with n_rec > 0 in its kind's launch) is a
// REPEAT when (kind, proto index, payload bytes) of its first result equal those of the previous
// result-bearing line of the stream; lines without results neither start nor break a run.
//
// The file in the order it is written:
//   helpers   what the kernels share: a key as one 16-byte load, "the last set line of the wave / of the
//             tile" from a ballot, the predecessor lookup over (ballot, the tile's waves, the tile table),
//             key equality, K + payload into a state, an orbit followed over the tiles' exits
//   kernels   k_rep_* (sdx_mark_repeats), k_rept_* (the timed passes; BS: over positions sorted by source),
//             k_reps_* (ids, radix sort, gather, the sources' slots), each group under its own comment
//   host      parse_kinds (the kinds' validation), TimedBufs + launch_timed<BS> (the seven timed launches)
//   entries   three compositions of those launches on the caller's stream, no look-back and no spinning (as
//             sdx_split.hip): sdx_mark_repeats; sdx_mark_repeats_timed = k_rep_keys + launch_timed<false>;
//             sdx_mark_repeats_by_source = keys, ids, sort, gather + launch_timed<true> + k_reps_state
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

// ---- helpers shared by the kernels (T threads = WAVES waves per tile, lane = line or position) --------
__device__ __forceinline__ int last_bit(uint64_t m) { return 63 - __builtin_clzll(m); }  // m != 0

// a key as one 16-byte load: x = kind, y = proto, z = len, w = off
__device__ __forceinline__ uint4 load_key(const sdx_repeat_key* key) { return *reinterpret_cast<const uint4*>(key); }
// line g's key, SDX_REPEAT_NONE behind the chunk
__device__ __forceinline__ sdx_repeat_key key_at(const sdx_repeat_key* keys, int g, int n) {
  if (g >= n) return sdx_repeat_key{SDX_REPEAT_NONE, 0, 0, 0};
  const uint4 v = load_key(keys + g);
  return sdx_repeat_key{v.x, v.y, v.z, v.w};
}

// The wave's ballot of ``set``; its last set line (-1 = none) goes to wlast[wave].  Every thread of the
// tile calls it; the table is read behind a __syncthreads() (pred_of, tile_last_out).
__device__ __forceinline__ uint64_t wave_last(bool set, int g, int32_t* wlast) {
  const uint64_t m = __ballot(set);
  const int lane = threadIdx.x & 63;
  if (lane == 0) wlast[threadIdx.x >> 6] = m ? (int)(g - lane + last_bit(m)) : -1;
  return m;
}
// thread 0: the tile's last set line = the maximum over the waves' -> out[tile]
__device__ __forceinline__ void tile_last_out(const int32_t* wlast, int32_t* __restrict__ out) {
  if (threadIdx.x == 0) {
    int last = -1;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) last = max(last, wlast[w]);
    out[blockIdx.x] = last;
  }
}
// The last set line in front of line g (INCL: at or in front of it), -1 = none: from the wave's ballot m,
// else the tile's earlier waves (wlast), else the table of what stands in front of every tile.
template <bool INCL>
__device__ __forceinline__ int pred_of(uint64_t m, int g, const int32_t* wlast, const int32_t* __restrict__ before) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t lower = INCL ? m & (~0ull >> (63 - lane)) : lane ? m & (~0ull >> (64 - lane)) : 0ull;
  if (lower) return g - lane + last_bit(lower);
  int p = -1;
  for (int w = wave - 1; w >= 0 && p < 0; --w) p = wlast[w];
  if (p < 0) p = before[blockIdx.x];
  return p;
}

__device__ __forceinline__ bool same_bytes(const uint8_t* a, const uint8_t* b, uint32_t len) {
  for (uint32_t i = 0; i < len; ++i)
    if (a[i] != b[i]) return false;
  return true;
}
// key (its payload at ``mine``) against another line's or a state's (kind, proto, len, payload)
__device__ __forceinline__ bool same_key(const sdx_repeat_key& key, const uint8_t* mine, uint32_t kind, uint32_t proto,
                                         uint32_t len, const uint8_t* theirs) {
  return kind == key.kind && proto == key.proto && len == key.len && same_bytes(mine, theirs, key.len);
}

// K of a state: the header's fields (either layout's header begins valid, kind, proto, len) ...
template <class HDR>
__device__ __forceinline__ void set_key(HDR& h, const uint4& v) {
  h.valid = 1;
  h.kind = v.x;
  h.proto = v.y;
  h.len = v.z;
}
// ... and the payload behind it, by the caller's threads tid, tid + stride, ...
__device__ __forceinline__ void copy_payload(const Kinds& in, const uint4& v, uint8_t* dst, uint32_t tid, uint32_t stride) {
  const uint8_t* src = in.k[v.x].heap + v.w;
  for (uint32_t i = tid; i < v.z; i += stride) dst[i] = src[i];
}

// An orbit that leaves its tile is followed from tile to tile over the exits, at most nt of them -> its
// line in the last tile it reaches.  ARR: every line it lands on is entered into its tile's tile_arr.
template <bool ARR>
__device__ __forceinline__ int follow_exits(int x, int n, int nt, const int32_t* __restrict__ exitv, int32_t* tile_arr) {
  for (int it = 0; it < nt; ++it) {
    const int e = exitv[x];
    if (e < 0 || e >= n) break;
    if constexpr (ARR) tile_arr[e / T] = e;
    x = e;
  }
  return x;
}

// ---- sdx_mark_repeats' kernels ----------------------------------------------------------------------
//   k_rep_keys     lane = line: the kinds' descriptors -> one 16-byte key per line, and per tile of
//                  SDX_REPEAT_TILE lines its last result-bearing line
//   k_rep_tiles    one workgroup: the last result-bearing line in front of every tile, and the chunk's last
//   k_rep_resolve  lane = line: the predecessor (pred_of) or the carried state; same_key
//   k_rep_state    one workgroup: key + payload of the chunk's last result-bearing line -> state
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
  wave_last(key.kind != SDX_REPEAT_NONE, g, wlast);
  __syncthreads();
  tile_last_out(wlast, tile_last);
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

__global__ __launch_bounds__(T) void k_rep_resolve(Kinds in, int n, const sdx_repeat_key* __restrict__ keys,
                                                   const int32_t* __restrict__ tile_prev,
                                                   const uint8_t* __restrict__ state, uint8_t* __restrict__ repeat) {
  __shared__ int32_t wlast[WAVES];
  const int g = blockIdx.x * T + threadIdx.x;
  const sdx_repeat_key key = key_at(keys, g, n);
  const bool have = key.kind != SDX_REPEAT_NONE;
  const uint64_t m = wave_last(have, g, wlast);
  __syncthreads();
  if (g >= n) return;
  if (!have) {
    repeat[g] = 0;
    return;
  }
  const int pred = pred_of<false>(m, g, wlast, tile_prev);
  const uint8_t* mine = in.k[key.kind].heap + key.off;
  bool eq;
  if (pred >= 0) {
    const uint4 v = load_key(keys + pred);
    eq = same_key(key, mine, v.x, v.y, v.z, in.k[key.kind].heap + v.w);
  } else {  // no earlier result-bearing line in this chunk: the carried state
    const sdx_repeat_state_hdr h = *reinterpret_cast<const sdx_repeat_state_hdr*>(state);
    eq = h.valid && same_key(key, mine, h.kind, h.proto, h.len, state + sizeof(sdx_repeat_state_hdr));
  }
  repeat[g] = eq ? 1 : 0;
}

__global__ __launch_bounds__(T) void k_rep_state(Kinds in, const sdx_repeat_key* __restrict__ keys,
                                                 const int32_t* __restrict__ head, uint8_t* __restrict__ state) {
  const int last = head[0];
  if (last < 0) return;  // no result-bearing line in this chunk: the state stays
  const uint4 v = load_key(keys + last);
  if (threadIdx.x == 0) set_key(*reinterpret_cast<sdx_repeat_state_hdr*>(state), v);
  copy_payload(in, v, state + sizeof(sdx_repeat_state_hdr), threadIdx.x, T);
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
// Behind k_rep_keys, seven launches (launch_timed):
//   k_rep_tiles    the last result-bearing line in front of every tile, as in sdx_mark_repeats
//   k_rept_heads   lane = line: predecessor as k_rep_resolve, key compare and gap -> flags, te (a line
//                  without results takes its predecessor's time, so te is non-decreasing and a search
//                  never stops on such a line), the tile's last head
//   k_rep_tiles    over the tiles' last heads -> the last head in front of every tile
//   k_rept_seg     lane = line: the line's segment head
//   k_rept_succ    lane = line: succ by binary search, inside the wave over the lanes' registers
//                  (shuffles), behind it galloping over te / seg in memory; then pointer doubling over
//                  the tile (LDS, 8 rounds): the orbit's last line inside the tile and its first behind it
//   k_rept_chain   one workgroup, thread = tile: an orbit that leaves its head's tile is followed from
//                  tile to tile (follow_exits: one load per tile it enters; orbits of different segments in
//                  parallel) and entered into the tiles it lands in; then the state: K as k_rep_state, T =
//                  the time of the last line of the last head's orbit
//   k_rept_mark    lane = line: the tile's heads and its entry walk their orbit inside the tile (LDS)
// Every search and walk is bounded by indices: on times that decrease the mask is unspecified, but
// nothing leaves its buffer and every loop ends.
namespace sdxt {

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
  const int g = blockIdx.x * T + threadIdx.x;
  const sdx_repeat_key key = key_at(keys, g, n);
  const bool have = key.kind != SDX_REPEAT_NONE;
  const uint64_t m = wave_last(have, g, wlast);
  __syncthreads();
  uint32_t f = 0;
  if (g < n) {
    const int pred = pred_of<false>(m, g, wlast, tile_prev);
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
        const uint4 v = load_key(keys + pred);
        const bool cont = !past(t, times[pred], window) && same_key(key, mine, v.x, v.y, v.z, in.k[key.kind].heap + v.w);
        if (!cont) f |= SDX_RT_HEAD;
      } else {  // the chunk's first result-bearing line: the carried (K, T)
        const uint8_t* slot = slot_of<BS>(state, bs, g);
        const sdx_repeat_timed_state_hdr h = *reinterpret_cast<const sdx_repeat_timed_state_hdr*>(slot);
        f |= SDX_RT_HEAD;
        if (h.valid && !past(t, h.t, window) &&
            same_key(key, mine, h.kind, h.proto, h.len, slot + sizeof(sdx_repeat_timed_state_hdr)))
          f |= SDX_RT_SREP;
      }
    } else if (pred >= 0) {
      t = times[pred];
    }
    te[g] = t;
    flags[g] = (uint8_t)f;
  }
  wave_last((f & SDX_RT_HEAD) != 0, g, whead);
  __syncthreads();
  tile_last_out(whead, tile_head);
  if (threadIdx.x == 0) tile_arr[blockIdx.x] = -1;
}

__global__ __launch_bounds__(T) void k_rept_seg(int n, const uint8_t* __restrict__ flags,
                                                const int32_t* __restrict__ tile_prevhead, int32_t* __restrict__ seg) {
  __shared__ int32_t whead[WAVES];
  const int g = blockIdx.x * T + threadIdx.x;
  const uint64_t hm = wave_last(g < n && (flags[g] & SDX_RT_HEAD), g, whead);
  __syncthreads();
  if (g >= n) return;
  seg[g] = pred_of<true>(hm, g, whead, tile_prevhead);
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
    // only a tile's last head can have an orbit that leaves the tile
    const int x = follow_exits<true>(h, n, nt, exitv, tile_arr);
    if (!BS && h == last_head) {  // T: the last published line; it stays when the carried anchor covers them all
      const int l = lastv[x];
      if (!(l == h && (flags[h] & SDX_RT_SREP))) sh->t = te[l];
    }
  }
  if constexpr (BS) return;  // the sources' slots: k_reps_state
  const int last = head[0];
  if (last < 0) return;  // no result-bearing line in this chunk: the state stays
  const uint4 v = load_key(keys + last);
  if (threadIdx.x == 0) set_key(*sh, v);
  copy_payload(in, v, state + sizeof(sdx_repeat_timed_state_hdr), threadIdx.x, ST);
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
//   launch_timed<true>   over positions; k_rept_mark<1> writes the mask back in line order
//   k_reps_state   a wave per source: K from the run's last result-bearing line, T from its last head's
//                  orbit end (follow_exits), the payload copied by the wave; the source's entry of the
//                  compact table.  Its range checks on what it reads from the scratch are its own.
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
      if ((uint32_t)source[line] < (uint32_t)S) v = load_key(lkeys + line);
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
  wave_last(have, g, wlast);
  __syncthreads();
  tile_last_out(wlast, tile_last);
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
    const uint4 v = load_key(keys + last);
    set_key(h, v);
    const int hd = seg[hi - 1];  // the run's last head: its first result-bearing line is one
    if (hd >= lo && hd < hi) {
      const int l = lastv[follow_exits<false>(hd, n, nt, exitv, nullptr)];  // as k_rept_chain follows it
      if (l >= 0 && l < n && !(l == hd && (flags[hd] & SDX_RT_SREP))) h.t = te[l];
    }
    const uint32_t pl = (uint32_t)perm[last];
    line = pl < (uint32_t)n ? (int)pl : -1;
    if (v.x <= (uint32_t)SDX_KIND_MN && in.k[v.x].heap)
      copy_payload(in, v, slot + sizeof(sdx_repeat_timed_state_hdr), lane, 64);
    if (lane == 0) *reinterpret_cast<sdx_repeat_timed_state_hdr*>(slot) = h;
  }
  if (lane == 0) table[s] = sdx_repeat_source_entry{h.valid, h.kind, h.proto, h.len, h.t, line, 0};
}

}  // namespace sdxs

// ---- host: what the three entries share ----------------------------------------------------------------
static int bad_arg(const char* fn, const char* what) { return sdx::set_error(SDX_EINVAL, std::string(fn) + ": " + what); }

// the checks every entry begins with; parse_kinds relies on them
static int check_counts(const char* fn, const sdx_json_in* kinds, int k, int32_t n) {
  if (!kinds || k < 1 || k > 4) return bad_arg(fn, "1 to 4 kinds");
  if (n < 0) return bad_arg(fn, "n < 0");
  return SDX_OK;
}
// kinds[0 .. k) -> in, every kind at most once, with all three buffers and the chunk's n
static int parse_kinds(const char* fn, const sdx_json_in* kinds, int k, int32_t n, Kinds& in) {
  in = Kinds{};
  for (int i = 0; i < k; ++i) {
    const sdx_json_in& j = kinds[i];
    if (j.kind < SDX_KIND_MU || j.kind > SDX_KIND_MN) return bad_arg(fn, "bad kind");
    if (in.k[j.kind].desc) return bad_arg(fn, "a kind given twice");
    if (!j.desc_dev || !j.rec_dev || !j.heap_dev) return bad_arg(fn, "null buffer");
    if (j.n != n) return bad_arg(fn, "every kind's n must be the chunk's n");
    in.k[j.kind] = KindIn{j.desc_dev, j.rec_dev, j.heap_dev};
  }
  return SDX_OK;
}
static int launched(const char* fn) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? SDX_OK : sdx::set_error(SDX_EHIP, std::string(fn) + ": " + hipGetErrorString(e));
}

// the arrays of the timed passes inside a scratch buffer: by line in sdx_mark_repeats_timed's, by position
// in sdx_mark_repeats_by_source's (sdx_repeat_layout.h)
struct TimedBufs {
  int32_t* head;
  sdx_repeat_key* keys;
  int64_t* te;
  int32_t *seg, *succ, *exitv, *lastv;
  int32_t *tile_last, *tile_prev, *tile_head, *tile_prevhead, *tile_arr;
  uint8_t* flags;
};
template <class X>
static X* at(uint8_t* s, size_t off) {
  return reinterpret_cast<X*>(s + off);
}
static TimedBufs timed_bufs(uint8_t* s, int32_t n) {
  auto tile = [&](int t) { return at<int32_t>(s, sdx_rt_tile_off(n, t)); };
  return TimedBufs{at<int32_t>(s, 0), at<sdx_repeat_key>(s, sdx_rt_keys_off()), at<int64_t>(s, sdx_rt_te_off(n)),
                   at<int32_t>(s, sdx_rt_seg_off(n)), at<int32_t>(s, sdx_rt_succ_off(n)), at<int32_t>(s, sdx_rt_exit_off(n)),
                   at<int32_t>(s, sdx_rt_last_off(n)), tile(0), tile(1), tile(2), tile(3), tile(4), s + sdx_rt_flags_off(n)};
}
template <class X>
static X* part(void* scratch, int32_t n, int S, int p) {  // a part of sdx_mark_repeats_by_source's scratch
  return at<X>(static_cast<uint8_t*>(scratch), sdx_rs_off(n, S, p));
}
static TimedBufs source_bufs(uint8_t* s, int32_t n, int S) {
  const size_t nt = (size_t)sdx_repeat_tiles(n);
  int32_t* tiles = part<int32_t>(s, n, S, SDX_RS_TILES);
  return TimedBufs{part<int32_t>(s, n, S, SDX_RS_HEAD), part<sdx_repeat_key>(s, n, S, SDX_RS_KEYS),
                   part<int64_t>(s, n, S, SDX_RS_TE), part<int32_t>(s, n, S, SDX_RS_SEG), part<int32_t>(s, n, S, SDX_RS_SUCC),
                   part<int32_t>(s, n, S, SDX_RS_EXIT), part<int32_t>(s, n, S, SDX_RS_LAST), tiles, tiles + nt,
                   tiles + 2 * nt, tiles + 3 * nt, tiles + 4 * nt, part<uint8_t>(s, n, S, SDX_RS_FLAGS)};
}

// The timed passes behind the keys (b.keys, b.tile_last are written): seven launches -> repeat and, BS =
// false, the state; BS = true leaves the sources' slots to k_reps_state.
template <bool BS>
static void launch_timed(const Kinds& in, int n, const TimedBufs& b, const int64_t* times, int64_t window, uint8_t* state,
                         uint8_t* repeat, const sdxt::BySrc& bs, hipStream_t st) {
  const int nt = (int)sdx_repeat_tiles(n);
  const dim3 grid(nt), blk(T), one(1), wide(ST);
  hipLaunchKernelGGL(k_rep_tiles, one, wide, 0, st, (const int32_t*)b.tile_last, nt, b.tile_prev, b.head);
  hipLaunchKernelGGL(sdxt::k_rept_heads<BS>, grid, blk, 0, st, in, n, (const sdx_repeat_key*)b.keys,
                     (const int32_t*)b.tile_prev, times, window, (const uint8_t*)state, b.te, b.flags, b.tile_head,
                     b.tile_arr, bs);
  hipLaunchKernelGGL(k_rep_tiles, one, wide, 0, st, (const int32_t*)b.tile_head, nt, b.tile_prevhead, b.head + 1);
  hipLaunchKernelGGL(sdxt::k_rept_seg, grid, blk, 0, st, n, (const uint8_t*)b.flags, (const int32_t*)b.tile_prevhead, b.seg);
  hipLaunchKernelGGL(sdxt::k_rept_succ<BS>, grid, blk, 0, st, n, (const int64_t*)b.te, (const int32_t*)b.seg,
                     (const uint8_t*)b.flags, window, (const uint8_t*)state, b.succ, b.exitv, b.lastv, bs);
  hipLaunchKernelGGL(sdxt::k_rept_chain<BS>, one, wide, 0, st, in, n, nt, (const sdx_repeat_key*)b.keys,
                     (const int32_t*)b.head, (const int32_t*)b.tile_head, (const int32_t*)b.exitv, (const int32_t*)b.lastv,
                     (const int64_t*)b.te, (const uint8_t*)b.flags, b.tile_arr, state);
  hipLaunchKernelGGL(sdxt::k_rept_mark<BS>, grid, blk, 0, st, n, (const int32_t*)b.succ, (const uint8_t*)b.flags,
                     (const int32_t*)b.tile_arr, repeat, bs);
}
}  // namespace sdxr

// ---- the entries ---------------------------------------------------------------------------------------
extern "C" size_t sdx_repeat_state_bytes(void) { return sdx_repeat_state_size(); }
extern "C" size_t sdx_repeat_scratch_bytes(int32_t n) { return sdx_repeat_scratch_size(n); }
extern "C" int sdx_repeat_tile(void) { return SDX_REPEAT_TILE; }

extern "C" int sdx_mark_repeats(const sdx_bank* bank, const sdx_json_in* kinds, int k, int32_t n, uint8_t* repeat_dev,
                                void* key_scratch_dev, void* state_dev, void* hip_stream) {
  using namespace sdxr;
  static const char FN[] = "sdx_mark_repeats";
  (void)bank;  // keys are table indices: no bank record is read
  Kinds in;
  if (int rc = check_counts(FN, kinds, k, n)) return rc;
  if (int rc = parse_kinds(FN, kinds, k, n, in)) return rc;
  // an empty chunk is accepted before the buffers are looked at: the other two entries check theirs first.
  // Callers may rely on either, so the asymmetry stays.
  if (n == 0) return SDX_OK;
  if (!repeat_dev || !key_scratch_dev || !state_dev) return bad_arg(FN, "null buffer");
  if (((uintptr_t)key_scratch_dev | (uintptr_t)state_dev) & 15)
    return bad_arg(FN, "key_scratch_dev and state_dev must be 16-byte aligned");
  uint8_t *s = static_cast<uint8_t*>(key_scratch_dev), *state = static_cast<uint8_t*>(state_dev);
  int32_t* head = at<int32_t>(s, 0);
  sdx_repeat_key* keys = at<sdx_repeat_key>(s, sdx_repeat_keys_off());
  int32_t* tile_last = at<int32_t>(s, sdx_repeat_tile_last_off(n));
  int32_t* tile_prev = at<int32_t>(s, sdx_repeat_tile_prev_off(n));
  const int nt = (int)sdx_repeat_tiles(n);
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(k_rep_keys, dim3(nt), dim3(T), 0, st, in, (int)n, keys, tile_last);
  hipLaunchKernelGGL(k_rep_tiles, dim3(1), dim3(ST), 0, st, (const int32_t*)tile_last, nt, tile_prev, head);
  hipLaunchKernelGGL(k_rep_resolve, dim3(nt), dim3(T), 0, st, in, (int)n, (const sdx_repeat_key*)keys,
                     (const int32_t*)tile_prev, (const uint8_t*)state, repeat_dev);
  hipLaunchKernelGGL(k_rep_state, dim3(1), dim3(T), 0, st, in, (const sdx_repeat_key*)keys, (const int32_t*)head, state);
  return launched(FN);
}

extern "C" size_t sdx_repeat_timed_state_bytes(void) { return sdx_repeat_timed_state_size(); }
extern "C" size_t sdx_repeat_timed_scratch_bytes(int32_t n) { return sdx_repeat_timed_scratch_size(n); }

extern "C" int sdx_mark_repeats_timed(const sdx_bank* bank, const sdx_json_in* kinds, int k, int32_t n,
                                      const int64_t* times_dev, int64_t window_us, uint8_t* repeat_dev,
                                      void* scratch_dev, void* state_dev, void* hip_stream) {
  using namespace sdxr;
  static const char FN[] = "sdx_mark_repeats_timed";
  (void)bank;
  Kinds in;
  if (int rc = check_counts(FN, kinds, k, n)) return rc;
  if (window_us < 0) return bad_arg(FN, "window_us < 0");
  if (!times_dev || !repeat_dev || !scratch_dev || !state_dev) return bad_arg(FN, "null buffer");
  if ((((uintptr_t)scratch_dev | (uintptr_t)state_dev) & 15) || ((uintptr_t)times_dev & 7))
    return bad_arg(FN, "scratch_dev and state_dev must be 16-byte, times_dev 8-byte aligned");
  if (int rc = parse_kinds(FN, kinds, k, n, in)) return rc;
  if (n == 0) return SDX_OK;
  const TimedBufs b = timed_bufs(static_cast<uint8_t*>(scratch_dev), n);
  hipStream_t st = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(k_rep_keys, dim3((int)sdx_repeat_tiles(n)), dim3(T), 0, st, in, (int)n, b.keys, b.tile_last);
  launch_timed<false>(in, n, b, times_dev, window_us, static_cast<uint8_t*>(state_dev), repeat_dev, sdxt::BySrc{}, st);
  return launched(FN);
}

extern "C" size_t sdx_repeat_sources_state_bytes(int32_t n_sources) { return sdx_repeat_sources_state_size(n_sources); }
extern "C" size_t sdx_repeat_sources_scratch_bytes(int32_t n, int32_t n_sources) {
  return sdx_repeat_sources_scratch_size(n, n_sources);
}

extern "C" int sdx_mark_repeats_by_source(const sdx_bank* bank, const sdx_json_in* kinds, int k, int32_t n,
                                          const int32_t* source_dev, int32_t n_sources, const int64_t* times_dev,
                                          int64_t window_us, uint8_t* repeat_dev, void* scratch_dev, void* state_dev,
                                          void* hip_stream) {
  using namespace sdxr;
  static const char FN[] = "sdx_mark_repeats_by_source";
  (void)bank;
  Kinds in;
  if (int rc = check_counts(FN, kinds, k, n)) return rc;
  if (!sdx_rs_sources_ok(n_sources)) return bad_arg(FN, "n_sources must be 1 .. SDX_REPEAT_SOURCES_MAX");
  if (times_dev && window_us < 0) return bad_arg(FN, "window_us < 0");
  if (!source_dev || !repeat_dev || !scratch_dev || !state_dev) return bad_arg(FN, "null buffer");
  if ((((uintptr_t)scratch_dev | (uintptr_t)state_dev) & 15) || ((uintptr_t)times_dev & 7) || ((uintptr_t)source_dev & 3))
    return bad_arg(FN, "scratch_dev and state_dev must be 16-byte, times_dev 8-byte, source_dev 4-byte aligned");
  if (int rc = parse_kinds(FN, kinds, k, n, in)) return rc;
  if (n == 0) return SDX_OK;
  const int S = n_sources, nt = (int)sdx_repeat_tiles(n);
  uint8_t *s = static_cast<uint8_t*>(scratch_dev), *state = static_cast<uint8_t*>(state_dev);
  const TimedBufs b = source_bufs(s, n, S);  // by position; the rest of the scratch: the sort and the runs
  int32_t *run_lo = part<int32_t>(s, n, S, SDX_RS_RUN_LO), *run_hi = part<int32_t>(s, n, S, SDX_RS_RUN_HI);
  sdx_repeat_key* lkeys = part<sdx_repeat_key>(s, n, S, SDX_RS_LKEYS);
  int64_t* ptimes = part<int64_t>(s, n, S, SDX_RS_PTIMES);
  int32_t *ipred = part<int32_t>(s, n, S, SDX_RS_IPRED), *perm = part<int32_t>(s, n, S, SDX_RS_PERM);
  uint32_t *k0 = part<uint32_t>(s, n, S, SDX_RS_K0), *k1 = part<uint32_t>(s, n, S, SDX_RS_K1);
  int32_t* v0 = part<int32_t>(s, n, S, SDX_RS_V0);
  int32_t* tile_spare = part<int32_t>(s, n, S, SDX_RS_TILES) + 5 * (size_t)nt;
  uint32_t *hist = part<uint32_t>(s, n, S, SDX_RS_HIST), *tot = part<uint32_t>(s, n, S, SDX_RS_TOT);
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid(nt), blk(T);
  hipLaunchKernelGGL(k_rep_keys, grid, blk, 0, st, in, (int)n, lkeys, tile_spare);
  const int gi = ((n > S ? n : S) + T - 1) / T;
  hipLaunchKernelGGL(sdxs::k_reps_ids, dim3(gi), blk, 0, st, (int)n, S, source_dev, k0, run_lo, run_hi);
  const int passes = sdx_rs_passes(S);
  uint32_t* psrc = k1;
  for (int d = 0; d < passes; ++d) {  // (k0, line) -> (k1, v0 or perm) -> (k0, perm)
    uint32_t *kin = d ? k1 : k0, *kout = d ? k0 : k1;
    hipLaunchKernelGGL(sdxs::k_reps_hist, grid, blk, 0, st, (const uint32_t*)kin, (int)n, nt, d, hist);
    hipLaunchKernelGGL(sdxs::k_reps_scan, dim3(256 / WAVES), blk, 0, st, hist, nt, tot);
    hipLaunchKernelGGL(sdxs::k_reps_scatter, grid, blk, 0, st, (const uint32_t*)kin, (const int32_t*)(d ? v0 : nullptr),
                       (int)n, nt, d, (const uint32_t*)hist, (const uint32_t*)tot, kout, d == passes - 1 ? perm : v0);
    psrc = kout;
  }
  hipLaunchKernelGGL(sdxs::k_reps_gather, grid, blk, 0, st, (int)n, S, (const int32_t*)perm, (const uint32_t*)psrc,
                     source_dev, (const sdx_repeat_key*)lkeys, times_dev, b.keys, ptimes, run_lo, run_hi, b.tile_last);
  // without times every time is 0 and W = 0: no gap ever exceeds the window
  launch_timed<true>(in, n, b, ptimes, times_dev ? window_us : 0, state, repeat_dev, sdxt::BySrc{psrc, perm, ipred, S}, st);
  hipLaunchKernelGGL(sdxs::k_reps_state, dim3((S + WAVES - 1) / WAVES), blk, 0, st, in, (int)n, nt, S,
                     (const sdx_repeat_key*)b.keys, (const int32_t*)run_lo, (const int32_t*)run_hi, (const int32_t*)ipred,
                     (const int32_t*)b.seg, (const int32_t*)b.exitv, (const int32_t*)b.lastv, (const int64_t*)b.te,
                     (const uint8_t*)b.flags, (const int32_t*)perm, state,
                     part<sdx_repeat_source_entry>(s, n, S, SDX_RS_TABLE));
  return launched(FN);
}
