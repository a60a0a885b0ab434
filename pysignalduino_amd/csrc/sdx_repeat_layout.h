// sdx_repeat_layout.h -- sizes and offsets of sdx_mark_repeats' two caller-owned buffers, and of
// sdx_mark_repeats_timed's and sdx_mark_repeats_by_source's two each (further down), host + device.
// Plain C++ without any HIP type, so that a stand-alone host program can include it
// (tools/repeat_layout_check.cpp, tools/repeat_timed_layout_check.cpp and
// tools/repeat_sources_layout_check.cpp run these functions under the address / UB sanitizers).
//
//   state    [ sdx_repeat_state_hdr | payload bytes, room for SDX_REPEAT_PAYLOAD_MAX ]
//   scratch  [ head: 4 x int32, [0] = the chunk's last result-bearing line or -1
//            | keys: sdx_repeat_key[n]
//            | tile_last: int32[tiles]   last result-bearing line of tile b, -1 = none
//            | tile_prev: int32[tiles]   last result-bearing line in front of tile b, -1 = none ]
#ifndef SDX_REPEAT_LAYOUT_H
#define SDX_REPEAT_LAYOUT_H
#include <stddef.h>
#include <stdint.h>

#define SDX_REPEAT_TILE 256            /* lines per workgroup of the key and resolve passes */
#define SDX_REPEAT_PAYLOAD_MAX 65535   /* sdx_result.payload_len is 16 bits wide */
#define SDX_REPEAT_NONE 0xFFFFFFFFu    /* sdx_repeat_key.kind of a line without results */

typedef struct {
  uint32_t kind;   /* enum sdx_kind, SDX_REPEAT_NONE = the line has no result */
  uint32_t proto;  /* decoded[0]'s record index inside its kind's table */
  uint32_t len;    /* its payload: heap[off, off + len) of the kind's launch */
  uint32_t off;
} sdx_repeat_key;  /* 16 bytes */

typedef struct {
  uint32_t valid;  /* 0 = no previous result-bearing line (a new stream: the caller zeroes the header) */
  uint32_t kind, proto, len;
} sdx_repeat_state_hdr;  /* 16 bytes, the payload bytes follow */

static inline size_t sdx_repeat_state_size(void) {
  /* the payload room rounded up to 16 bytes: the buffer's end stays aligned */
  return sizeof(sdx_repeat_state_hdr) + (((size_t)SDX_REPEAT_PAYLOAD_MAX + 15) & ~(size_t)15);
}

static inline int64_t sdx_repeat_tiles(int64_t n) { return n > 0 ? (n + SDX_REPEAT_TILE - 1) / SDX_REPEAT_TILE : 0; }

static inline size_t sdx_repeat_keys_off(void) { return 16; }
static inline size_t sdx_repeat_tile_last_off(int64_t n) {
  return sdx_repeat_keys_off() + sizeof(sdx_repeat_key) * (size_t)(n > 0 ? n : 0);
}
static inline size_t sdx_repeat_tile_prev_off(int64_t n) {
  return sdx_repeat_tile_last_off(n) + sizeof(int32_t) * (size_t)sdx_repeat_tiles(n);
}
static inline size_t sdx_repeat_scratch_size(int64_t n) {
  const size_t end = sdx_repeat_tile_prev_off(n) + sizeof(int32_t) * (size_t)sdx_repeat_tiles(n);
  return (end + 15) & ~(size_t)15;
}

/* ---- sdx_mark_repeats_timed: buffers of its own, the two above stay as they are ------------------
 *   state    [ sdx_repeat_timed_state_hdr: valid, kind, proto, len, T | payload bytes, room as above ]
 *            K = (kind, proto, payload) of the last result-bearing line, T = the time of the last one
 *            that was not marked
 *   scratch  [ head: 4 x int32, [0] = the chunk's last result-bearing line, [1] = its last segment head
 *            | keys: sdx_repeat_key[n]
 *            | te:   int64[n]   the line's time; a line without results holds its predecessor's
 *            | seg:  int32[n]   the last segment head at or in front of the line, -1 = none
 *            | succ: int32[n]   next line of the orbit when the line is an anchor, -1 = the segment ends
 *            | exit: int32[n]   first orbit line behind the line's tile, -1 = none
 *            | last: int32[n]   last orbit line inside the line's tile
 *            | tile_last, tile_prev, tile_head, tile_prevhead, tile_arr: int32[tiles] each
 *            | flags: uint8[n]  SDX_RT_* ] */
#define SDX_RT_RB 1u    /* result-bearing */
#define SDX_RT_HEAD 2u  /* segment head: another key than the predecessor's, or a gap > W to it */
#define SDX_RT_SREP 4u  /* the chunk's first result-bearing line, a repeat by the carried (K, T) */

typedef struct {
  uint32_t valid;  /* 0 = a new stream (the caller zeroes the header) */
  uint32_t kind, proto, len;
  int64_t t;       /* T, microseconds */
} sdx_repeat_timed_state_hdr; /* 24 bytes, the payload bytes follow */

/* a macro, so that device code can use it too (the slots of sdx_mark_repeats_by_source) */
#define SDX_REPEAT_TIMED_STATE_SIZE ((sizeof(sdx_repeat_timed_state_hdr) + (size_t)SDX_REPEAT_PAYLOAD_MAX + 15) & ~(size_t)15)
static inline size_t sdx_repeat_timed_state_size(void) { return SDX_REPEAT_TIMED_STATE_SIZE; }

static inline size_t sdx_rt_lines(int64_t n) { return (size_t)(n > 0 ? n : 0); }
static inline size_t sdx_rt_keys_off(void) { return 16; }
static inline size_t sdx_rt_te_off(int64_t n) { return sdx_rt_keys_off() + sizeof(sdx_repeat_key) * sdx_rt_lines(n); }
static inline size_t sdx_rt_seg_off(int64_t n) { return sdx_rt_te_off(n) + sizeof(int64_t) * sdx_rt_lines(n); }
static inline size_t sdx_rt_succ_off(int64_t n) { return sdx_rt_seg_off(n) + sizeof(int32_t) * sdx_rt_lines(n); }
static inline size_t sdx_rt_exit_off(int64_t n) { return sdx_rt_succ_off(n) + sizeof(int32_t) * sdx_rt_lines(n); }
static inline size_t sdx_rt_last_off(int64_t n) { return sdx_rt_exit_off(n) + sizeof(int32_t) * sdx_rt_lines(n); }
/* the five tile tables, t = 0 .. 4 in the order above */
static inline size_t sdx_rt_tile_off(int64_t n, int t) {
  return sdx_rt_last_off(n) + sizeof(int32_t) * sdx_rt_lines(n) + sizeof(int32_t) * (size_t)sdx_repeat_tiles(n) * (size_t)t;
}
static inline size_t sdx_rt_flags_off(int64_t n) { return sdx_rt_tile_off(n, 5); }
static inline size_t sdx_repeat_timed_scratch_size(int64_t n) {
  return (sdx_rt_flags_off(n) + sdx_rt_lines(n) + 15) & ~(size_t)15;
}

/* ---- sdx_mark_repeats_by_source: one (K, T) per source id, buffers of its own --------------------
 *   state    n_sources slots of sdx_repeat_timed_state_size() bytes, each with the timed state's layout;
 *            slot s carries source s
 *   scratch  the parts below in this order, each rounded up to 16 bytes.  "position" = a line's place
 *            after the stable sort by source id, so that every source's lines are contiguous and in
 *            stream order; the timed pass's arrays are indexed by position here */
#define SDX_REPEAT_SOURCES_MAX 4096

typedef struct {
  uint32_t valid;  /* the slot's header after this chunk ... */
  uint32_t kind, proto, len;
  int64_t t;       /* ... and its T */
  int32_t last;    /* the source's last result-bearing line in this chunk (line index), -1 = none */
  int32_t pad;
} sdx_repeat_source_entry; /* 32 bytes */

enum {
  SDX_RS_HEAD,    /* 4 x int32: [0] = the last result-bearing position, [1] = the last segment head */
  SDX_RS_TABLE,   /* sdx_repeat_source_entry[S]: what the host reads back, one copy per chunk */
  SDX_RS_RUN_LO,  /* int32[S]  first position of the source's lines ... */
  SDX_RS_RUN_HI,  /* int32[S]  ... and the position behind its last (lo == hi: absent) */
  SDX_RS_LKEYS,   /* sdx_repeat_key[n] by line */
  SDX_RS_KEYS,    /* sdx_repeat_key[n] by position */
  SDX_RS_TE,      /* int64[n] as the timed pass's */
  SDX_RS_PTIMES,  /* int64[n] the lines' times by position (0 without times) */
  SDX_RS_SEG,     /* int32[n] */
  SDX_RS_SUCC,    /* int32[n] */
  SDX_RS_EXIT,    /* int32[n] */
  SDX_RS_LAST,    /* int32[n] */
  SDX_RS_IPRED,   /* int32[n] the last result-bearing position at or in front of the position, -1 = none */
  SDX_RS_PERM,    /* int32[n] position -> line */
  SDX_RS_K0,      /* uint32[n] sort keys (the clamped ids), two copies, and one spare copy of the values */
  SDX_RS_K1,
  SDX_RS_V0,
  SDX_RS_TILES,   /* int32[6 * tiles]: tile_last, tile_prev, tile_head, tile_prevhead, tile_arr, spare */
  SDX_RS_HIST,    /* uint32[256 * tiles]: hist[digit * tiles + tile] */
  SDX_RS_TOT,     /* uint32[256] */
  SDX_RS_FLAGS,   /* uint8[n] SDX_RT_* */
  SDX_RS_END
};

static inline int sdx_rs_sources_ok(int64_t n_sources) { return n_sources >= 1 && n_sources <= SDX_REPEAT_SOURCES_MAX; }

static inline size_t sdx_rs_part_bytes(int64_t n, int64_t n_sources, int part) {
  const size_t L = sdx_rt_lines(n), S = sdx_rs_sources_ok(n_sources) ? (size_t)n_sources : 0;
  const size_t tiles = (size_t)sdx_repeat_tiles(n);
  switch (part) {
    case SDX_RS_HEAD: return 16;
    case SDX_RS_TABLE: return sizeof(sdx_repeat_source_entry) * S;
    case SDX_RS_RUN_LO: case SDX_RS_RUN_HI: return sizeof(int32_t) * S;
    case SDX_RS_LKEYS: case SDX_RS_KEYS: return sizeof(sdx_repeat_key) * L;
    case SDX_RS_TE: case SDX_RS_PTIMES: return sizeof(int64_t) * L;
    case SDX_RS_SEG: case SDX_RS_SUCC: case SDX_RS_EXIT: case SDX_RS_LAST: case SDX_RS_IPRED: case SDX_RS_PERM:
    case SDX_RS_K0: case SDX_RS_K1: case SDX_RS_V0: return sizeof(int32_t) * L;
    case SDX_RS_TILES: return sizeof(int32_t) * 6 * tiles;
    case SDX_RS_HIST: return sizeof(uint32_t) * 256 * tiles;
    case SDX_RS_TOT: return sizeof(uint32_t) * 256;
    case SDX_RS_FLAGS: return L;
    default: return 0;
  }
}
/* offset of a part; sdx_rs_off(n, S, SDX_RS_END) = the scratch buffer's size */
static inline size_t sdx_rs_off(int64_t n, int64_t n_sources, int part) {
  size_t off = 0;
  for (int p = 0; p < part && p < SDX_RS_END; ++p) off += (sdx_rs_part_bytes(n, n_sources, p) + 15) & ~(size_t)15;
  return off;
}
static inline size_t sdx_repeat_sources_scratch_size(int64_t n, int64_t n_sources) {
  return sdx_rs_sources_ok(n_sources) ? sdx_rs_off(n, n_sources, SDX_RS_END) : 0;
}
static inline size_t sdx_repeat_sources_state_size(int64_t n_sources) {
  return sdx_rs_sources_ok(n_sources) ? (size_t)n_sources * sdx_repeat_timed_state_size() : 0;
}
/* radix passes of 8 bits over the ids 0 .. S - 1 */
static inline int sdx_rs_passes(int64_t n_sources) { return n_sources > 256 ? 2 : 1; }
#endif
