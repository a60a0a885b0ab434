// sdx_repeat_layout.h -- sizes and offsets of sdx_mark_repeats' two caller-owned buffers, and of
// sdx_mark_repeats_timed's two (further down), host + device.
// Plain C++ without any HIP type, so that a stand-alone host program can include it
// (tools/repeat_layout_check.cpp and tools/repeat_timed_layout_check.cpp run these functions under the
// address / UB sanitizers).
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

static inline size_t sdx_repeat_timed_state_size(void) {
  return (sizeof(sdx_repeat_timed_state_hdr) + (size_t)SDX_REPEAT_PAYLOAD_MAX + 15) & ~(size_t)15;
}

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
#endif
