// sdx_repeat_layout.h -- sizes and offsets of sdx_mark_repeats' two caller-owned buffers, host + device.
// Plain C++ without any HIP type, so that a stand-alone host program can include it
// (tools/repeat_layout_check.cpp runs these functions under the address / UB sanitizers).
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
#endif
