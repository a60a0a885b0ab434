// sdx_route_layout.h -- the route table's blob (pysignalduino_amd/routes.py writes it, sdx_route.hip
// uploads and walks it) and its validator, host + device.  Plain C++ without any HIP type, so that a
// stand-alone host program can include it (tools/route_blob_check.cpp runs the validator under the
// address / UB sanitizers over good and damaged blobs).
//
//   blob  [ sdx_route_hdr (32 bytes)
//         | cls_of: uint8[256]            byte -> class, every entry < n_class
//         | dfa: sdx_route_dfa[n_routes]  per route: state count, start state, offsets of its two tables
//         | per route, in route order:    flags: uint8[n_states] (SDX_ROUTE_ACC_NOW / _ACC_END / _DEAD),
//                                         trans: uintW[n_states][n_class], W = trans_width bytes (1 or 2);
//                                         each table begins on a 4-byte boundary ]
// Offsets count from the blob's first byte.  All integers little-endian.
// A walk: st = start; for each payload byte b while flags[st] has neither ACC_NOW nor DEAD:
// st = trans[st][cls_of[b]].  Match = ACC_NOW, or every byte consumed and ACC_END (re.search).
#ifndef SDX_ROUTE_LAYOUT_H
#define SDX_ROUTE_LAYOUT_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define SDX_ROUTE_MAGIC 0x54525853u     /* "SXRT" */
#define SDX_ROUTE_VERSION 1u
#define SDX_ROUTE_MAX 64                /* routes per table: one bit each of the line's mask */
#define SDX_ROUTE_STATES_MAX 4096       /* states per DFA */
#define SDX_ROUTE_BLOB_MAX (1u << 20)   /* bytes per blob */
#define SDX_ROUTE_ACC_NOW 1u            /* regex_dfa.ACC_NOW: a match ends here */
#define SDX_ROUTE_ACC_END 2u            /* regex_dfa.ACC_END: a match when the payload ends here */
#define SDX_ROUTE_DEAD 4u               /* regex_dfa.DEAD: no match reachable any more */
#define SDX_ROUTE_TILE 256              /* lines per workgroup of k_route */
/* LDS of one k_route workgroup: eight workgroups of 256 threads fill a CU's 32 wave slots and its 160 KiB */
#define SDX_ROUTE_LDS_BYTES 20480u

typedef struct {
  uint32_t magic, version;
  uint32_t n_routes;     /* 1 .. SDX_ROUTE_MAX */
  uint32_t n_class;      /* 1 .. 256 */
  uint32_t trans_width;  /* 1: every DFA has <= 256 states, uint8 transitions; 2: uint16 */
  uint32_t total_bytes;  /* the blob's size */
  uint32_t res[2];       /* 0 */
} sdx_route_hdr;         /* 32 bytes */

typedef struct {
  uint32_t n_states;     /* 1 .. SDX_ROUTE_STATES_MAX (<= 256 with trans_width 1) */
  uint32_t start;        /* < n_states */
  uint32_t flags_off;    /* uint8[n_states] */
  uint32_t trans_off;    /* uintW[n_states * n_class], every entry < n_states */
} sdx_route_dfa;         /* 16 bytes */

/* macros, so that device code can use them too */
#define SDX_ROUTE_CLS_OFF sizeof(sdx_route_hdr)
#define SDX_ROUTE_DFA_OFF (SDX_ROUTE_CLS_OFF + 256)
static inline size_t sdx_route_tables_off(uint32_t n_routes) { return SDX_ROUTE_DFA_OFF + sizeof(sdx_route_dfa) * (size_t)n_routes; }

/* The whole blob checked against nbytes: 0 = good, otherwise a message (static storage).  Reads nothing
 * outside blob[0, nbytes); the blob may stand at any address (fields are copied out). */
static inline const char* sdx_route_validate(const uint8_t* blob, size_t nbytes) {
  if (!blob) return "null blob";
  if (nbytes < sizeof(sdx_route_hdr)) return "shorter than its header";
  if (nbytes > SDX_ROUTE_BLOB_MAX) return "larger than SDX_ROUTE_BLOB_MAX";
  sdx_route_hdr h;
  memcpy(&h, blob, sizeof h);
  if (h.magic != SDX_ROUTE_MAGIC) return "wrong magic";
  if (h.version != SDX_ROUTE_VERSION) return "wrong version";
  if (h.total_bytes != nbytes) return "total_bytes is not the blob's size";
  if (nbytes & 3u) return "the blob's size is no multiple of 4";
  if (h.n_routes < 1 || h.n_routes > SDX_ROUTE_MAX) return "route count outside 1 .. 64";
  if (h.n_class < 1 || h.n_class > 256) return "class count outside 1 .. 256";
  if (h.trans_width != 1 && h.trans_width != 2) return "transition width is neither 1 nor 2";
  if (h.res[0] || h.res[1]) return "reserved header words are not 0";
  const size_t tables = sdx_route_tables_off(h.n_routes);
  if (tables > nbytes) return "cls_of / DFA records run past the blob";
  const uint8_t* cls = blob + SDX_ROUTE_CLS_OFF;
  for (int b = 0; b < 256; ++b)
    if (cls[b] >= h.n_class) return "a cls_of entry is not below the class count";
  size_t at = tables; /* the tables stand in route order without overlap */
  for (uint32_t r = 0; r < h.n_routes; ++r) {
    sdx_route_dfa d;
    memcpy(&d, blob + SDX_ROUTE_DFA_OFF + sizeof d * (size_t)r, sizeof d);
    if (d.n_states < 1 || d.n_states > SDX_ROUTE_STATES_MAX) return "a DFA's state count is outside 1 .. 4096";
    if (h.trans_width == 1 && d.n_states > 256) return "a DFA of more than 256 states with uint8 transitions";
    if (d.start >= d.n_states) return "a start state is not below the state count";
    if ((d.flags_off & 3u) || (d.trans_off & 3u)) return "a table is not 4-byte aligned";
    if (d.flags_off < at || d.flags_off > nbytes || (size_t)d.n_states > nbytes - d.flags_off)
      return "a flags table lies outside the blob or in front of its place";
    at = (size_t)d.flags_off + d.n_states;
    const size_t tb = (size_t)d.n_states * h.n_class * h.trans_width;
    if (d.trans_off < at || d.trans_off > nbytes || tb > nbytes - d.trans_off)
      return "a transition table lies outside the blob or in front of its place";
    at = (size_t)d.trans_off + tb;
    const uint8_t* fl = blob + d.flags_off;
    for (uint32_t s = 0; s < d.n_states; ++s)
      if (fl[s] > (SDX_ROUTE_ACC_NOW | SDX_ROUTE_ACC_END | SDX_ROUTE_DEAD)) return "unknown state flags";
    const uint8_t* t = blob + d.trans_off;
    const size_t cells = (size_t)d.n_states * h.n_class;
    for (size_t i = 0; i < cells; ++i) {
      const uint32_t to = h.trans_width == 1 ? t[i] : (uint32_t)t[2 * i] | ((uint32_t)t[2 * i + 1] << 8);
      if (to >= d.n_states) return "a transition is not below its DFA's state count";
    }
  }
  return 0;
}

/* How many of the table's routes k_route serves from LDS: it stages blob[sizeof(hdr), end) with end = the
 * end of the last route whose tables still lie inside the budget (at least cls_of and the DFA records,
 * which always fit).  *lds_bytes = the staged bytes, a multiple of 4.  Only for a validated blob. */
static inline uint32_t sdx_route_lds_routes(const uint8_t* blob, uint32_t budget, uint32_t* lds_bytes) {
  sdx_route_hdr h;
  memcpy(&h, blob, sizeof h);
  size_t end = sdx_route_tables_off(h.n_routes);
  uint32_t r = 0;
  for (; r < h.n_routes; ++r) {
    sdx_route_dfa d;
    memcpy(&d, blob + SDX_ROUTE_DFA_OFF + sizeof d * (size_t)r, sizeof d);
    const size_t e = ((size_t)d.trans_off + (size_t)d.n_states * h.n_class * h.trans_width + 3) & ~(size_t)3;
    if (e - sizeof(sdx_route_hdr) > budget) break;
    end = e;
  }
  /* whole words: the blob's size is a multiple of 4, so a table's rounded end lies inside it */
  *lds_bytes = (uint32_t)(end - sizeof(sdx_route_hdr));
  return r;
}
#endif
