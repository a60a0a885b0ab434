// sdx_profile_layout.h -- the receiver-profile table's blob (pysignalduino_amd/profiles.py writes it,
// sdx_profile.hip uploads and reads it) and its validator, host + device.  Plain C++ without any HIP type,
// so that a stand-alone host program can include it (tools/profile_blob_check.cpp runs the validator under
// the address / UB sanitizers over good and damaged blobs).
//
//   blob  [ sdx_profile_hdr (48 bytes)
//         | mask: uint64[n_profiles][4][4]   per profile and kind (enum sdx_kind) 256 bits: bit c = the kind's
//                                            class c (sdx_result.proto) is enabled
//         | of_source: uint8[n_sources]      source id -> profile index, every entry < n_profiles
//         | zero bytes up to a multiple of 16 ]
// All integers little-endian.  A record of kind K of a line of source s is kept when bit proto of
// mask[of_source[s]][K] is set.
#ifndef SDX_PROFILE_LAYOUT_H
#define SDX_PROFILE_LAYOUT_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define SDX_PROFILE_MAGIC 0x46505853u   /* "SXPF" */
#define SDX_PROFILE_VERSION 1u
#define SDX_PROFILE_MAX 64              /* profiles per table */
#define SDX_PROFILE_SOURCES_MAX 4096    /* source ids per table: SDX_REPEAT_SOURCES_MAX */
#define SDX_PROFILE_CLASS_MAX 256       /* classes per kind: the bits of one mask */
#define SDX_PROFILE_TILE 256            /* lines per workgroup of the filter's kernels */

typedef struct {
  uint32_t magic, version;
  uint32_t total_bytes;   /* the blob's size, a multiple of 16 */
  uint32_t n_profiles;    /* 1 .. SDX_PROFILE_MAX */
  uint32_t n_sources;     /* 1 .. SDX_PROFILE_SOURCES_MAX */
  uint32_t n_class[4];    /* the bank's class counts by enum sdx_kind (MU, MS, MC, MN), each <= 256 */
  uint32_t res[3];        /* 0 */
} sdx_profile_hdr;        /* 48 bytes */

/* macros, so that device code can use them too */
#define SDX_PROFILE_MASK_OFF sizeof(sdx_profile_hdr)
#define SDX_PROFILE_MASK_BYTES 128u     /* one profile: 4 kinds of 4 words */
static inline size_t sdx_profile_src_off(uint32_t n_profiles) { return SDX_PROFILE_MASK_OFF + (size_t)SDX_PROFILE_MASK_BYTES * n_profiles; }
static inline size_t sdx_profile_bytes(uint32_t n_profiles, uint32_t n_sources) {
  return (sdx_profile_src_off(n_profiles) + n_sources + 15) & ~(size_t)15;
}

/* The whole blob checked against nbytes: 0 = good, otherwise a message (static storage).  Reads nothing
 * outside blob[0, nbytes); the blob may stand at any address (fields are copied out). */
static inline const char* sdx_profile_validate(const uint8_t* blob, size_t nbytes) {
  if (!blob) return "null blob";
  if (nbytes < sizeof(sdx_profile_hdr)) return "shorter than its header";
  sdx_profile_hdr h;
  memcpy(&h, blob, sizeof h);
  if (h.magic != SDX_PROFILE_MAGIC) return "wrong magic";
  if (h.version != SDX_PROFILE_VERSION) return "wrong version";
  if (h.total_bytes != nbytes) return "total_bytes is not the blob's size";
  if (h.n_profiles < 1 || h.n_profiles > SDX_PROFILE_MAX) return "profile count outside 1 .. 64";
  if (h.n_sources < 1 || h.n_sources > SDX_PROFILE_SOURCES_MAX) return "source count outside 1 .. 4096";
  for (int kd = 0; kd < 4; ++kd)
    if (h.n_class[kd] > SDX_PROFILE_CLASS_MAX) return "a class count above 256";
  if (h.res[0] || h.res[1] || h.res[2]) return "reserved header words are not 0";
  if (sdx_profile_bytes(h.n_profiles, h.n_sources) != nbytes) return "the blob's size is not that of its counts";
  for (uint32_t p = 0; p < h.n_profiles; ++p)
    for (int kd = 0; kd < 4; ++kd)
      for (uint32_t w = 0; w < 4; ++w) {
        uint64_t m;
        memcpy(&m, blob + SDX_PROFILE_MASK_OFF + (size_t)SDX_PROFILE_MASK_BYTES * p + 32u * kd + 8u * w, sizeof m);
        const uint32_t lo = 64u * w; /* the word's first class */
        const uint64_t legal = h.n_class[kd] >= lo + 64 ? ~0ull : h.n_class[kd] <= lo ? 0ull : (1ull << (h.n_class[kd] - lo)) - 1;
        if (m & ~legal) return "a mask bit at or above its kind's class count";
      }
  const size_t so = sdx_profile_src_off(h.n_profiles);
  for (uint32_t s = 0; s < h.n_sources; ++s)
    if (blob[so + s] >= h.n_profiles) return "an of_source entry is not below the profile count";
  for (size_t i = so + h.n_sources; i < nbytes; ++i)
    if (blob[i]) return "padding bytes are not 0";
  return 0;
}
#endif
