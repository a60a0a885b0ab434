// sdx_dispatch_layout.h -- the validator of sdx_dispatch_rules (include/sdx.h; pysignalduino_amd/dispatch.py
// fills the struct, sdx_dispatch.hip copies it into its kernels' arguments).  Plain C++ without any HIP type,
// so that a stand-alone host program can include it (tools/dispatch_rules_check.cpp runs the validator under
// the address / UB sanitizers over good and damaged structs).
//
//   keep_equal[kind][w]  bit b of word w = class 64 * w + b of the kind is exempt from the equal-message drop
//   max_repeat[kind]     >= 0, 0 = no cap
//   drop_equal           any value, 0 = off
//   res                  0
#ifndef SDX_DISPATCH_LAYOUT_H
#define SDX_DISPATCH_LAYOUT_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/sdx.h"

#define SDX_DISPATCH_CLASS_MAX 256 /* classes per kind: the bits of one mask */
#define SDX_DISPATCH_TILE 256      /* lines per workgroup of the pass's kernels */

#ifdef __cplusplus
static_assert(sizeof(sdx_dispatch_rules) == 152, "sdx_dispatch_rules layout");
static_assert(offsetof(sdx_dispatch_rules, max_repeat) == 128 && offsetof(sdx_dispatch_rules, drop_equal) == 144 &&
                  offsetof(sdx_dispatch_rules, res) == 148, "sdx_dispatch_rules layout");
#endif

/* 0 = good, otherwise a message (static storage).  n_class: the bank's class counts by enum sdx_kind. */
static inline const char* sdx_dispatch_validate(const sdx_dispatch_rules* r, const uint32_t n_class[4]) {
  if (!r) return "null rules";
  if (!n_class) return "null class counts";
  if (r->res) return "the reserved word is not 0";
  for (int kd = 0; kd < 4; ++kd) {
    if (n_class[kd] > SDX_DISPATCH_CLASS_MAX) return "a class count above 256";
    if (r->max_repeat[kd] < 0) return "a negative max_repeat";
    for (uint32_t w = 0; w < 4; ++w) {
      const uint32_t lo = 64u * w; /* the word's first class */
      const uint64_t legal = n_class[kd] >= lo + 64 ? ~0ull : n_class[kd] <= lo ? 0ull : (1ull << (n_class[kd] - lo)) - 1;
      if (r->keep_equal[kd][w] & ~legal) return "a keep_equal bit at or above its kind's class count";
    }
  }
  return 0;
}
#endif
