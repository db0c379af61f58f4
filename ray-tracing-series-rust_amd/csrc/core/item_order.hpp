// The order of a pass's items: which (pixel, sample) pair item g of the index space [0, npix * S) is.  Plain integers, no HIP:
// the trace kernels call it through pass_items.inc, the launcher prepares it per pass, tests/item_order_host_check.cpp sweeps it.
//
// A pass of npix pixels (or entries of an adaptive pass's active list) and S samples is cut into NG = ceil(npix / P) GROUPS of P
// consecutive local pixels; only the last group may be short (P_last = npix - (NG - 1) P pixels).  Group k owns the contiguous
// items [k P S, k P S + P_k S), and inside a group item r is sample-major: s = r / P_k, p = r % P_k, lp = k P + p.  So a wave
// that claims consecutive items holds many samples of few pixels when P is small, and P >= npix is one group: item
// g = s * npix + lp, a row strip of one sample.  The sample's SLOT in the pass's sample buffer does not depend on P:
// slot = s * npix + lp, the layout the reduction kernels read.
//
// The three divisors (P S, P, P_last) are constants of a pass: the host turns each into a multiplier and two shifts
// (Granlund & Montgomery 1994, the round-up form, exact for every 32-bit dividend and every divisor >= 1), so that a path's
// start costs two multiply-highs instead of emulated divisions.
#pragma once

#include <cstdint>

#include "rt_config.hpp"

namespace rt {

// n / d for a divisor known on the host: t = mulhi(m, n), q = (t + ((n - t) >> sh1)) >> sh2.
struct Div32 {
  uint32_t d, m, sh1, sh2;
};

inline Div32 make_div32(uint32_t d) {  // d >= 1
  uint32_t l = 0;
  while (l < 32u && ((uint64_t)1 << l) < (uint64_t)d) ++l;  // ceil(log2 d)
  Div32 v;
  v.d = d;
  v.m = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << l) - (uint64_t)d)) / (uint64_t)d + 1u);
  v.sh1 = l < 1u ? l : 1u;
  v.sh2 = l < 1u ? 0u : l - 1u;
  return v;
}

RT_HD uint32_t mulhi_u32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

RT_HD uint32_t div32(uint32_t n, uint32_t m, uint32_t sh1, uint32_t sh2) {
  const uint32_t t = mulhi_u32(m, n);
  return (t + ((n - t) >> sh1)) >> sh2;
}

// Largest pixels-per-group a pass takes (RTX_ITEM_GROUP's range is [1, ITEM_GROUP_MAX]); at or above npix it is the row-strip order.
constexpr uint32_t ITEM_GROUP_MAX = 1u << 30;

// One pass's order, prepared on the host (make_item_order).
struct ItemOrder {
  Div32 group;      // by P S: items of a full group
  Div32 body;       // by P
  Div32 last;       // by P_last
  uint32_t last_k;  // NG - 1: the one group that may be short
  uint32_t npix;    // pixels (or active-list entries) of the pass: a sample plane of the sample buffer
};
constexpr uint32_t ITEM_ORDER_DWORDS = 14;
static_assert(sizeof(ItemOrder) == ITEM_ORDER_DWORDS * 4u, "pass_items.inc reads it dword by dword");

// npix >= 1, S >= 1, P >= 1, npix * S < 2^32.
inline ItemOrder make_item_order(uint32_t npix, uint32_t S, uint32_t P) {
  if (P > npix) P = npix;  // (one group: P S stays below 2^32)
  const uint32_t ng = (npix + P - 1u) / P;
  ItemOrder o;
  o.group = make_div32(P * S);
  o.body = make_div32(P);
  o.last = make_div32(npix - (ng - 1u) * P);
  o.last_k = ng - 1u;
  o.npix = npix;
  return o;
}

// Item g -> local pixel (or active-list entry) *lp and sample *s of the pass; returns the sample's slot s * npix + lp.
RT_HD uint32_t item_order_map(const ItemOrder& o, uint32_t g, uint32_t* lp, uint32_t* s) {
  const uint32_t k = div32(g, o.group.m, o.group.sh1, o.group.sh2);
  const uint32_t r = g - k * o.group.d;
  const bool in_last = k == o.last_k;
  const uint32_t pk = in_last ? o.last.d : o.body.d;
  const uint32_t sl = div32(r, in_last ? o.last.m : o.body.m, in_last ? o.last.sh1 : o.body.sh1, in_last ? o.last.sh2 : o.body.sh2);
  const uint32_t pix = k * o.body.d + (r - sl * pk);
  *lp = pix;
  *s = sl;
  return sl * o.npix + pix;
}

}  // namespace rt
