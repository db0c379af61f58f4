// core/item_order.hpp swept on the host: the map from a pass's item index to (local pixel, sample, slot) for every pixels-per-group
// P.  Part one is exhaustive over small passes: every (pixel, sample) pair is produced exactly once, the slot is s * npix + lp,
// the items of a group are contiguous and sample-major, and P >= npix is the row-strip order (item == slot).  Part two spot-checks
// the prepared divisions near the largest pass the launcher makes (2^30 items): the first and last 4096 items and both sides of
// every group boundary, against plain 64-bit arithmetic.  Stand-alone: g++ tests/item_order_host_check.cpp && ./a.out
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../ray-tracing-series-rust_amd/csrc/core/item_order.hpp"

static long long failures = 0;
#define CHECK(cond)                                                                                                  \
  do {                                                                                                               \
    if (!(cond) && failures++ < 20)                                                                                  \
      std::printf("FAILED %s: npix %u S %u P %u item %llu\n", #cond, npix, S, P, (unsigned long long)g);              \
  } while (0)

// The issue's definition, in 64-bit arithmetic with the language's own divisions.
struct Plain { uint64_t k, lp, s, slot; };
static Plain plain_map(uint64_t npix, uint64_t S, uint64_t P, uint64_t g) {
  if (P > npix) P = npix;
  const uint64_t ng = (npix + P - 1) / P, p_last = npix - (ng - 1) * P;
  uint64_t k = g / (P * S);
  if (k > ng - 1) k = ng - 1;  // (never: the last group starts at (ng - 1) P S and is the shortest)
  const uint64_t r = g - k * P * S, pk = k == ng - 1 ? p_last : P;
  Plain m;
  m.k = k; m.s = r / pk; m.lp = k * P + r % pk; m.slot = m.s * npix + m.lp;
  return m;
}

static void check_item(uint32_t npix, uint32_t S, uint32_t P, const rt::ItemOrder& o, uint32_t g) {
  uint32_t lp = 0, s = 0;
  const uint32_t slot = rt::item_order_map(o, g, &lp, &s);
  const Plain m = plain_map(npix, S, P, g);
  CHECK(lp == m.lp);
  CHECK(s == m.s);
  CHECK(slot == m.slot);
  CHECK(lp < npix && s < S);
}

int main() {
  long long orders = 0, items = 0;
  // ---- part one
  const uint32_t npixs[] = {1u, 2u, 63u, 64u, 65u, 130u};
  const uint32_t spps[] = {1u, 2u, 5u, 64u, 67u};
  for (uint32_t npix : npixs)
    for (uint32_t S : spps) {
      const uint32_t groups[] = {1u, 2u, 3u, 8u, 64u, 65u, npix, npix + 1u, 1u << 30};
      for (uint32_t P : groups) {
        const rt::ItemOrder o = rt::make_item_order(npix, S, P);
        const uint32_t total = npix * S, pe = P < npix ? P : npix;
        std::vector<uint32_t> seen((size_t)total, 0u);
        uint32_t prev_k = 0, prev_s = 0, prev_lp = 0;
        for (uint32_t g = 0; g < total; ++g, ++items) {
          uint32_t lp = 0, s = 0;
          const uint32_t slot = rt::item_order_map(o, g, &lp, &s);
          CHECK(lp < npix && s < S);
          if (lp >= npix || s >= S) continue;
          CHECK(slot == s * npix + lp);
          seen[(size_t)s * npix + lp] += 1u;
          const uint32_t k = lp / pe;
          // contiguous groups in ascending order; inside one, sample-major: the pixel runs fastest, then the sample
          if (g > 0) {
            if (k == prev_k) {
              const uint32_t pk = (k + 1u) * pe <= npix ? pe : npix - k * pe;
              if (lp == prev_lp + 1u) CHECK(s == prev_s);
              else { CHECK(lp == k * pe && prev_lp == k * pe + pk - 1u && s == prev_s + 1u); }
            } else {
              CHECK(k == prev_k + 1u && lp == k * pe && s == 0u && prev_s == S - 1u && prev_lp == k * pe - 1u);
            }
          } else {
            CHECK(k == 0u && lp == 0u && s == 0u);
          }
          if (P >= npix) CHECK(slot == g);
          prev_k = k; prev_s = s; prev_lp = lp;
        }
        uint32_t g = total;  // (for the message)
        for (size_t q = 0; q < seen.size(); ++q)
          if (seen[q] != 1u) { CHECK(seen[q] == 1u); break; }
        ++orders;
      }
    }
  // ---- part two: passes of about 2^30 items (the 24 GiB default budget: 2^30 x 24 bytes)
  const uint32_t big_npix[] = {3840u * 2160u, 426400u};
  for (uint32_t npix : big_npix) {
    const uint32_t s_fit = (1u << 30) / npix;
    for (uint32_t S : {s_fit, s_fit + 1u, s_fit - 1u}) {
      const uint32_t groups[] = {1u, 2u, 3u, 4u, 8u, 16u, 32u, 64u, 65u, 1000u, 4096u, npix - 1u, npix, npix + 1u, 1u << 30};
      for (uint32_t P : groups) {
        const rt::ItemOrder o = rt::make_item_order(npix, S, P);
        const uint64_t total = (uint64_t)npix * S;
        if (total >= 0xFFFF0000ull) continue;  // (the launcher's limit of a pass)
        for (uint32_t g = 0; g < 4096u; ++g, items += 2) {
          check_item(npix, S, P, o, g);
          check_item(npix, S, P, o, (uint32_t)(total - 1u - g));
        }
        // both sides of every group boundary (of a strided subset where there are millions of groups; always the last ones)
        const uint64_t pe = P < npix ? P : npix, per_group = pe * S, ng = (npix + pe - 1) / pe;
        const uint64_t stride = ng > 20000 ? ng / 20000 : 1;
        for (uint64_t k = 1; k < ng; k += (k + stride < ng - 4 ? stride : 1)) {
          const uint64_t b = k * per_group;
          for (uint64_t g = b - 2; g <= b + 1 && g < total; ++g, ++items) check_item(npix, S, P, o, (uint32_t)g);
          // ... and of the sample boundaries inside the group before it
          for (uint64_t g = b - pe - 1; g <= b - pe + 1 && g < total; ++g, ++items) check_item(npix, S, P, o, (uint32_t)g);
        }
        ++orders;
      }
    }
  }
  // ---- the divisions themselves at the edges of 32 bits
  {
    const uint32_t npix = 0, S = 0, P = 0;
    const uint32_t ds[] = {1u, 2u, 3u, 5u, 7u, 64u, 65u, 641u, 65535u, 65536u, 65537u, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFEFFFFu, 0xFFFFFFFFu};
    const uint32_t ns[] = {0u, 1u, 2u, 63u, 64u, 65535u, 65536u, 0x7FFFFFFFu, 0x80000000u, 0xFFFEFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu};
    for (uint32_t d : ds) {
      const rt::Div32 v = rt::make_div32(d);
      for (uint32_t n0 : ns)
        for (uint32_t dn = 0; dn < 3u; ++dn) {
          const uint32_t g = n0 - dn;
          CHECK(rt::div32(g, v.m, v.sh1, v.sh2) == g / d);
          const uint32_t g2 = (g / d) * d;  // a multiple and its neighbour below
          CHECK(rt::div32(g2, v.m, v.sh1, v.sh2) == g2 / d);
          if (g2 > 0u) CHECK(rt::div32(g2 - 1u, v.m, v.sh1, v.sh2) == (g2 - 1u) / d);
        }
    }
  }
  if (failures) {
    std::printf("%lld failures over %lld orders, %lld items\n", failures, orders, items);
    return 1;
  }
  std::printf("item order host check clean: %lld orders, %lld items\n", orders, items);
  return 0;
}
