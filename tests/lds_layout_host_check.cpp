// ldsk_layout (csrc/hip/lds_layout.inc) swept on the host: the regions k_trace_lds carves out of its LDS block must be
// disjoint, in bounds and aligned as the kernel assumes, the node array must sit where the kernel's constant says, and
// `total` must be exactly what the launcher compares with its 160 KB.  Stand-alone: g++ tests/lds_layout_host_check.cpp && ./a.out
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../ray-tracing-series-rust_amd/csrc/core/flat_types.hpp"
#define __host__
#define __device__
namespace rtx {
#include "../ray-tracing-series-rust_amd/csrc/hip/lds_layout.inc"
}

static long long failures = 0;
#define CHECK(cond)                                                                                          \
  do {                                                                                                       \
    if (!(cond) && failures++ < 20)                                                                          \
      std::printf("FAILED %s: levels %u ring %u nodes %u x %u dwords, records %u (moving: %d)\n", #cond, levels, \
                  cap, d.n_nodes, d.node_dwords, n_rec, (int)moving);                                         \
  } while (0)

int main() {
  using namespace rtx;
  static_assert(sizeof(rt::FlatSphere) == 40 && sizeof(rt::FlatMovingSphere) == 80, "record sizes the layout is written for");
  static_assert(LDSK_OFF_NODES == 0u && LDSK_LEVEL_BYTES == 2048u && LDSK_LDS_MAX == 163840u, "constants the kernel is written for");
  const uint32_t caps[4] = {0u, 32u, 48u, 64u};
  const uint32_t node_sizes[3] = {LDSK_NODE_DWORDS, LDSK_MOTION1_NODE_DWORDS, LDSK_MOTION_NODE_DWORDS};
  const uint32_t counts[] = {1u, 2u, 3u, 7u, 30u, 97u, 301u, 485u, 1000u, 1947u, 4096u, LDSK_MAX_SLOTS};
  long long layouts = 0, fitting = 0;
  for (uint32_t levels = 2; levels <= 64; ++levels)
    for (uint32_t cap : caps)
      for (uint32_t nd : node_sizes)
        for (uint32_t n_rec : counts)
          for (uint32_t n_nodes : {n_rec > 1u ? n_rec - 1u : 1u, n_rec / 3u + 1u, LDSK_MAX_NODES})
            for (bool moving : {false, true}) {
              if (n_nodes == LDSK_MAX_NODES && n_rec != LDSK_MAX_SLOTS) continue;  // (the limits together, once)
              LdsSceneDims d = {n_nodes, n_rec, moving ? 0u : n_rec, moving ? n_rec : 0u, nd, 0u};
              const LdsKernelLayout L = ldsk_layout(levels, cap, d);
              ++layouts;
              // regions in address order, with their sizes in bytes
              const uint32_t node_bytes = n_nodes * nd * 4u, sphere_bytes = d.n_spheres * 40u, moving_bytes = d.n_moving * 80u;
              const uint32_t stack_bytes = levels * 1024u * 2u, ring_total = 16u * cap * 76u;
              const uint32_t off[5] = {L.off_nodes, L.off_spheres, L.off_moving, L.off_stacks, L.off_ring};
              const uint32_t len[5] = {node_bytes, sphere_bytes, moving_bytes, stack_bytes, ring_total};
              CHECK(L.off_nodes == LDSK_OFF_NODES);
              CHECK(L.off_refs == L.off_spheres);
              for (int i = 0; i < 5; ++i) {
                CHECK(off[i] % 16u == 0u);                                  // records, stacks and rings: 16-byte aligned
                CHECK((uint64_t)off[i] + len[i] <= (uint64_t)(i < 4 ? off[i + 1] : L.total));  // disjoint, in order, in bounds
              }
              CHECK(L.total - (L.off_ring + ring_total) == 0u);             // nothing counted that nobody uses
              // the deepest slot a walk can write (level `levels - 1` of thread 1023) lies inside the stacks
              CHECK(L.off_stacks + (levels - 1u) * LDSK_LEVEL_BYTES + 1023u * 2u + 2u <= L.off_ring);
              // odd dword strides are what spreads a wave's node reads over the banks
              CHECK(nd % 2u == 1u);
              // `total` is the sum of the aligned parts: what the launcher holds against 160 KB
              const uint64_t want = (uint64_t)((node_bytes + 15u) & ~15u) + ((sphere_bytes + 15u) & ~15u) + ((moving_bytes + 15u) & ~15u) +
                                    stack_bytes + ring_total;
              CHECK((uint64_t)L.total == want);
              if (L.total <= LDSK_LDS_MAX) ++fitting;
              // what the kernel's address arithmetic assumes: index x record size is a v_mul_u32_u24 (both factors and, for
              // a layout that fits, the product far below 2^24), and every field of a record -- the far child's block, the
              // axis pair, the item that closes the block -- is a DS immediate offset (16 bits) from the record's address
              CHECK(LDSK_MAX_NODES < (1u << 24) && nd * 4u < (1u << 24));
              CHECK((uint64_t)LDSK_MAX_NODES * nd * 4u < (1ull << 24));
              CHECK(nd * 4u < 65536u && LDSK_LEVEL_BYTES < 65536u);
            }
  std::printf("%lld layouts, %lld of them within %u bytes, %lld failures\n", layouts, fitting, LDSK_LDS_MAX, failures);
  if (failures == 0 && fitting > 0) std::printf("lds layout host check clean\n");
  return failures == 0 && fitting > 0 ? 0 : 1;
}
