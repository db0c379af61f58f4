// k_trace_lds's LDS layout (included by render.hip inside namespace rtx, ahead of the kernels; needs core/flat_types.hpp and
// nothing of the device: tests/lds_layout_host_check.cpp compiles it with a host compiler and sweeps it).
//
//     [ nodes: n x 84 B (108 / 156 B with time-aware boxes) ][ spheres: n x 40 B ][ moving spheres: n x 80 B ]
//     [ walk stacks: levels x 1024 x u16 ][ primary-ray rings: 16 waves x ring_cap (64, or 48 when LDS is tight, else none) x 76 B ]   <= 160 KB
//
// The node array comes first, at a FIXED offset: a node's address is index x record size + a constant the compiler folds into
// the multiply, and every field of the record is an immediate offset of its DS instruction.  Everything behind it starts at a
// runtime offset; those bases are added where an address is formed once per thread (the stacks) or once per leaf (the records).

// A wave's ring of ready primary rays in LDS (k_trace_vote, k_trace_lds; RTX_RING): f64 [RING_F64][cap], then u32 [cap] (the
// item).  trace_ring.inc -- the top-up and the take, included by both kernels -- is the only text that knows the rows.  Bytes
// per wave:
#define RING_F64 9u
__host__ __device__ constexpr uint32_t ring_bytes(uint32_t cap) { return cap * (RING_F64 * 8u + 4u); }

struct LdsSceneDims {  // what k_trace_lds (trace_lds.inc) copies into LDS
  uint32_t n_nodes, n_refs, n_spheres, n_moving;  // n_refs = leaf slots; one record per slot, in slot order: n_spheres or n_moving = n_refs
  uint32_t node_dwords;  // LDSK_NODE_DWORDS, or LDSK_MOTION_NODE_DWORDS / LDSK_MOTION1_NODE_DWORDS for the time-aware instantiations
  uint32_t n_uni;        // scenes with moving spheres: how many of the n_moving records are the scene's STATIC spheres, kept as moving spheres that stand still (n_spheres = 0 then; informational: the kernel decides per slot)
};

#define LDSK_BLOCK 1024
#define LDSK_MAX_SLOTS 8190u    // leaf item: first < 2^13, count <= 4
#define LDSK_MAX_NODES 8191u     // node item = split axis << 13 | index: the axis travels with the item
#define LDSK_NODE_DWORDS 21u     // per child and axis [lo, hi, lo] (18) + the two child items + 1 of padding (odd stride: no LDS bank pile-up; record 0's holds the root's item)
#define LDSK_MOTION_NODE_DWORDS 39u  // time-aware boxes: per child 9 planes + 9 slopes + the item (19), twice, + 1 of padding
#define LDSK_MOTION1_NODE_DWORDS 27u  // ... when everything moves along ONE axis: per child 9 planes + that axis's 3 slopes + the item (13)
#define LDSK_OFF_NODES 0u  // where the node array starts: the kernel's constant (its dynamic LDS starts at address 0, which plan_lds checks)
#define LDSK_LEVEL_BYTES (LDSK_BLOCK * 2u)  // one stack level of the workgroup: a push or a pop moves a thread's top by exactly this
#define LDSK_LDS_MAX (160u * 1024u)  // what the launcher fits `total` into (and no more than the device reports)

// A work item is a 16-bit value kept sign-extended in a register: node >= 0 (split axis << 13 | index), leaf < -1
// (0x8000 | first_slot << 2 | count - 1: at most 0xFFF7 = -9), done = -1 -- so "is a node" and "is a leaf" are one signed compare each.
#define LDSK_DONE (-1)
__host__ __device__ inline int32_t ldsk_item(int32_t child) {  // (a node's item still wants its split axis: the caller has the node)
  if (child >= 0) return child;
  return (int32_t)(short)(unsigned short)(0x8000u | (rt::leaf_first(child) << 2) | (rt::leaf_count(child) - 1u));
}

struct LdsKernelLayout {
  uint32_t off_nodes, off_refs, off_spheres, off_moving, off_stacks, off_ring, total;
};
// levels: the tree's height + 1 (the spare one is the stack's sentinel slot); ring_cap: entries of a wave's primary-ray ring
// (0 = no ring; at most 64 = one per lane).  Every region starts on a 16-byte boundary.
__host__ __device__ inline LdsKernelLayout ldsk_layout(uint32_t levels, uint32_t ring_cap, const LdsSceneDims& d) {
  LdsKernelLayout L;
  uint32_t o = LDSK_OFF_NODES;
  L.off_nodes = o; o += (d.n_nodes * d.node_dwords * 4u + 15u) & ~15u;
  L.off_refs = o;  // (no reference array since the records are kept in slot order)
  L.off_spheres = o; o += (d.n_spheres * (uint32_t)sizeof(rt::FlatSphere) + 15u) & ~15u;
  L.off_moving = o; o += (d.n_moving * (uint32_t)sizeof(rt::FlatMovingSphere) + 15u) & ~15u;
  L.off_stacks = o; o += levels * LDSK_LEVEL_BYTES;  // (a multiple of 16: the rings behind it stay aligned)
  L.off_ring = o; o += (LDSK_BLOCK / 64u) * ring_bytes(ring_cap);
  L.total = o;
  return L;
}
