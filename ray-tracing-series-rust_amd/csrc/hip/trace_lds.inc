// k_trace_lds -- the voting kernel for scenes whose geometry fits in LDS (included by render.hip, namespace rtx).
//
// The Book-1 class of scenes (a few hundred spheres under one BVH) is tiny: culling tree, primitive
// references and sphere records together are ~40 KB.  k_trace_vote reads them through L1/L2 on every walk
// step, and with four waves per SIMD the dependent fetch (node -> child node, leaf -> reference -> sphere)
// is what a wave waits on between its VALU bursts.  Here ONE 1024-thread workgroup per CU (16 waves, the same
// occupancy as 4 x 256) copies that geometry into LDS once and walks it there (~64-cycle ds_read instead of
// an L1/L2 round trip); the space comes from sharing one copy among 16 waves and from 16-bit stack entries:
//
//     [ nodes: n x 84 B (108 / 156 B with time-aware boxes) ][ spheres: n x 40 B ][ moving spheres: n x 80 B ]
//     [ walk stacks: levels x 1024 x u16 ][ primary-ray rings: 16 waves x ring_cap (64, or 48 when LDS is tight, else none) x 76 B ]   <= 160 KB
//     (lds_layout.inc: ldsk_layout, the record sizes and the limits)
//
// Work items are 16 bits (axis << 13 | node index, index < 0x2000; or 0x8000 | first_slot << 2 | count - 1); the
// child fields of the LDS copy of the tree are rewritten to that encoding while copying.  A node item carries its
// node's split axis, so a step knows the near child before it has read anything: one LDS round trip, not two.  LDS node records are padded to 17
// dwords: lanes of a wave visit unrelated nodes, and with 64-byte records the same field of every node falls
// into the same two banks, whereas an odd stride spreads a wave's reads over all of them (and keeps every
// field at a compile-time offset from one per-lane base address).  Everything else -- regeneration through the per-wave ring, cost-weighted node/leaf voting, f32 culling, carry-over of straggler walks,
// shading -- is k_trace_vote's logic; results are bit-identical (tests/test_gpu_parity.py).

#define LDSK_NO_REF 0xFFFFFFFFu  // "nothing hit yet" in Closest::ref (primitive type 7 does not exist): k_trace_lds keeps no separate flag
#ifndef LDSK_NODE_BURST
#define LDSK_NODE_BURST 1  // node steps per vote (2 measured: see DESIGN.md 4)
#endif

// Slot 0 of every thread holds LDSK_DONE for the whole kernel (init()), and a walk's own entries start at slot 1: popping an
// "empty" stack returns "done" like any other item -- no emptiness test, no branch (the levels the launcher sizes the stack with
// are the tree's height + 1: the height is what a walk can hold, the spare one is this slot).
//
// LDS by absolute address.  The kernel has no static LDS, so its dynamic block starts at address 0 (the launcher asks the code
// object: plan_lds in render.hip): an address built from integers lets the compiler fold the node array's fixed offset into the index multiply and
// every field into the DS instruction's immediate offset -- through `ldsk + ...` the base is a symbol that is resolved (to 0)
// only after instruction selection, and stays behind as an add of its own.
typedef __attribute__((address_space(3))) unsigned char LdsByte;
typedef __attribute__((address_space(3))) float LdsF32;
typedef __attribute__((address_space(3))) int32_t LdsI32;
typedef __attribute__((address_space(3))) short LdsI16;
typedef __attribute__((address_space(3))) unsigned short LdsU16;
__device__ __forceinline__ const LdsByte* lds_at(uint32_t addr) { return (const LdsByte*)(uintptr_t)addr; }
// What a walk carries is the BYTE ADDRESS of its top entry (`sp`), not a depth: the top is read at that address, a pop reads it
// and steps down by the constant LDSK_LEVEL_BYTES, a push steps up and stores -- no address is rebuilt from a depth in any
// step.  The thread's slot 0 (`bottom`) has the stacks' runtime base folded in once.
struct LdsStack16 {  // slot (level, thread) at bottom + level * LDSK_LEVEL_BYTES
  uint32_t bottom, sp;
  __device__ __forceinline__ void init() { *(LdsU16*)lds_at(bottom) = 0xFFFFu; sp = bottom; }  // 0xFFFF sign-extends to LDSK_DONE
  // empty, then `under` (16 bits, wave-uniform) pushed unless it is "done" -- without a branch: "done" is written over slot 0,
  // which holds it already
  __device__ __forceinline__ void reset_with(uint32_t under) {
    sp = bottom + (under != 0xFFFFu ? LDSK_LEVEL_BYTES : 0u);
    set_top((int32_t)under);
  }
  __device__ __forceinline__ void set_top(int32_t v) { *(LdsU16*)lds_at(sp) = (unsigned short)v; }
  __device__ __forceinline__ void push(int32_t v) { sp += LDSK_LEVEL_BYTES; set_top(v); }
  __device__ __forceinline__ int32_t top() const { return (int32_t)*(const LdsI16*)lds_at(sp); }  // ds_read_i16: sign-extending
  __device__ __forceinline__ int32_t pop() { const int32_t v = top(); sp -= LDSK_LEVEL_BYTES; return v; }
  // a node step's net effect: one level up when both children may be hit (the caller then stores the far one with set_top), one
  // down when neither: hf + hs - 1 levels.  Written as two adds of a bool so that a compare's lane mask goes in as the carry of
  // an add / subtract (v_addc_co / v_subbrev_co) instead of through a 0 / 1 select of its own.
  __device__ __forceinline__ void move(bool hf, bool hs) {
    int32_t d = -1;
    d += (int32_t)hf;
    d += (int32_t)hs;
    sp += (uint32_t)d * LDSK_LEVEL_BYTES;
  }
};
// (the work items these stacks hold: ldsk_item, lds_layout.inc)

// MOTION: time-aware culling boxes (core/flat_types.hpp: FlatMotion32).  Every plane of a child block is followed, 36 bytes on, by
// its slope over the BVH's time interval, and a node step evaluates plane + s * slope (one fma) with the ray's own normalised
// time s before the slab test.  Only launched when the camera's shutter lies inside that interval (render.hip).
// MOTION = 1: slopes for every axis; MOTION = 2 + a: every moving sphere of the scene moves along axis a alone (Book-1 at HEAD: y), so only
// that axis's planes carry slopes -- 4 fmas and 4 LDS dwords per child pair instead of 12 and 12, node records of 27 dwords.
template <uint32_t F, bool RING, uint32_t MOTION, class SM = ShardMap>
__global__ __launch_bounds__(LDSK_BLOCK) void k_trace_lds(rt::SceneView sv, rt::RenderParams rp, SM sm,
                                                          uint32_t s_begin, uint32_t total,
                                                          double* __restrict__ samples, unsigned int* work_counter,
                                                          uint32_t leaf_weight, uint32_t walk_threshold, uint32_t chunk, uint32_t ring_cap,
                                                          uint32_t stack_levels, LdsSceneDims dims, rt::real motion_t0, rt::real motion_inv_dt,
                                                          uint32_t mv_common, rt::real mv_t0, rt::real mv_t1) {
  static_assert(!MOTION || (F & rt::F_MOVING_SPHERE), "time-aware boxes only make sense with moving spheres");
  // the launcher packs four small numbers into one kernel argument: bits 0-7 the walk threshold, bit 8 "every leaf holds one
  // primitive", bits 16-22 and 24-30 the miss-retire rule's D and M (below, at the vote).  With a ring the word stays packed in
  // its ONE scalar register and is unpacked where a number is used, from a copy the compiler cannot see through (as `entry`
  // below): unpacked here, threshold, D and M each held a register for the whole kernel and pushed five other values into lanes
  // of the spill register, read back once per bounce.
  const bool single_leaf = (walk_threshold & 0x100u) != 0u;
  const uint32_t tuning = walk_threshold;
  if (!RING) walk_threshold &= 0xFFu;
  constexpr bool UNI = (F & rt::F_MOVING_SPHERE) != 0;               // static spheres as moving spheres that stand still (see the copy below)
  constexpr uint32_t FL = UNI ? (F & ~rt::F_SPHERE) : F;             // what the leaf tests and the HitRecord are compiled for
  static_assert(MOTION <= 4u, "0: no slopes, 1: all axes, 2 + a: axis a only");
  constexpr uint32_t ND = MOTION == 1u ? LDSK_MOTION_NODE_DWORDS : (MOTION >= 2u ? LDSK_MOTION1_NODE_DWORDS : LDSK_NODE_DWORDS);  // dwords per LDS node record
  constexpr uint32_t CBD = MOTION == 1u ? 19u : (MOTION >= 2u ? 13u : 10u);                                                    // dwords per child block
  constexpr uint32_t MA = MOTION >= 2u ? MOTION - 2u : 0u;                                                                     // the one moving axis
  constexpr uint32_t CB = CBD * 4u;                                             // ... in bytes
  constexpr uint32_t ITEM_OFF = CB - 4u;                                        // the child's work item closes its block
  constexpr uint32_t ROOT_ITEM_DWORD = 2u * CBD;                                // node record 0's dword of padding holds the root's item
  static_assert((F & ~(rt::F_SPHERE | rt::F_MOVING_SPHERE | rt::F_BVH | rt::F_LAMBERTIAN | rt::F_METAL |
                       rt::F_DIELECTRIC | rt::F_CHECKER)) == 0, "k_trace_lds caches spheres and moving spheres only");
  extern __shared__ __attribute__((aligned(16))) unsigned char ldsk[];
  const LdsKernelLayout L = ldsk_layout(stack_levels, RING ? ring_cap : 0u, dims);
  const uint32_t lane = threadIdx.x & 63u;
  const rt::FlatEntry& bvh = sv.entries[sv.top_level[0]];
  // Where every walk enters (lds_entry_pair, lds_variant.inc): the root -- or, under a leaf-first root (Book-1: the ground's leaf
  // beside the tree of everything else), the state the root step leaves for a ray that may hit both children: the leaf in hand,
  // child 1 on stack level 1.  The root step is then not run at all.  A ray it would have spared the leaf finds no root in range
  // in the leaf's exact test; a ray it would have spared child 1 finds both of child 1's boxes culled one step later, a step the
  // wave runs for its other lanes anyway; the tie rule of leaf_test does not ask in which order the leaves came.  The stack is
  // as deep as after the root step, so the sentinel slot and `stack_levels` are what they were.  (Rays with a component that is
  // not finite are the exception: see the bounce begin.)
  // Both items in ONE scalar register, where `root` was (the kernel has no scalar register to spare: a second one costs a VGPR).
  int32_t entry_pair[2];
  lds_entry_pair(sv.nodes32, bvh.a, entry_pair);
  const uint32_t entry = ((uint32_t)entry_pair[0] & 0xFFFFu) | ((uint32_t)entry_pair[1] << 16);  // wave-uniform
  const uint32_t first_ref = (uint32_t)bvh.b;

  // ---- geometry -> LDS
  uint32_t* const lds_nodes = (uint32_t*)(ldsk + LDSK_OFF_NODES);  // [n_nodes][21], see the copy loop below (L.off_nodes is this constant)
  rt::FlatSphere* const lds_spheres = (rt::FlatSphere*)(ldsk + L.off_spheres);
  rt::FlatMovingSphere* const lds_moving = (rt::FlatMovingSphere*)(ldsk + L.off_moving);
  {
    static_assert(sizeof(rt::FlatNode32) == 64 && offsetof(rt::FlatNode32, child) == 48 && offsetof(rt::FlatNode32, axis) == 56,
                  "the padded LDS copy assumes FlatNode32's layout");
    // LDS node record (21 dwords) = two child blocks of 10 dwords + 1 of padding.  A child block holds, per axis a, the triple
    // [lo, hi, lo] at dword 3 a, so that a lane reads (near, far) of that axis as two consecutive dwords at offset `sign of its
    // ray on a` -- no min / max to sort the planes (core/cull32.hpp: cull32_may_hit_nf) -- and the child's work item at dword 9.
    const uint32_t* src = (const uint32_t*)sv.nodes32;
    const uint32_t* msrc = (const uint32_t*)sv.motion32;  // FlatMotion32: lo0[2][3] at 0, hi0 at 6, dlo at 12, dhi at 18
    for (uint32_t k = threadIdx.x; k < dims.n_nodes * 2u * CBD; k += LDSK_BLOCK) {
      const uint32_t node = k / (2u * CBD), field = k - node * (2u * CBD);
      const uint32_t c = field / CBD, r = field - c * CBD;
      uint32_t v;
      if (r < 9u) {
        const uint32_t a = r / 3u, t = r - a * 3u;
        v = MOTION ? msrc[node * 24u + (t == 1u ? 6u : 0u) + c * 3u + a]
                   : src[node * 16u + (t == 1u ? 6u : 0u) + c * 3u + a];  // FlatNode32: lo[2][3] at 0, hi[2][3] at 6
      } else if (MOTION == 1u && r < 18u) {
        const uint32_t a = (r - 9u) / 3u, t = (r - 9u) - a * 3u;
        v = msrc[node * 24u + (t == 1u ? 18u : 12u) + c * 3u + a];
      } else if (MOTION >= 2u && r < 12u) {  // [dlo, dhi, dlo] of the moving axis behind the nine planes
        const uint32_t t = r - 9u;
        v = msrc[node * 24u + (t == 1u ? 18u : 12u) + c * 3u + MA];
      } else {
        const int32_t child = (int32_t)src[node * 16u + 12u + c];
        int32_t item = ldsk_item(child);
        if (child >= 0) item |= sv.nodes32[child].axis << 13;
        v = (uint32_t)item;
      }
      lds_nodes[node * ND + field] = v;
    }
    if (threadIdx.x == 0) lds_nodes[ROOT_ITEM_DWORD] = (uint32_t)(bvh.a | (sv.nodes32[bvh.a].axis << 13));
    // The primitive records ride in LDS IN LEAF-SLOT ORDER: record k is the primitive of slot k of the BVH's reference list, so a
    // leaf step goes from its item straight to the record (no reference fetch: one dependent LDS read less per test, and the
    // reference array -- 2 KB on Book-1, what its ring of 64 was short of -- is not copied at all).  A reference of this kernel
    // is therefore (type, slot), valid against the LDS arrays only (lsv below).
    // UNI (scenes with moving spheres): a static sphere becomes a moving sphere that does not move (c1 = c0: the centre
    // c0 + ratio * (c1 - c0) is c0 exactly) -- so that a leaf step has ONE kind of primitive and one code path; with two kinds a
    // wave ran the sphere test and then the moving-sphere test, each with the lanes of its kind (Book-1 at HEAD: 20 % static,
    // and the ground every ray asks).
    if (UNI) {
      for (uint32_t k = threadIdx.x; k < dims.n_refs; k += LDSK_BLOCK) {
        const rt::PrimRef ref = sv.refs[first_ref + k];
        rt::FlatMovingSphere m;
        if (rt::primref_type(ref) == rt::PRIM_SPHERE) {
          const rt::FlatSphere sp = sv.spheres[rt::primref_index(ref)];
          m.c0[0] = sp.cx; m.c0[1] = sp.cy; m.c0[2] = sp.cz; m.c1[0] = sp.cx; m.c1[1] = sp.cy; m.c1[2] = sp.cz;
          m.time0 = rt::real(0.0); m.time1 = rt::real(1.0); m.radius = sp.radius; m.mat = sp.mat; m.pad = 0;
        } else {
          m = sv.moving_spheres[rt::primref_index(ref)];
        }
        lds_moving[k] = m;
      }
    } else {
      constexpr uint32_t SD = (uint32_t)(sizeof(rt::FlatSphere) / 4);
      uint32_t* ds = (uint32_t*)lds_spheres;
      const uint32_t* ss = (const uint32_t*)sv.spheres;
      for (uint32_t k = threadIdx.x; k < dims.n_refs * SD; k += LDSK_BLOCK) {
        const uint32_t slot = k / SD, field = k - slot * SD;
        ds[k] = ss[rt::primref_index(sv.refs[first_ref + slot]) * SD + field];
      }
    }
  }
  __syncthreads();
  rt::SceneView lsv = sv;  // geometry reads go to LDS; materials and textures stay in global memory
  lsv.spheres = lds_spheres;
  lsv.moving_spheres = lds_moving;

  LdsStack16 stack;
  stack.bottom = (uint32_t)(uintptr_t)(LdsByte*)ldsk + L.off_stacks + threadIdx.x * 2u;
  stack.init();
  double* const ring_f = (double*)(ldsk + L.off_ring + (threadIdx.x >> 6) * ring_bytes(ring_cap));
  uint32_t* const ring_g = (uint32_t*)(ring_f + RING_F64 * ring_cap);
  uint32_t ring_n = 0;                    // wave-uniform
  uint32_t chunk_pos = 0, chunk_end = 0;  // wave-uniform
  bool queue_empty = false;               // wave-uniform
  bool active = false;
  uint32_t g = 0;  // the path's slot of the sample buffer (start_path)
  rt::PathState ps;
  bool midwalk = false;
  rt::Ray32 q = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  uint32_t dir_neg = 0;
  uint32_t off_x = 0, off_y = 12, off_z = 24;  // byte offset of this ray's (near, far) pair of each axis inside a child block
  uint32_t flip_b = 0;  // byte a: CB (the far child's block comes first along axis a for this ray) or 0; byte 3 ("axis 3": child 0 first) is 0
  float t_max32 = 0.f;
  float s32 = 0.f;  // MOTION: the ray's time, normalised to the BVH's interval
  rt::real mv_ratio = rt::real(0.0);  // UNI with one common (time0, time1): (ray.time - time0) / (time1 - time0), per bounce
  int32_t cur = LDSK_DONE;
  rt::Closest best;
  best.t = 0.0; best.ref = LDSK_NO_REF; best.order = 0; best.hit = false;  // (.hit is not used here: see LDSK_NO_REF)

  for (;;) {
    // ---- hand new paths to the lanes without one (see k_trace_vote)
    const unsigned long long need_mask = wave_ballot(!active);
    if (need_mask != 0ull) {
      const uint32_t n_need = (uint32_t)__popcll(need_mask);
      const uint32_t rank = lane_rank(need_mask);
      if (RING) {
#define RING_CAP ring_cap
#define RING_DIAG(mask)
#include "trace_ring.inc"
#undef RING_DIAG
#undef RING_CAP
      } else {
        if (chunk_pos >= chunk_end && !queue_empty) {
          uint32_t base = 0;
          if (lane == 0) base = atomicAdd(work_counter, chunk);
          base = __builtin_amdgcn_readfirstlane(base);
          if (base >= total) {
            queue_empty = true;
          } else {
            chunk_pos = base;
            chunk_end = (total - base < chunk) ? total : base + chunk;
          }
        }
        if (chunk_pos < chunk_end) {
          const uint32_t avail = chunk_end - chunk_pos;
          if (!active && rank < avail) {
            g = start_path(rp, sm, s_begin, chunk_pos + rank, &ps);
            active = true;
          }
          chunk_pos += (n_need < avail) ? n_need : avail;
        }
      }
    }
    if (wave_ballot(active) == 0ull) break;
    // ---- begin a bounce for every lane that is not in the middle of a carried-over walk
    if (active && !midwalk) {
      if (rt::path_bounce_begin(&ps)) {
        store_sample(samples, g, ps.output);
        active = false;
      } else {
        q = rt::make_ray32(ps.ray, rt::ray_t_min(ps.ray));
        dir_neg = rt::ray32_dir_neg(q);  // the planes are picked by it: the slope's sign (core/cull32.hpp)
        off_x = (dir_neg & 1u) << 2; off_y = 12u + ((dir_neg & 2u) << 1); off_z = 24u + (dir_neg & 4u);
        flip_b = ((dir_neg & 1u) * CB) | (((dir_neg >> 1) & 1u) * (CB << 8)) | (((dir_neg >> 2) & 1u) * (CB << 16));
        t_max32 = __builtin_huge_valf();
        if (UNI && mv_common != 0u) mv_ratio = (ps.ray.time - mv_t0) / (mv_t1 - mv_t0);
        if (MOTION) s32 = __builtin_fminf(__builtin_fmaxf((float)((ps.ray.time - motion_t0) * motion_inv_dt), 0.f), 1.f);
        best.t = RT_INFINITY; best.ref = LDSK_NO_REF; best.order = 0;
        // (unpacked HERE, from a copy the compiler cannot see through: hoisted out of the loop, the two items, "is there a second"
        // and the address of level 1 each want a register of their own for the whole kernel)
        uint32_t e = entry;
        asm volatile("" : "+s"(e));
        cur = (int32_t)(short)e;
        stack.reset_with(e >> 16);
        // ... for a ray that is finite in every component.  A box test also rules out rays no primitive test can: with an infinite
        // or NaN component (a frame one pixel wide or high has such primary rays: u = x / 0) the sphere's quadratic has a NaN
        // root, which `root < t_min || t_max < root` lets through, while the box's planes all lie at distance 0 and cull it.
        // Such a lane starts at the root as before.  One number tells: the slopes' product is finite and not 0 (no direction
        // component is 0, infinite or NaN), and adding 0 x (the sum of the origin terms and the time) leaves it so.
        float fin = (q.oix + q.oiy) + q.oiz;
        if (UNI) fin += (float)ps.ray.time;
        if (!__builtin_amdgcn_classf(__builtin_fmaf(fin, 0.f, (q.ix * q.iy) * q.iz), 0x198u)) {  // +- normal or denormal
          cur = *(const LdsI32*)lds_at(LDSK_OFF_NODES + ROOT_ITEM_DWORD * 4u);
          stack.sp = stack.bottom;
        }
        midwalk = true;
      }
    }
    // ---- walk: cost-weighted node/leaf vote with carry-over of stragglers
    const bool no_refill = queue_empty && ring_n == 0u;  // wave-uniform
    uint32_t tn = tuning;
    if (RING) asm volatile("" : "+s"(tn));
    const uint32_t threshold = no_refill ? 1u : (RING ? (tn & 0xFFu) : walk_threshold);
    auto node_step = [&]() {
      // the child that is near along the node's split axis is tested and queued first; which block that is is decided in
      // the ADDRESS (block 1 starts 40 bytes after block 0), not by selecting results afterwards
      const LdsByte* nd = lds_at(LDSK_OFF_NODES + ((uint32_t)cur & 0x1FFFu) * (ND * 4u));
      const uint32_t first_b = __builtin_amdgcn_ubfe(flip_b, ((uint32_t)cur >> 10) & 0x18u, 8u);  // byte `axis` of flip_b: 0 or CB
      const LdsByte* bf = nd + first_b;         // near child's block
      const LdsByte* bs = nd + (CB - first_b);  // far child's block
      const LdsF32 *fx = (const LdsF32*)(bf + off_x), *fy = (const LdsF32*)(bf + off_y), *fz = (const LdsF32*)(bf + off_z);
      const LdsF32 *sx = (const LdsF32*)(bs + off_x), *sy = (const LdsF32*)(bs + off_y), *sz = (const LdsF32*)(bs + off_z);
      int32_t top = stack.top();
      bool hf, hs;
      if (MOTION >= 2u) {  // one moving axis: its slope pair sits at dword 9 of the block, i.e. 9 - 3 MA dwords after its plane pair
        constexpr uint32_t SO = 9u - 3u * MA;
        const auto* fm = MA == 0u ? fx : (MA == 1u ? fy : fz);
        const auto* sm = MA == 0u ? sx : (MA == 1u ? sy : sz);
        const float fn = __builtin_fmaf(s32, fm[SO], fm[0]), ff = __builtin_fmaf(s32, fm[SO + 1u], fm[1]);
        const float sn = __builtin_fmaf(s32, sm[SO], sm[0]), sf = __builtin_fmaf(s32, sm[SO + 1u], sm[1]);
        hf = rt::cull32_may_hit_nf_pos(MA == 0u ? fn : fx[0], MA == 0u ? ff : fx[1], MA == 1u ? fn : fy[0], MA == 1u ? ff : fy[1],
                                       MA == 2u ? fn : fz[0], MA == 2u ? ff : fz[1], q, t_max32);
        hs = rt::cull32_may_hit_nf_pos(MA == 0u ? sn : sx[0], MA == 0u ? sf : sx[1], MA == 1u ? sn : sy[0], MA == 1u ? sf : sy[1],
                                       MA == 2u ? sn : sz[0], MA == 2u ? sf : sz[1], q, t_max32);
      } else if (MOTION) {  // plane(s) = plane0 + s * slope; the slopes sit 9 dwords after their planes
        hf = rt::cull32_may_hit_nf_pos(__builtin_fmaf(s32, fx[9], fx[0]), __builtin_fmaf(s32, fx[10], fx[1]), __builtin_fmaf(s32, fy[9], fy[0]),
                                   __builtin_fmaf(s32, fy[10], fy[1]), __builtin_fmaf(s32, fz[9], fz[0]), __builtin_fmaf(s32, fz[10], fz[1]), q, t_max32);
        hs = rt::cull32_may_hit_nf_pos(__builtin_fmaf(s32, sx[9], sx[0]), __builtin_fmaf(s32, sx[10], sx[1]), __builtin_fmaf(s32, sy[9], sy[0]),
                                   __builtin_fmaf(s32, sy[10], sy[1]), __builtin_fmaf(s32, sz[9], sz[0]), __builtin_fmaf(s32, sz[10], sz[1]), q, t_max32);
      } else {
        hf = rt::cull32_may_hit_nf_pos(fx[0], fx[1], fy[0], fy[1], fz[0], fz[1], q, t_max32);
        hs = rt::cull32_may_hit_nf_pos(sx[0], sx[1], sy[0], sy[1], sz[0], sz[1], q, t_max32);
      }
      int32_t cf = *(const LdsI32*)(bf + ITEM_OFF), cs = *(const LdsI32*)(bs + ITEM_OFF);
      // the three candidates for the next item are READ AHEAD, beside the planes: an empty statement that "uses" them keeps the
      // compiler from sinking each read behind the compare that selects it (a dependent LDS round trip at the end of every step)
      asm volatile("" : "+v"(top), "+v"(cf), "+v"(cs));
      // next item without a branch: the near child if it may be hit (the far one is stacked if it may be too), else the
      // far child, else the top of the stack -- read ahead of the tests, and LDSK_DONE when the walk's own entries are used up
      const bool both = hf && hs;
      // (selects and pointer update in the block of the compares, the one predicated store behind them: the sign extension of
      // `top` folds into its read and the two masks into the pointer arithmetic only where the compiler sees them side by side)
      cur = hf ? cf : (hs ? cs : top);
      stack.move(hf, hs);
      if (both) stack.set_top(cs);
    };
    auto leaf_test = [&](uint32_t slot) {
      const rt::PrimRef ref = rt::make_primref(UNI ? rt::PRIM_MOVING_SPHERE : rt::PRIM_SPHERE, slot);  // record k = slot k (see the copy)
      rt::real t;
      bool ok;
      if (UNI && mv_common != 0u) {
        // every record is a moving sphere and all of them share one (time0, time1): MovingSphere::get_center's
        // (time - time0) / (time1 - time0) (hit.rs:275-278) is the same number for every test of this ray -- divided once
        // per bounce (`mv_ratio`) instead of once per leaf test.  Same operands, same quotient.
        const rt::FlatMovingSphere& sp = lds_moving[slot];
        const rt::Point3 c0 = rt::load_v3(sp.c0), c1 = rt::load_v3(sp.c1);
        ok = rt::sphere_root(c0 + mv_ratio * (c1 - c0), sp.radius, ps.ray, rt::ray_t_min(ps.ray), best.t, &t);
      } else {
        ok = rt::prim_t<FL, false>(lsv, ref, ps.ray, rt::ray_t_min(ps.ray), best.t, &t, nullptr);
      }
      // offer_prim's tie rule (core/geometry.hpp) without its "was anything hit" flag: best.order is 0 until something is
      // hit, and no slot is below 0 -- one loop-carried lane mask less for every step of the walk
      if (ok && !(t == best.t && slot < best.order)) { best.t = t; best.ref = ref; best.order = slot; }
    };
    // The vote closes the loop instead of opening it: the ballots are convergent operations, which the compiler will not duplicate
    // to rotate the loop itself, and an exit test at the head of a loop with divergent regions inside becomes a "stop" lane mask
    // carried to the latch.  At the latch the wave-uniform compare is the back edge's own condition (s_cmp + s_cbranch_scc).
    //
    // Miss retire (RING only; DESIGN.md 4, item 17).  A round ends when fewer than `threshold` lanes still walk, and until then a
    // lane whose walk found nothing waits for a shading block of which it needs five operations and a store.  With D != 0 the
    // loop's exit compare gets a per-round right-hand side, max(threshold, walkers at this entry - D): the walkers are
    // wave-uniform already, so a step gets no new ballot.  When the loop leaves above `threshold` the round is not over: only
    // the finished MISSES pass the shading block (its miss branch), store and go inactive, the next outer iteration hands them
    // rays from the ring and votes on with a new right-hand side; finished hits wait as they are, in the state they have
    // between the loop's exit and the shading block anyway.  One ballot at that exit skips the pass when fewer than M lanes
    // would retire: the misses wait too, and the next exit point lies D lanes further.  Off when no refill is possible
    // (`no_refill`: the threshold is 1 then and a round ends as a whole) and for D = 0.
    bool round_over = true;
    {
      // cur == LDSK_DONE whenever a lane is not in a walk, so the item alone tells the lane's state
      bool is_node = cur >= 0;
      bool is_leaf = cur < -1;
      uint32_t n_node = (uint32_t)__popcll(wave_ballot(is_node)), n_leaf = (uint32_t)__popcll(wave_ballot(is_leaf));
      // (the launcher sends "off" as D = 127: no wave has that many walkers, and neither has one that cannot refill)
      int32_t exit_at = (int32_t)threshold;
      if (RING) exit_at = max(exit_at, (int32_t)(n_node + n_leaf) - (int32_t)(no_refill ? 127u : ((tn >> 16) & 0x7Fu)));
      if (n_node + n_leaf >= (uint32_t)exit_at) {
        do {
          if (n_node * leaf_weight >= n_leaf) {
            if (is_node) node_step();
#if LDSK_NODE_BURST >= 2
            if (cur >= 0) node_step();  // a second node step without a vote in between (the lanes that left for a leaf sit it out)
#endif
          } else {
            if (is_leaf) {
              const uint32_t f = ((uint32_t)cur & 0x7FFFu) >> 2;
              if (single_leaf) {  // wave-uniform: every leaf of this tree holds one primitive -- no loop
                leaf_test(f);
              } else {
                const uint32_t k = ((uint32_t)cur & 3u) + 1u;
                for (uint32_t i = 0; i < k; ++i) leaf_test(f + i);
              }
              t_max32 = rt::cull_round_up(best.t);
              cur = stack.pop();
            }
          }
          is_node = cur >= 0;
          is_leaf = cur < -1;
          n_node = (uint32_t)__popcll(wave_ballot(is_node));
          n_leaf = (uint32_t)__popcll(wave_ballot(is_leaf));
        } while (n_node + n_leaf >= (uint32_t)exit_at);
      }
      if (RING) round_over = n_node + n_leaf < threshold;
    }
    // ---- shade the lanes whose walk is complete; in a round that is not over, the misses among them (if there are M)
    bool shade = midwalk && cur == LDSK_DONE;
    if (!round_over) {
      shade = shade && best.ref == LDSK_NO_REF;
      uint32_t tm = tuning;
      asm volatile("" : "+s"(tm));
      if ((uint32_t)__popcll(wave_ballot(shade)) < (tm >> 24)) shade = false;
    }
    if (shade) {
      midwalk = false;
      rt::HitRecord rec;
      const bool hit = best.ref != LDSK_NO_REF;
      if (hit) rt::prim_finalize<FL>(lsv, best.ref, ps.ray, best.t, &rec);
      if (rt::path_bounce_end<F, false>(sv, rp, &ps, hit, rec, nullptr)) {
        store_sample(samples, g, ps.output);
        active = false;
      }
    }
  }
}
