// The voting walk: node / leaf steps, the 4-wide culling tree and k_trace_vote (included by render.hip,
// namespace rtx).

// ---- wave-synchronous BVH walk with deferred leaves --------------------------------------------
// In bvh_step a leaf child is intersected inline, i.e. inside a branch only the lanes that reached
// a leaf take, while the rest of the wave waits -- on every step.  Here a leaf is just another work
// item: an item is a node (code >= 0) or a leaf (code < 0); a node step tests the node's two child
// boxes and only QUEUES hit children (near one becomes the current item, far one goes on the LDS
// stack), a leaf step intersects the leaf's primitives.  Each iteration the wave votes (__ballot)
// and runs the kind of step most of its lanes are waiting for, so both bodies run well filled.
// Visiting order differs from bvh_step; the closest hit (with its tie rule) does not.
#define WALK_DONE 0x7fffffff
template <uint32_t F>
__device__ __forceinline__ void walk_node_step(const rt::SceneView& sv, const rt::Ray& r, rt::Vec3 inv_d,
                                               uint32_t dir_neg, rt::real t_min, rt::real best_t,
                                               int32_t* cur, LdsStack& stack) {
  const rt::FlatNode& n = sv.nodes[*cur];
  int first = (int)((dir_neg >> (uint32_t)n.pad[0]) & 1u);
  bool hf = rt::aabb_may_hit(n.bmin[first], n.bmax[first], r.origin, inv_d, t_min, best_t);
  bool hs = rt::aabb_may_hit(n.bmin[1 - first], n.bmax[1 - first], r.origin, inv_d, t_min, best_t);
  int32_t cf = n.child[first], cs = n.child[1 - first];
  if (hf) {
    *cur = cf;
    if (hs) stack.push(cs);
  } else if (hs) {
    *cur = cs;
  } else {
    *cur = stack.empty() ? WALK_DONE : stack.pop();
  }
}
// Node step on the f32 culling tree (core/cull32.hpp): cheaper per step (2-cycle f32 issue, 64-B
// node) and, being conservative, invisible in the result.
template <class STACK>
__device__ __forceinline__ void walk_node_step32(const rt::FlatNode32& n, const rt::Ray32& q, uint32_t dir_neg,
                                                 float t_max32, int32_t* cur, STACK& stack) {
  int first = (int)((dir_neg >> (uint32_t)n.axis) & 1u);
  bool hf, hs;
  rt::cull32_may_hit2(n.lo[first], n.hi[first], n.lo[1 - first], n.hi[1 - first], q, t_max32, &hf, &hs);
  int32_t cf = n.child[first], cs = n.child[1 - first];
  if constexpr (STACK::kBottom) {  // no branch: near child, else far child, else the top of the stack (read ahead)
    const int32_t top = stack.top();
    const bool both = hf && hs;
    if (both) stack.base[stack.n * TRACE_BLOCK] = cs;
    *cur = hf ? cf : (hs ? cs : top);
    stack.n += (int)both - (int)!(hf || hs);
  } else if (hf) {
    *cur = cf;
    if (hs) stack.push(cs);
  } else if (hs) {
    *cur = cs;
  } else {
    *cur = stack.empty() ? WALK_DONE : stack.pop();
  }
}
// tri_base >= 0: the BVH holds triangles only and slot s is triangle tri_base + s (the flattener stores a mesh's
// triangles in leaf order), so the primitive reference need not be fetched.
// A stack with a bottom (LdsStackB) marks the resident kernels, which also keep no "anything hit" flag in their walk loops:
// Closest::ref stays WALK_NO_REF until a primitive is hit (one loop-carried lane mask less for every step), Closest::hit is
// not maintained, and offer_prim's tie rule needs no flag -- Closest::order is 0 until something is hit and no slot is below 0.
#define WALK_NO_REF 0xFFFFFFFFu  // primitive type 7 does not exist
template <uint32_t F, class STACK>
__device__ __forceinline__ void walk_leaf_step(const rt::SceneView& sv, uint32_t first_ref, const rt::Ray& r,
                                               rt::real t_min, rt::Closest* best, int32_t* cur, STACK& stack,
                                               int32_t tri_base = -1) {
  uint32_t f = rt::leaf_first(*cur), k = rt::leaf_count(*cur);
  for (uint32_t i = 0; i < k; ++i) {
    const rt::PrimRef ref = ((F & rt::F_TRIANGLE) && tri_base >= 0)
                                ? rt::make_primref(rt::PRIM_TRIANGLE, (uint32_t)tri_base + f + i)
                                : sv.refs[first_ref + f + i];
    if constexpr (STACK::kBottom) {
      rt::real t;
      if (rt::prim_t<F, false>(sv, ref, r, t_min, best->t, &t, nullptr) && !(t == best->t && f + i < best->order)) {
        best->t = t; best->ref = ref; best->order = f + i;
      }
    } else {
      rt::offer_prim<F, false>(sv, ref, f + i, r, t_min, best, nullptr);
    }
  }
  if constexpr (STACK::kBottom) *cur = stack.pop();
  else *cur = stack.empty() ? WALK_DONE : stack.pop();
}

// ------------------------------------------------------------------ 4-wide culling tree (big meshes)
// FlatNode4, the host collapse that builds it (build_wide_nodes) and the stack sizing live in host/wide_tree.hpp.

// One wide step: test the four child boxes, push the hit ones so that the nearest ends on top, pop it.
// The near / far plane of every axis is picked by the sign of the ray's direction THROUGH THE ADDRESS: `sign_pack` holds, per
// axis, the byte offset inside the node record of the float4 of near planes (x: 0 or 48, y: 16 or 64, z: 32 or 80; the far
// planes sit at 48 - x, 80 - y, 112 - z).  For a finite slope near = min and far = max of the two plane distances, so tn / tf
// are the numbers the min / max form computes (and NaNs of a zero slope are dropped by fmaxf / fminf either way): same
// verdicts, same order, same walk -- without the six v_min / v_max per box that only sorted the planes (4 clocks each on gfx950).
// The sign is the direction's SIGN BIT, which is the sign bit of the slope the planes are multiplied by (narrowing to f32 and a
// reciprocal both keep it; rt::ray32_dir_neg says why `d < 0` is not enough: -0.0).  Taken from the direction rather than from
// the Ray32 because that is what cost nothing: a compare on the slope made k_trace_world 0.7 % slower on Book-2 (DESIGN.md 5.6).
__device__ __forceinline__ uint32_t wide_sign_pack(const rt::Ray& r) {
  const uint32_t nx = rt::real_sign_bit(r.direction.x) * 48u, ny = 16u + rt::real_sign_bit(r.direction.y) * 48u, nz = 32u + rt::real_sign_bit(r.direction.z) * 48u;
  return nx | (ny << 8) | (nz << 16);
}
// The key a wide step sorts a child by: the slab entry distance clamped into [t_min, 3e38].  The clamp is what keeps the
// ranking below well defined for every ray: an entry distance of +inf (a direction component of exactly 0 -- rare in f64
// rays narrowed to f32, common in f32 rays -- or an origin that overflowed) would tie with the +inf that marks a missed
// child, and a NaN would compare false both ways; either breaks the "ranks are a permutation" property and leaves a stack
// slot unwritten.  v_med3_f32 returns min3 of its operands when one of them is a NaN (tests/test_gpu_f32.py pins that
// through rtx_device_math): a NaN entry distance becomes t_min.
__device__ __forceinline__ float wide_key(float entry, float t_min) { return __builtin_amdgcn_fmed3f(entry, t_min, 3.0e38f); }
__device__ __forceinline__ bool slab_interval_nf(float nx, float fx, float ny, float fy, float nz, float fz, const rt::Ray32& q,
                                                 float t_max32, float* t_near) {
  const float tn = wide_key(__builtin_fmaxf(__builtin_fmaxf(__builtin_fmaf(nx, q.ix, -q.oix), __builtin_fmaf(ny, q.iy, -q.oiy)),
                                            __builtin_fmaf(nz, q.iz, -q.oiz)), q.t_min);
  const float tf = __builtin_fminf(__builtin_fminf(__builtin_fminf(__builtin_fmaf(fx, q.ix, -q.oix), __builtin_fmaf(fy, q.iy, -q.oiy)),
                                                   __builtin_fmaf(fz, q.iz, -q.oiz)), t_max32);
  *t_near = tn;
  return !(tn - tf > __builtin_fmaf(__builtin_fabsf(tn) + __builtin_fabsf(tf), 0x1.0p-21f, q.err2));  // as cull32_may_hit
}
template <class STACK>
__device__ __forceinline__ void walk_node_step4(const FlatNode4* __restrict__ nodes4, const rt::Ray32& q, uint32_t sign_pack, float t_max32,
                                                int32_t* cur, STACK& stack) {
  const unsigned char* base = (const unsigned char*)&nodes4[*cur];
  const uint32_t ox = sign_pack & 0xffu, oy = (sign_pack >> 8) & 0xffu, oz = sign_pack >> 16;
  const float4 nx = *(const float4*)(base + ox), fx = *(const float4*)(base + (48u - ox));
  const float4 ny = *(const float4*)(base + oy), fy = *(const float4*)(base + (80u - oy));
  const float4 nz = *(const float4*)(base + oz), fz = *(const float4*)(base + (112u - oz));
  const int4 ch = *(const int4*)(base + 96);
  float k0, k1, k2, k3;
  const bool h0 = slab_interval_nf(nx.x, fx.x, ny.x, fy.x, nz.x, fz.x, q, t_max32, &k0) && ch.x != WALK_DONE;
  const bool h1 = slab_interval_nf(nx.y, fx.y, ny.y, fy.y, nz.y, fz.y, q, t_max32, &k1) && ch.y != WALK_DONE;
  const bool h2 = slab_interval_nf(nx.z, fx.z, ny.z, fy.z, nz.z, fz.z, q, t_max32, &k2) && ch.z != WALK_DONE;
  const bool h3 = slab_interval_nf(nx.w, fx.w, ny.w, fy.w, nz.w, fz.w, q, t_max32, &k3) && ch.w != WALK_DONE;
  const float inf = __builtin_huge_valf();
  k0 = h0 ? k0 : inf; k1 = h1 ? k1 : inf; k2 = h2 ? k2 : inf; k3 = h3 ? k3 : inf;
  // rank = number of children that come before this one (ties: lower slot first); hits rank 0 .. nh-1
  const int b10 = k1 < k0, b20 = k2 < k0, b30 = k3 < k0, b21 = k2 < k1, b31 = k3 < k1, b32 = k3 < k2;
  const int r0 = b10 + b20 + b30;
  const int r1 = (1 - b10) + b21 + b31;
  const int r2 = (1 - b20) + (1 - b21) + b32;
  const int r3 = (1 - b30) + (1 - b31) + (1 - b32);
  const int nh = (int)h0 + (int)h1 + (int)h2 + (int)h3;
  if constexpr (STACK::kBottom) {
    // No condition and no read-back.  The ranks are a permutation of 0..3 with the hits in front.  The nearest hit (rank 0) is
    // the next item and never needs a slot; the other hits go to slots n .. n + nh - 2, farthest lowest.  The nearest hit and
    // every miss are stored too -- four unconditional stores -- into slot n + nh - 1, which is dead: the first free slot when
    // something was hit, and when nothing was, the old top, which was read ahead of the tests and is the next item.
    const int32_t top = stack.top();
    const int last = stack.n + nh - 1;
    stack.base[(last - (h0 ? r0 : 0)) * TRACE_BLOCK] = ch.x;
    stack.base[(last - (h1 ? r1 : 0)) * TRACE_BLOCK] = ch.y;
    stack.base[(last - (h2 ? r2 : 0)) * TRACE_BLOCK] = ch.z;
    stack.base[(last - (h3 ? r3 : 0)) * TRACE_BLOCK] = ch.w;
    const int32_t nearest = r0 == 0 ? ch.x : (r1 == 0 ? ch.y : (r2 == 0 ? ch.z : ch.w));
    *cur = nh > 0 ? nearest : top;
    stack.n = last;
  } else {
    const int top = stack.n + nh - 1;  // the nearest hit goes here
    if (h0) stack.base[(top - r0) * TRACE_BLOCK] = ch.x;
    if (h1) stack.base[(top - r1) * TRACE_BLOCK] = ch.y;
    if (h2) stack.base[(top - r2) * TRACE_BLOCK] = ch.z;
    if (h3) stack.base[(top - r3) * TRACE_BLOCK] = ch.w;
    stack.n += nh;
    *cur = stack.empty() ? WALK_DONE : stack.pop();
  }
}

// Persistent waves with path regeneration and the deferred-leaf walk, for worlds that are one BVH.  Waves pull
// TRACE_CHUNK-item chunks of the pass's index space (pass_items.inc) from a global counter and hand items to their lanes
// as lanes finish paths: the lanes without a path are compacted with a 64-bit __ballot and ranked with mbcnt (the
// wavefront prefix sum), and take consecutive items (= consecutive pixels of one sample: coherent camera rays).  A lane
// therefore never idles while the queue has work, whatever the length of its neighbours' paths.
// DIAG: per-region occupancy counters (diag[2k] = times the wave executed region k, diag[2k+1] = lanes
// active in it); regions: 0 outer iteration, 1 regenerate, 2 node step, 3 leaf step, 4 shade (hit lanes),
// 5 shade (all walking lanes).  Diagnostic build only (RTX_TRACE_KERNEL=vote_diag); never timed.
//
// RING: primary rays are produced 64 at a time into the wave's ring in LDS instead of every outer iteration for just the
// ~20 lanes whose path had ended (trace_ring.inc; layout and size: pass_items.inc).  Which lane traces a sample is
// invisible in the result.
// (VoteTop, the plain entries beside the BVH as a kernel argument, is declared in render.hip next to DeviceScene.)
template <uint32_t F, bool DIAG, bool RING, bool WIDE, class SM = ShardMap>
__global__ __launch_bounds__(TRACE_BLOCK, 4) void k_trace_vote(rt::SceneView sv, rt::RenderParams rp,
                                                            SM sm, uint32_t s_begin, uint32_t total,
                                                            double* __restrict__ samples,
                                                            unsigned int* work_counter,
                                                            unsigned long long* diag, uint32_t leaf_weight,
                                                            uint32_t walk_threshold, uint32_t stack_levels, uint32_t bvh_pos,
                                                            const FlatNode4* __restrict__ nodes4, int32_t tri_base,
                                                            uint32_t lds_tables, VoteTop top) {
  unsigned long long dg[12];
  if (DIAG) for (int k = 0; k < 12; ++k) dg[k] = 0;
  extern __shared__ int32_t lds_stack[];
  LdsStackB stack;
  stack.base = lds_stack + threadIdx.x;
  stack.init();
  const uint32_t lane = threadIdx.x & 63u;
  // Worlds with a handful of materials (the mesh room: 8) keep the material and texture records in LDS behind the stacks
  // (and the ring): every shading fetches material -> texture, two dependent per-lane loads.  lds_tables = materials | textures << 16.
  if (lds_tables != 0u) {
    uint32_t* const dst = (uint32_t*)(lds_stack + stack_levels * TRACE_BLOCK) + (RING ? (TRACE_BLOCK / 64u) * (ring_bytes(64) / 4u) : 0u);
    const uint32_t mw = (lds_tables & 0xffffu) * (uint32_t)(sizeof(rt::FlatMaterial) / 4u), tw = (lds_tables >> 16) * (uint32_t)(sizeof(rt::FlatTexture) / 4u);
    const uint32_t* const ms = (const uint32_t*)sv.materials;
    const uint32_t* const ts = (const uint32_t*)sv.textures;
    for (uint32_t k = threadIdx.x; k < mw; k += TRACE_BLOCK) dst[k] = ms[k];
    for (uint32_t k = threadIdx.x; k < tw; k += TRACE_BLOCK) dst[mw + k] = ts[k];
    __syncthreads();
    sv.materials = (const rt::FlatMaterial*)dst;
    sv.textures = (const rt::FlatTexture*)(dst + mw);
  }
  // the launcher packs two thresholds into one argument: walk (low 16 bits) and regeneration (high 16 bits, at least 1)
  const uint32_t regen_min = (walk_threshold >> 16) ? (walk_threshold >> 16) : 1u;
  walk_threshold &= 0xffffu;
  // this wave's ring of ready primary rays (pass_items.inc)
  double* const ring_f = (double*)((unsigned char*)(lds_stack + stack_levels * TRACE_BLOCK) +
                                   (threadIdx.x >> 6) * ring_bytes(64));
  uint32_t* const ring_g = (uint32_t*)(ring_f + RING_F64 * 64);
  uint32_t ring_n = 0;                    // wave-uniform: entries in the ring (a stack)
  const rt::FlatEntry& bvh = sv.entries[sv.top_level[bvh_pos]];
  const int32_t root = bvh.a;
  const uint32_t first_ref = (uint32_t)bvh.b;
  constexpr uint32_t chunk = TRACE_CHUNK;  // items per claim
  uint32_t chunk_pos = 0, chunk_end = 0;  // wave-uniform
  bool queue_empty = false;               // wave-uniform
  bool active = false;
  uint32_t g = 0;  // the path's slot of the sample buffer (start_path)
  rt::PathState ps;
  // walk state, kept across outer iterations so an unfinished walk can be carried over
  bool midwalk = false;
  rt::Ray32 q = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  uint32_t dir_neg = 0;
  float t_max32 = 0.f;
  int32_t cur = WALK_DONE;
  rt::Closest best;
  best.t = 0.0; best.ref = WALK_NO_REF; best.order = 0; best.hit = false;  // (.hit is not maintained in this kernel: WALK_NO_REF)
  int32_t win_rect = -1;    // axis | material << 2 of the winning rectangle of the kernarg table (-1: the winner is not one)
  uint32_t diag_steps = 0;  // DIAG: node steps of this lane's current walk (a walk that visits the whole tree is reported)
  for (;;) {
    unsigned long long need_mask = wave_ballot(!active);
    if (RING) {
      if (need_mask != 0ull) {
        const uint32_t n_need = (uint32_t)__popcll(need_mask);
        const uint32_t rank = lane_rank(need_mask);
#define RING_CAP 64u
#define RING_DIAG(mask) DIAG_ADD(1, mask)
#include "trace_ring.inc"
#undef RING_DIAG
#undef RING_CAP
      }
    } else if ((uint32_t)__popcll(need_mask) >= regen_min) {  // regeneration is ~600 VALU: it waits until enough lanes want it
      if (chunk_pos >= chunk_end && !queue_empty) {
        const uint32_t base = queue_claim(work_counter, TRACE_CHUNK);
        if (base >= total) {
          queue_empty = true;
        } else {
          chunk_pos = base;
          chunk_end = (total - base < TRACE_CHUNK) ? total : base + TRACE_CHUNK;
        }
      }
      if (chunk_pos < chunk_end) {
        uint32_t rank = lane_rank(need_mask);
        uint32_t n_need = (uint32_t)__popcll(need_mask);
        uint32_t avail = chunk_end - chunk_pos;
        DIAG_ADD(1, wave_ballot(!active && rank < avail));
        if (!active && rank < avail) {
          g = start_path<WIDE>(rp, sm, s_begin, chunk_pos + rank, &ps);
          active = true;
        }
        chunk_pos += (n_need < avail) ? n_need : avail;
      }
    }
    if (wave_ballot(active) == 0ull) break;
    DIAG_ADD(0, wave_ballot(active));
    // ---- begin a bounce for every lane that is not in the middle of a carried-over walk
    if (active && !midwalk) {
      if (rt::path_bounce_begin(&ps)) {
        store_sample(samples, g, ps.output);
        active = false;
      } else {
        q = rt::make_ray32(ps.ray, rt::ray_t_min(ps.ray));
        dir_neg = WIDE ? wide_sign_pack(ps.ray) : rt::ray_dir_neg(ps.ray);  // wide walks keep their plane offsets in this register
        t_max32 = __builtin_huge_valf();
        best.t = RT_INFINITY; best.ref = WALK_NO_REF; best.order = 0;
        stack.reset();
        cur = root;
        midwalk = true;
        diag_steps = 0;
      }
    }
    // ---- walk: cost-weighted node/leaf vote.  The loop stops as soon as fewer than `walk_threshold`
    // lanes are still walking: the stragglers keep their walk state and continue next round, so the
    // wave never waits for the longest walk of a bounce (all remaining ones once the queue is empty).
    const uint32_t threshold = (queue_empty && ring_n == 0u) ? 1u : walk_threshold;
    for (;;) {
      // cur == WALK_DONE whenever a lane is not in a walk, so the item alone tells the lane's state
      bool is_leaf = cur < 0;
      bool is_node = (uint32_t)cur < (uint32_t)WALK_DONE;
      unsigned long long m_node = wave_ballot(is_node), m_leaf = wave_ballot(is_leaf);
      if ((uint32_t)__popcll(m_node | m_leaf) < threshold) break;
      if ((uint32_t)__popcll(m_node) * leaf_weight >= (uint32_t)__popcll(m_leaf)) {
        DIAG_ADD(2, m_node);
        if (is_node) {
          if (WIDE) walk_node_step4(nodes4, q, dir_neg, t_max32, &cur, stack);
          else walk_node_step32(sv.nodes32[cur], q, dir_neg, t_max32, &cur, stack);
          if (DIAG && ++diag_steps == 50000u && atomicAdd(&diag[12], 1ull) == 0ull) {  // the first runaway walk: its ray
            const float v[12] = {(float)ps.ray.origin.x, (float)ps.ray.origin.y, (float)ps.ray.origin.z, (float)ps.ray.direction.x,
                                 (float)ps.ray.direction.y, (float)ps.ray.direction.z, q.ix, q.iy, q.iz, q.err2, q.t_min, t_max32};
            for (int k = 0; k < 6; ++k) diag[13 + k] = (unsigned long long)__float_as_uint(v[2 * k]) | ((unsigned long long)__float_as_uint(v[2 * k + 1]) << 32);
            diag[19] = (unsigned long long)(uint32_t)ps.depth;
          }
        }
      } else {
        DIAG_ADD(3, m_leaf);
        if (is_leaf) {
          walk_leaf_step<F>(sv, first_ref, ps.ray, rt::ray_t_min(ps.ray), &best, &cur, stack, tri_base);
          t_max32 = rt::cull_round_up(best.t);
        }
      }
    }
    // ---- shade the lanes whose walk is complete
    const bool finished = midwalk && cur == WALK_DONE;
    DIAG_ADD(4, wave_ballot(finished && best.ref != WALK_NO_REF));
    DIAG_ADD(5, wave_ballot(finished));
    if (finished) {
      midwalk = false;
      bool hit = best.ref != WALK_NO_REF;
      if (F & rt::F_PRIM_ENTRY) {
        // Plain primitives beside the BVH in the top-level list (the dragon room's seven rectangles): tested here,
        // after the walk, in list order.  HittableList::hit (hit.rs:660-690) lets the LATER entry win an exact
        // tie, wherever the BVH sits in the list; everything else about a closest hit is order independent.
        int32_t win_entry = hit ? (int32_t)bvh_pos : -1;
        win_rect = -1;
        if ((F & rt::F_RECT) && top.n >= 0) {  // all of them rectangles, records in the kernarg segment
          for (int i = 0; i < top.n; ++i) {
            const int32_t k = dev_load_uniform(&top.k[i]);
            rt::FlatRect q;
            q.a0 = dev_load_uniform(&top.rect[i].a0); q.a1 = dev_load_uniform(&top.rect[i].a1);
            q.b0 = dev_load_uniform(&top.rect[i].b0); q.b1 = dev_load_uniform(&top.rect[i].b1);
            q.k = dev_load_uniform(&top.rect[i].k); q.axis = dev_load_uniform(&top.rect[i].axis); q.mat = 0;
            rt::real t;
            if (rt::rect_t(q, ps.ray, rt::ray_t_min(ps.ray), best.t, &t)) {
              if (t < best.t || win_entry < k) {
                best.t = t; best.ref = (rt::PrimRef)dev_load_uniform(&top.ref[i]); hit = true; win_entry = k;
                win_rect = q.axis | (dev_load_uniform(&top.rect[i].mat) << 2);  // what the HitRecord needs of the winner
              }
            }
          }
        } else {
          for (int32_t k = 0; k < sv.n_top_level; ++k) {
            if (k == (int32_t)bvh_pos) continue;
            const rt::FlatEntry* e = &sv.entries[dev_load_uniform(&sv.top_level[k])];
            const rt::PrimRef ref = (rt::PrimRef)dev_load_uniform(&e->a);
            rt::real t;
            if (rt::prim_t<F, false>(sv, ref, ps.ray, rt::ray_t_min(ps.ray), best.t, &t, nullptr)) {
              if (t < best.t || win_entry < k) { best.t = t; best.ref = ref; hit = true; win_entry = k; }
            }
          }
        }
      }
      rt::HitRecord rec;
      if (!(F & rt::F_IMAGE) && (F & rt::F_PRIM_ENTRY) && win_rect >= 0) {
        // a rectangle of the kernarg table won: its record need not be fetched again (hit.rs:486-500, 551-565, 616-630; uv unused)
        const int32_t axis = win_rect & 3;
        rec.t = best.t;
        rec.p = rt::ray_at(ps.ray, best.t);
        rec.u = 0.0; rec.v = 0.0;
        rt::create_normal_face(ps.ray, axis == rt::RECT_XY ? rt::v3(0, 0, 1) : (axis == rt::RECT_XZ ? rt::v3(0, 1, 0) : rt::v3(1, 0, 0)), &rec.normal, &rec.front_face);
        rec.mat = win_rect >> 2;
      } else if (hit) rt::prim_finalize<F>(sv, best.ref, ps.ray, best.t, &rec);
      if (rt::path_bounce_end<F, false>(sv, rp, &ps, hit, rec, nullptr)) {
        store_sample(samples, g, ps.output);
        active = false;
      }
    }
  }
  if (DIAG) {
    if (lane == 0)
      for (int k = 0; k < 12; ++k) atomicAdd(&diag[k], dg[k]);
  }
}

