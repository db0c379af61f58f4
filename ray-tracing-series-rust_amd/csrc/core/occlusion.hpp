// Occlusion of a segment: the any-hit walk of the world list, with the exact optical depth of its ConstantMedia.
//
// world_occlusion(ray, t_min, t_max) answers ONE real, tau:
//   +inf   some top-level entry that is not a ConstantMedium has a primitive prim_t accepts in [t_min, t_max] -- the test
//          world_hit applies, with t_max NEVER narrowed;
//   else   the sum, over the ConstantMedium slots of the world list in ascending slot order and starting from +0.0, of
//              ((t2 - t1) * length(direction)) / (-neg_inv_density)
//          with the boundary asked exactly as world_hit asks it (rec1 over (-inf, inf), rec2 from rec1.t + 0.0001),
//          t1 = max(rec1.t, t_min), t2 = min(rec2.t, t_max); a slot whose boundary misses either query or has t1 >= t2
//          adds nothing; t1 < 0 becomes 0.  Density 0 (stored -inf) adds +0; an infinite density (stored -0) adds +inf,
//          which reads like a blocker.
// ConstantMedium::hit (hit.rs:955-986) misses with probability exp(-density * distance_inside_boundary): tau is what its draw
// is a sample of, so exp(-tau) is the probability that world_hit reports no hit at all on independent streams.  No draw is
// made here and only + - * / and sqrt are reached: the answer is deterministic in both precisions.
//
// Why "blocked" equals world_hit's hit flag on a world whose media cannot hit (none, or all of density 0): prim_t's range test
// and both box tests (aabb_may_hit, cull32_may_hit) are monotone in t_max -- what passes under a smaller t_max passes under a
// larger one -- and a closest-hit walk narrows t_max only AFTER it has a hit.  So (=>) a primitive world_hit accepted under
// its narrowed bound is accepted here under the full one, inside boxes that pass a fortiori; (<=) if some primitive is
// accepted here, then either world_hit already had a hit when it came to that primitive's entry, or its bound was still the
// full t_max there, every box on the way passed as it does here, and the primitive is accepted.  Tie rules and visiting order
// decide WHICH hit wins there, never whether there is one -- which is why this walk is free to stop at the first.
//
// The any-hit pieces: bvh_any (no near-first order, no Closest, return at the first accepted primitive), geom_any (the same
// early return for PRIM and GROUP entries), instance_any (the members of an instance tree, culled with a FIXED t_max32).
// Everything else is geometry.hpp's: prim_t, geom_closest for the two boundary queries, xform_ray, the entry decoding of
// world_hit and cull32_may_hit.  Like world_hit the top-level scan is wave-uniform; it ends for the wave once every lane that
// runs it is blocked, and a blocked lane skips geometry but keeps scanning with its wave.
#pragma once
#include "geometry.hpp"

namespace rt {

// Does the ray hit ANY primitive of the BVH in [t_min, t_max]?  Children in storage order; the stack is left as it is on a hit.
template <uint32_t F, class STACK>
RT_HD bool bvh_any(const SceneView& sv, int32_t root, uint32_t first_ref, const Ray& r, real t_min, real t_max, STACK& stack) {
  const Vec3 inv_d = ray_inv_dir(r);
  stack.reset();
  int32_t node = root;
  for (;;) {
    const FlatNode& n = sv.nodes[node];
    int32_t next = -1;
    bool have_next = false;
    for (int c = 0; c < 2; ++c) {
      if (!aabb_may_hit(n.bmin[c], n.bmax[c], r.origin, inv_d, t_min, t_max)) continue;
      const int32_t child = n.child[c];
      if (node_child_is_leaf(child)) {
        const uint32_t f = leaf_first(child), k = leaf_count(child);
        for (uint32_t i = 0; i < k; ++i) {
          real t;
          if (prim_t<F, false>(sv, sv.refs[first_ref + f + i], r, t_min, t_max, &t, nullptr)) return true;
        }
      } else if (have_next) {
        stack.push(child);
      } else {
        next = child; have_next = true;
      }
    }
    if (have_next) { node = next; continue; }
    if (stack.empty()) return false;
    node = stack.pop();
  }
}

// PRIM / GROUP / BVH entries: is any primitive accepted in [t_min, t_max]?  (geom_closest's dispatch.)
template <uint32_t F, class STACK>
RT_HD bool geom_any(const SceneView& sv, const FlatEntry& e, const Ray& r, real t_min, real t_max, STACK& stack) {
  if ((F & F_BVH) && (e.kind == ENTRY_BVH || !(F & (F_PRIM_ENTRY | F_GROUP))))
    return bvh_any<F>(sv, e.a, (uint32_t)e.b, r, t_min, t_max, stack);
  real t;
  if ((F & F_PRIM_ENTRY) && (e.kind == ENTRY_PRIM || !(F & F_GROUP)))
    return prim_t<F, false>(sv, (PrimRef)e.a, r, t_min, t_max, &t, nullptr);
  if (F & F_GROUP) {
    for (int32_t i = 0; i < e.b; ++i)
      if (prim_t<F, false>(sv, sv.refs[e.a + i], r, t_min, t_max, &t, nullptr)) return true;
  }
  return false;
}

// One solid slot (PRIM / GROUP / BVH, or an XFORM chain over one), per-lane loads: instance_offer_slot's decoding.
template <uint32_t F, class STACK>
RT_HD bool slot_any(const SceneView& sv, int32_t slot, const Ray& r, real t_min, real t_max, STACK& stack) {
  const FlatEntry* solid = &sv.entries[sv.top_level[slot]];
  Ray rq = r;
  const FlatEntry* geom = solid;
  if ((F & F_XFORM) && solid->kind == ENTRY_XFORM) {
    geom = &sv.entries[solid->a];
    for (int k = 0; k < solid->b; ++k) rq = xform_ray(solid->ops[k], rq);
  }
  StackAbove<STACK> above = {stack, stack.n};
  return geom_any<F>(sv, *geom, rq, t_min, t_max, above);
}

// The members of one instance tree: instance_walk's box test with t_max32 fixed, return at the first member that is hit.
template <uint32_t F, class STACK>
RT_HD bool instance_any(const SceneView& sv, int32_t root, const Ray& r, real t_min, real t_max, STACK& stack) {
  const Ray32 q = make_ray32(r, t_min);
  const float t_max32 = cull_round_up(t_max);
  stack.reset();
  int32_t cur = root;
  for (;;) {
    if (!node_child_is_leaf(cur)) {
      const FlatNode32& n = sv.nodes32[cur];
      const bool h0 = cull32_may_hit(n.lo[0], n.hi[0], q, t_max32);
      const bool h1 = cull32_may_hit(n.lo[1], n.hi[1], q, t_max32);
      if (h0) { cur = n.child[0]; if (h1) stack.push(n.child[1]); continue; }
      if (h1) { cur = n.child[1]; continue; }
    } else {
      const uint32_t f = leaf_first(cur), k = leaf_count(cur);
      for (uint32_t i = 0; i < k; ++i)
        if (slot_any<F>(sv, (int32_t)(f + i), r, t_min, t_max, stack)) return true;
    }
    if (stack.empty()) return false;
    cur = stack.pop();
  }
}

template <uint32_t F, class STACK>
RT_HD real world_occlusion(const SceneView& sv, const Ray& r, real t_min, real t_max, STACK& stack) {
  bool blocked = false;
  real tau = real(0.0);
  const bool cull_prims = (F & F_PRIM_ENTRY) && sv.top_box32 != nullptr;
  Ray32 q32 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (cull_prims) q32 = make_ray32(r, t_min);
  const float t_max32 = cull_round_up(t_max);
  // instance trees: the next range of member slots a tree covers (wave-uniform, like the scan itself)
  int32_t inst_cur = 0, inst_first = 0x7fffffff;
  if ((F & F_INSTANCE) && sv.inst_entries != 0u) {
    inst_cur = (int32_t)sv.inst_entries;
    inst_first = rt_load_uniform(&sv.entries[inst_cur].b);
  }
  for (int32_t i = 0; i < sv.n_top_level; ++i) {
    if (!RT_WAVE_ANY(!blocked)) break;  // nothing left to learn for this wave
    if ((F & F_INSTANCE) && i == inst_first) {
      const int32_t root = rt_load_uniform(&sv.entries[inst_cur].a), n_slots = rt_load_uniform(&sv.entries[inst_cur].c);
      inst_first = rt_load_uniform(&sv.entries[++inst_cur].b);
      if (!blocked) blocked = instance_any<F>(sv, root, r, t_min, t_max, stack);
      i += n_slots - 1;
      continue;
    }
    // the table walk is wave-uniform: entries are fetched once per wave (rt_load_uniform)
    const FlatEntry e_rec = rt_load_uniform(&sv.entries[rt_load_uniform(&sv.top_level[i])]);
    const FlatEntry* e = &e_rec;
    if (cull_prims && e->kind == ENTRY_PRIM) {
      const float* bx = sv.top_box32 + 6 * i;
      const float lo[3] = {rt_load_uniform(bx + 0), rt_load_uniform(bx + 1), rt_load_uniform(bx + 2)};
      const float hi[3] = {rt_load_uniform(bx + 3), rt_load_uniform(bx + 4), rt_load_uniform(bx + 5)};
      const bool may = !blocked && cull32_may_hit(lo, hi, q32, t_max32);
      if (!RT_WAVE_ANY(may)) continue;
    }
    const bool is_medium = (F & F_MEDIUM) && e->kind == ENTRY_MEDIUM;
    FlatEntry solid_rec = e_rec;
    if (is_medium) solid_rec = rt_load_uniform(&sv.entries[e->a]);
    const FlatEntry* solid = &solid_rec;
    const bool is_xform = (F & F_XFORM) && solid->kind == ENTRY_XFORM;
    FlatEntry geom_rec = solid_rec;
    if (is_xform) geom_rec = rt_load_uniform(&sv.entries[solid->a]);
    if (blocked) continue;  // (after the uniform loads: a blocked lane only skips the geometry)
    Ray rq = r;
    if (is_xform) {
      for (int k = 0; k < solid->b; ++k) rq = xform_ray(solid->ops[k], rq);
    }
    if (!is_medium) {
      blocked = geom_any<F>(sv, geom_rec, rq, t_min, t_max, stack);
      continue;
    }
    // the medium's boundary, asked as ConstantMedium::hit asks it (hit.rs:961-967; world_hit)
    Closest best;
    geom_closest<F, false>(sv, geom_rec, rq, -RT_INFINITY, RT_INFINITY, &best, stack, nullptr);
    if (!best.hit) continue;
    const real rec1_t = best.t;
    geom_closest<F, false>(sv, geom_rec, rq, medium_second_t_min(rec1_t), RT_INFINITY, &best, stack, nullptr);
    if (!best.hit) continue;
    real t1 = rt_fmax(rec1_t, t_min);
    const real t2 = rt_fmin(best.t, t_max);
    if (t1 >= t2) continue;
    if (t1 < real(0.0)) t1 = real(0.0);
    const real distance_inside_boundary = (t2 - t1) * length(r.direction);
    tau = tau + distance_inside_boundary / (-e->f[0]);
  }
  return blocked ? RT_INFINITY : tau;
}

}  // namespace rt
