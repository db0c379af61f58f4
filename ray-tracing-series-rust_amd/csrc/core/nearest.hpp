// Nearest-point queries: the closest surface point of the world list to a point p at a time (include/rtx_abi.h, "nearest-point
// queries", states the definition; DESIGN.md 7.7 the derivations).
//
//   prim_nearest     the point q of ONE primitive closest to p, by kind.  The order of operations below IS the definition: the
//                    device kernel (hip/nearest.inc), the culled host walk and the exhaustive host scan
//                    (tests/nearest_host_check.cpp) all call this one text, in either precision.
//   nearest_offer    the key d2 = dot(p - q, p - q) in the primitive's own frame and the replacement rule: smaller d2 wins, an
//                    equal d2 goes to the lexicographically smaller (slot, order).  Nothing else decides the answer.
//   box_d2_lower     a lower bound of d2 over everything inside an f32 box, with an explicit slack.
//   bvh_nearest      the ordered walk of one BVH's culling tree (nodes32) against the shrinking bound.
//   instance_nearest the same walk over an instance tree's member boxes.
//   world_nearest    the wave-uniform scan of the world list.
// Boxes only decide which primitives are asked: a subtree is dropped when its bound is STRICTLY above the best d2 so far, so
// every candidate that could win or tie is met, and the answer is that of a plain loop over all slots and refs.
#pragma once
#include "geometry.hpp"

namespace rt {

// ---- the slack of box_d2_lower --------------------------------------------------------------------------------------------------
// u = 2^-53 (f64) or 2^-24 (f32) is the unit roundoff of `real`, M_a = max(|lo_a|, |hi_a|) the largest plane magnitude of the
// box on axis a.  Every primitive's stored box contains the primitive's exact coordinates on that axis, so |c_a|, |r| and every
// vertex coordinate are at most M_a (an inner node's box contains its primitives' boxes: its M_a is no smaller).
//   * The computed q can leave its box.  A sphere's q_a = c_a + v_a * (|r| / len): v = p - c, the dot product, sqrt, the quotient,
//     the product and the sum round once each; the exact value lies in [c_a - |r|, c_a + |r|], the computed one within
//     about 6 u (|c_a| + |r|) <= 12 u M_a of it, and the box's own planes are the ROUNDED c_a -+ |r| (1 u M_a more; an outward f32
//     narrowing adds nothing when the plane is exact in f32, e.g. an integer).  A moving sphere's centre is a rounded lerp of
//     two rounded end centres inside the union of the end boxes: 4 u M_a more.  A rectangle's q is a clamp (exact) and a
//     triangle's q is clamped into its vertices' box by prim_nearest itself: both stay inside.  An f32 scene's primitives are the
//     f64 ones narrowed (1 u each for c and r) while its boxes come from the f64 values: 2 u M_a more.  Total: below 20 u M_a.
//   * The bound's own arithmetic.  The gap lo_a - p_a (or p_a - hi_a) rounds once: u (|p_a| + M_a).
//   * The key's arithmetic.  p_a - q_a rounds once, relative u: covered by the final factor below.
// So the per-axis gap is shrunk by EPS (|p_a| + M_a) with EPS = 32 u: 2^-48 in f64, 2^-19 in f32 (the f32 figure also swallows
// the narrowing of p itself, which both the bound and the key see alike).  Squares and the three-term sum round with a relative
// error below 4 u, the key's dot product likewise from below: the sum is scaled by DOWN = 1 - 16 u, 1 - 2^-49 and 1 - 2^-20.
// The members of an instance tree stand in WORLD space while the key is taken in the member's frame: their boxes are already
// padded by 2^-22 of the largest magnitude met on the way (core/member_box.hpp), 2^26 times the f64 error of the stored
// sin / cos and of the ops; under an f32 scene the padding is 4 u32 of that magnitude, and the ops' rounding (3 u32 per op, four
// ops at most) is covered by EPS on top of it.
#if defined(RT_F32)
#define RT_NEAREST_EPS real(0x1.0p-19)
#define RT_NEAREST_DOWN (real(1.0) - real(0x1.0p-20))
#else
#define RT_NEAREST_EPS real(0x1.0p-48)
#define RT_NEAREST_DOWN (real(1.0) - real(0x1.0p-49))
#endif

// Work of a query, for the host checker (COUNT = true).
struct NearestCounters {
  unsigned long long box_tests;   // box_d2_lower evaluations
  unsigned long long prim_tests;  // prim_nearest evaluations
};

// A query's running answer.  q is in the frame of the entry being walked until entry_nearest maps it out (changed says that it
// has to); mat_override >= 0: the phase material of the ConstantMedium the winner bounds.
struct NearestBest {
  real d2;
  Vec3 q;
  PrimRef ref;
  int32_t slot;
  uint32_t order;
  int32_t mat_override;
  bool found, changed;
};

RT_HD void nearest_begin(NearestBest* b, real r_max) {
  b->d2 = r_max * r_max;
  b->q = v3(real(0.0), real(0.0), real(0.0));
  b->ref = 0; b->slot = -1; b->order = 0; b->mat_override = -1;
  b->found = false; b->changed = false;
}

// The point of triangle (a, b, c) closest to p: the barycentric-region algorithm (C. Ericson, Real-Time Collision Detection,
// 5.1.5), regions tested in the order vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, face.  Last, q is clamped into the
// box of the three vertices per axis: a no-op for every well-conditioned triangle, and for a sliver whose region tests cancel it
// keeps q inside the box that culls the triangle.
RT_HD Vec3 triangle_nearest(Vec3 a, Vec3 b, Vec3 c, Vec3 p) {
  const Vec3 ab = b - a, ac = c - a, ap = p - a;
  const real d1 = dot(ab, ap), d2 = dot(ac, ap);
  Vec3 q;
  bool done = false;
  if (d1 <= real(0.0) && d2 <= real(0.0)) { q = a; done = true; }
  const Vec3 bp = p - b;
  const real d3 = dot(ab, bp), d4 = dot(ac, bp);
  if (!done && d3 >= real(0.0) && d4 <= d3) { q = b; done = true; }
  const real vc = d1 * d4 - d3 * d2;
  if (!done && vc <= real(0.0) && d1 >= real(0.0) && d3 <= real(0.0)) {
    const real v = d1 / (d1 - d3);
    q = a + ab * v; done = true;
  }
  const Vec3 cp = p - c;
  const real d5 = dot(ab, cp), d6 = dot(ac, cp);
  if (!done && d6 >= real(0.0) && d5 <= d6) { q = c; done = true; }
  const real vb = d5 * d2 - d1 * d6;
  if (!done && vb <= real(0.0) && d2 >= real(0.0) && d6 <= real(0.0)) {
    const real w = d2 / (d2 - d6);
    q = a + ac * w; done = true;
  }
  const real va = d3 * d6 - d5 * d4;
  if (!done && va <= real(0.0) && (d4 - d3) >= real(0.0) && (d5 - d6) >= real(0.0)) {
    const real w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    q = b + (c - b) * w; done = true;
  }
  if (!done) {
    const real denom = real(1.0) / (va + vb + vc);
    const real v = vb * denom, w = vc * denom;
    q = (a + ab * v) + ac * w;
  }
  q.x = rt_fmin(rt_fmax(q.x, rt_fmin(rt_fmin(a.x, b.x), c.x)), rt_fmax(rt_fmax(a.x, b.x), c.x));
  q.y = rt_fmin(rt_fmax(q.y, rt_fmin(rt_fmin(a.y, b.y), c.y)), rt_fmax(rt_fmax(a.y, b.y), c.y));
  q.z = rt_fmin(rt_fmax(q.z, rt_fmin(rt_fmin(a.z, b.z), c.z)), rt_fmax(rt_fmax(a.z, b.z), c.z));
  return q;
}

// The point of a sphere of centre c closest to p: c + (p - c) * (|radius| / |p - c|); at the centre itself, c + (|radius|, 0, 0).
RT_HD Vec3 sphere_nearest(Vec3 c, real radius, Vec3 p) {
  const Vec3 v = p - c;
  const real len = rt_sqrt(dot(v, v));
  const real ar = rt_fabs(radius);
  if (len == real(0.0)) return c + v3(ar, real(0.0), real(0.0));
  return c + v * (ar / len);
}

// q = the point of primitive `ref` closest to p at `time`; false: the primitive is not a candidate (an inverted rectangle, a
// zero-area triangle, a GravitySphere).
template <uint32_t F>
RT_HD bool prim_nearest(const SceneView& sv, PrimRef ref, Vec3 p, real time, Vec3* q) {
  const uint32_t idx = primref_index(ref);
  const uint32_t type = primref_type(ref);
  if ((F & F_SPHERE) && type == PRIM_SPHERE) {
    const FlatSphere& s = sv.spheres[idx];
    *q = sphere_nearest(v3(s.cx, s.cy, s.cz), s.radius, p);
    return true;
  }
  if ((F & F_MOVING_SPHERE) && type == PRIM_MOVING_SPHERE) {
    const FlatMovingSphere& s = sv.moving_spheres[idx];
    *q = sphere_nearest(moving_sphere_center(s, time), s.radius, p);
    return true;
  }
  if ((F & F_RECT) && type == PRIM_RECT) {
    const FlatRect& r = sv.rects[idx];
    if (r.a0 > r.a1 || r.b0 > r.b1) return false;
    if (r.axis == RECT_XY) *q = v3(rt_fmin(rt_fmax(p.x, r.a0), r.a1), rt_fmin(rt_fmax(p.y, r.b0), r.b1), r.k);
    else if (r.axis == RECT_XZ) *q = v3(rt_fmin(rt_fmax(p.x, r.a0), r.a1), r.k, rt_fmin(rt_fmax(p.z, r.b0), r.b1));
    else *q = v3(r.k, rt_fmin(rt_fmax(p.y, r.a0), r.a1), rt_fmin(rt_fmax(p.z, r.b0), r.b1));
    return true;
  }
  if ((F & F_TRIANGLE) && type == PRIM_TRIANGLE) {
    const FlatTriangle& t = sv.triangles[idx];
    if (t.normal[0] != t.normal[0] || t.normal[1] != t.normal[1] || t.normal[2] != t.normal[2]) return false;
    *q = triangle_nearest(load_v3(t.v0), load_v3(t.v1), load_v3(t.v2), p);
    return true;
  }
  return false;
}

// One primitive offered to the running answer (p in the primitive's frame).
template <uint32_t F, bool COUNT>
RT_HD void nearest_offer(const SceneView& sv, PrimRef ref, int32_t slot, uint32_t order, Vec3 p, real time, NearestBest* best,
                         NearestCounters* cnt) {
  if (COUNT) cnt->prim_tests++;
  Vec3 q;
  if (!prim_nearest<F>(sv, ref, p, time, &q)) return;
  const Vec3 v = p - q;
  const real d2 = dot(v, v);
  const bool first = !best->found || slot < best->slot || (slot == best->slot && order < best->order);
  if (!(d2 < best->d2 || (d2 == best->d2 && first))) return;  // (a NaN d2 fails both)
  best->d2 = d2; best->q = q; best->ref = ref; best->slot = slot; best->order = order;
  best->found = true; best->changed = true;
}

// A lower bound of the key over every primitive whose box lies inside [lo, hi] (f32 planes, any order): see the slack above.  An
// axis with a NaN or infinite plane gives no bound; a NaN p gives 0.
RT_HD real box_d2_lower(const float* lo, const float* hi, Vec3 p) {
  const real pc[3] = {p.x, p.y, p.z};
  real s = real(0.0);
  for (int a = 0; a < 3; ++a) {
    const float l32 = __builtin_fminf(lo[a], hi[a]), h32 = __builtin_fmaxf(lo[a], hi[a]);
    if (!(__builtin_fabsf(lo[a]) < __builtin_huge_valf()) || !(__builtin_fabsf(hi[a]) < __builtin_huge_valf())) continue;
    const real l = (real)l32, h = (real)h32;
    real g = rt_fmax(rt_fmax(l - pc[a], pc[a] - h), real(0.0));
    const real m = rt_fabs(pc[a]) + rt_fmax(rt_fabs(l), rt_fabs(h));
    g = rt_fmax(g - RT_NEAREST_EPS * m, real(0.0));
    s = s + g * g;
  }
  return s * RT_NEAREST_DOWN;
}

// The ordered walk of one BVH.  At a node both children's bounds are taken against the CURRENT best d2; leaf children are
// tested at once, the nearer first, and the second is judged again after the first may have shrunk the bound; then the walk
// descends into the nearer inner child that is still within the bound and pushes the other.  A popped node carries no bound:
// it is re-judged by its own children's tests.  cull = false (the mover rule): every bound is 0, the walk visits every ref.
// Stack: a step pushes at most one node and then descends one level, exactly as bvh_step does, so the stack never holds more
// than the depth of the tree -- the ray walk's max_stack; under an instance tree the member's walk runs above the slot walk's
// entries (StackAbove), and max_stack is the sum the flattener already counts for world_hit.
template <uint32_t F, bool COUNT, class STACK>
RT_HD void bvh_nearest(const SceneView& sv, int32_t root, uint32_t first_ref, int32_t slot, bool cull, Vec3 p, real time,
                       NearestBest* best, STACK& stack, NearestCounters* cnt) {
  stack.reset();
  int32_t node = root;
  for (;;) {
    const FlatNode32& n = sv.nodes32[node];
    if (COUNT) cnt->box_tests += 2;
    real b[2] = {real(0.0), real(0.0)};
    if (cull) { b[0] = box_d2_lower(n.lo[0], n.hi[0], p); b[1] = box_d2_lower(n.lo[1], n.hi[1], p); }
    const int first = b[1] < b[0] ? 1 : 0;
    for (int k = 0; k < 2; ++k) {
      const int c = k == 0 ? first : 1 - first;
      const int32_t child = n.child[c];
      if (!node_child_is_leaf(child) || b[c] > best->d2) continue;
      const uint32_t f = leaf_first(child), cnt_l = leaf_count(child);
      for (uint32_t i = 0; i < cnt_l; ++i)
        nearest_offer<F, COUNT>(sv, sv.refs[first_ref + f + i], slot, f + i, p, time, best, cnt);
    }
    const int32_t cn = n.child[first], cf = n.child[1 - first];
    const bool go_n = !node_child_is_leaf(cn) && !(b[first] > best->d2);
    const bool go_f = !node_child_is_leaf(cf) && !(b[1 - first] > best->d2);
    if (go_n) { node = cn; if (go_f) stack.push(cf); continue; }
    if (go_f) { node = cf; continue; }
    if (stack.empty()) return;
    node = stack.pop();
  }
}

// p as the child of one transform op sees it (xform_ray's origin arithmetic), and a point of the child mapped back out
// (xform_record's p arithmetic).
RT_HD Vec3 xform_point_in(const FlatXformOp& op, Vec3 p) {
  if (op.op == XFORM_TRANSLATE) return p - load_v3(op.v);
  const real sin_t = op.v[0], cos_t = op.v[1];
  return v3(cos_t * p.x - sin_t * p.z, p.y, sin_t * p.x + cos_t * p.z);
}
RT_HD Vec3 xform_point_out(const FlatXformOp& op, Vec3 q) {
  if (op.op == XFORM_TRANSLATE) return q + load_v3(op.v);
  const real sin_t = op.v[0], cos_t = op.v[1];
  return v3(cos_t * q.x + sin_t * q.z, q.y, -sin_t * q.x + cos_t * q.z);
}

// One solid entry of slot `slot` offered to the running answer: `solid` is the slot's entry (or a medium's boundary), `geom` the
// PRIM / GROUP / BVH entry below its XFORM chain (solid itself without one).  p goes in through the ops outermost first; a new
// winner's q comes back out innermost first.  medium_mat >= 0: the entry bounds a ConstantMedium with that phase material.
template <uint32_t F, bool COUNT, class STACK>
RT_HD void entry_nearest(const SceneView& sv, int32_t slot, const FlatEntry& solid, const FlatEntry& geom, bool is_xform,
                         int32_t medium_mat, Vec3 p, real time, NearestBest* best, STACK& stack, NearestCounters* cnt) {
  Vec3 pl = p;
  if (is_xform) {
    for (int k = 0; k < solid.b; ++k) pl = xform_point_in(solid.ops[k], pl);
  }
  best->changed = false;
  if ((F & F_BVH) && geom.kind == ENTRY_BVH) {
    // the mover rule: the boxes hold the BVH's MovingSpheres only inside its own time interval
    bool cull = true;
    if ((F & F_MOVING_SPHERE) && (sv.features & F_MOVING_SPHERE))
      cull = time >= rt_fmin(geom.f[0], geom.f[1]) && time <= rt_fmax(geom.f[0], geom.f[1]);
    bvh_nearest<F, COUNT>(sv, geom.a, (uint32_t)geom.b, slot, cull, pl, time, best, stack, cnt);
  } else if ((F & F_PRIM_ENTRY) && geom.kind == ENTRY_PRIM) {
    nearest_offer<F, COUNT>(sv, (PrimRef)geom.a, slot, 0u, pl, time, best, cnt);
  } else if ((F & F_GROUP) && geom.kind == ENTRY_GROUP) {
    for (int32_t i = 0; i < geom.b; ++i) nearest_offer<F, COUNT>(sv, sv.refs[geom.a + i], slot, (uint32_t)i, pl, time, best, cnt);
  }
  if (!best->changed) return;
  if (is_xform) {
    for (int k = solid.b - 1; k >= 0; --k) best->q = xform_point_out(solid.ops[k], best->q);
  }
  best->mat_override = medium_mat;
}

// One member slot of an instance tree (never a medium), per-lane loads: instance_offer_slot's decoding.
template <uint32_t F, bool COUNT, class STACK>
RT_HD void slot_nearest(const SceneView& sv, int32_t slot, Vec3 p, real time, NearestBest* best, STACK& stack, NearestCounters* cnt) {
  const FlatEntry* solid = &sv.entries[sv.top_level[slot]];
  const bool is_xform = (F & F_XFORM) && solid->kind == ENTRY_XFORM;
  const FlatEntry* geom = is_xform ? &sv.entries[solid->a] : solid;
  StackAbove<STACK> above = {stack, stack.n};
  entry_nearest<F, COUNT>(sv, slot, *solid, *geom, is_xform, -1, p, time, best, above, cnt);
}

// The members of one instance tree: bvh_nearest's ordered walk over the members' world boxes (a leaf holds member slots).
template <uint32_t F, bool COUNT, class STACK>
RT_HD void instance_nearest(const SceneView& sv, int32_t root, Vec3 p, real time, NearestBest* best, STACK& stack,
                            NearestCounters* cnt) {
  stack.reset();
  int32_t cur = root;
  for (;;) {
    if (!node_child_is_leaf(cur)) {
      const FlatNode32& n = sv.nodes32[cur];
      if (COUNT) cnt->box_tests += 2;
      const real b0 = box_d2_lower(n.lo[0], n.hi[0], p), b1 = box_d2_lower(n.lo[1], n.hi[1], p);
      const int first = b1 < b0 ? 1 : 0;
      const bool go_n = !((first ? b1 : b0) > best->d2), go_f = !((first ? b0 : b1) > best->d2);
      const int32_t cn = n.child[first], cf = n.child[1 - first];
      if (go_n) { cur = cn; if (go_f) stack.push(cf); continue; }
      if (go_f) { cur = cf; continue; }
    } else {
      const uint32_t f = leaf_first(cur), k = leaf_count(cur);
      for (uint32_t i = 0; i < k; ++i) slot_nearest<F, COUNT>(sv, (int32_t)(f + i), p, time, best, stack, cnt);
    }
    if (stack.empty()) return;
    cur = stack.pop();
  }
}

// The world list.  The scan is wave-uniform like world_occlusion's: entries are fetched once per wave, and a plain slot whose
// box no lane can improve on is skipped.  media: ConstantMedium slots offer their boundary (reported with the phase material)
// or are skipped.  A NaN r_max (best->d2 is NaN) finds nothing and walks nothing.
template <uint32_t F, bool COUNT, class STACK>
RT_HD void world_nearest(const SceneView& sv, Vec3 p, real time, real r_max, bool media, NearestBest* best, STACK& stack,
                         NearestCounters* cnt) {
  nearest_begin(best, r_max);
  const bool dead = !(best->d2 == best->d2);
  const bool cull_prims = (F & F_PRIM_ENTRY) && sv.top_box32 != nullptr;
  int32_t inst_cur = 0, inst_first = 0x7fffffff;
  if ((F & F_INSTANCE) && sv.inst_entries != 0u) {
    inst_cur = (int32_t)sv.inst_entries;
    inst_first = rt_load_uniform(&sv.entries[inst_cur].b);
  }
  for (int32_t i = 0; i < sv.n_top_level; ++i) {
    if (!RT_WAVE_ANY(!dead)) break;
    if ((F & F_INSTANCE) && i == inst_first) {
      const int32_t root = rt_load_uniform(&sv.entries[inst_cur].a), n_slots = rt_load_uniform(&sv.entries[inst_cur].c);
      inst_first = rt_load_uniform(&sv.entries[++inst_cur].b);
      if (!dead) instance_nearest<F, COUNT>(sv, root, p, time, best, stack, cnt);
      i += n_slots - 1;
      continue;
    }
    const FlatEntry e_rec = rt_load_uniform(&sv.entries[rt_load_uniform(&sv.top_level[i])]);
    if (cull_prims && e_rec.kind == ENTRY_PRIM) {
      const float* bx = sv.top_box32 + 6 * i;
      const float lo[3] = {rt_load_uniform(bx + 0), rt_load_uniform(bx + 1), rt_load_uniform(bx + 2)};
      const float hi[3] = {rt_load_uniform(bx + 3), rt_load_uniform(bx + 4), rt_load_uniform(bx + 5)};
      if (COUNT) cnt->box_tests++;
      const bool may = !dead && !(box_d2_lower(lo, hi, p) > best->d2);
      if (!RT_WAVE_ANY(may)) continue;
    }
    const bool is_medium = (F & F_MEDIUM) && e_rec.kind == ENTRY_MEDIUM;
    if (is_medium && !media) continue;
    FlatEntry solid_rec = e_rec;
    if (is_medium) solid_rec = rt_load_uniform(&sv.entries[e_rec.a]);
    const bool is_xform = (F & F_XFORM) && solid_rec.kind == ENTRY_XFORM;
    FlatEntry geom_rec = solid_rec;
    if (is_xform) geom_rec = rt_load_uniform(&sv.entries[solid_rec.a]);
    if (dead) continue;  // (after the uniform loads)
    entry_nearest<F, COUNT>(sv, i, solid_rec, geom_rec, is_xform, is_medium ? e_rec.b : -1, p, time, best, stack, cnt);
  }
}

// The material of a found answer: the winner's own, or the phase material of the medium it bounds.
RT_HD int32_t nearest_material(const SceneView& sv, const NearestBest& best) {
  if (best.mat_override >= 0) return best.mat_override;
  const uint32_t idx = primref_index(best.ref);
  switch (primref_type(best.ref)) {
    case PRIM_SPHERE: return sv.spheres[idx].mat;
    case PRIM_MOVING_SPHERE: return sv.moving_spheres[idx].mat;
    case PRIM_RECT: return sv.rects[idx].mat;
    default: return sv.triangles[idx].mat;
  }
}

}  // namespace rt
