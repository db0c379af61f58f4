// The reference bounding box of one STATIC flattened primitive (hit.rs bounding_box impls): a sphere (with |radius|: see
// host/flatten.cpp, prim_box), a rectangle (+-0.0001 on the thin axis) or a triangle.  ONE text for the flattener
// (host/flatten.cpp), the host refits of rtx_flat_set_triangles / _set_spheres (host/set_triangles.hpp)
// and the device refits of rtx_scene_set_triangles / _set_spheres (hip/mesh_update.inc): a refitted BVH
// is judged bit for bit against one flattened from scratch, so all of them must round alike.  Sums and differences of two
// doubles, min and max: exact or correctly rounded in either build.  The f32 boxes of top-level slots follow the same rule:
// plain_slot_box32 and medium_sphere_box32 below are what the flattener, the upload and the updates all call.
#pragma once
#include "flat_types.hpp"
#include "member_box.hpp"  // f32_narrow_down / _up, f32_step_down / _up

namespace rt {

// b = lo xyz, hi xyz.  Moving and gravity spheres have no static box: the caller keeps them away, and b is the empty box.
RT_HD void static_prim_box(PrimRef ref, const FlatSphere* spheres, const FlatRect* rects, const FlatTriangle* triangles, double* b) {
  const uint32_t idx = primref_index(ref);
  switch (primref_type(ref)) {
    case PRIM_SPHERE: {  // hit.rs:239-244
      const FlatSphere& s = spheres[idx];
      const double ar = rt_fabs((double)s.radius);
      b[0] = (double)s.cx - ar; b[1] = (double)s.cy - ar; b[2] = (double)s.cz - ar;
      b[3] = (double)s.cx + ar; b[4] = (double)s.cy + ar; b[5] = (double)s.cz + ar;
      break;
    }
    case PRIM_RECT: {  // hit.rs:503-508, 568-573, 633-638 (+-0.0001 on the thin axis)
      const FlatRect& q = rects[idx];
      const double a0 = q.a0, a1 = q.a1, b0 = q.b0, b1 = q.b1, k = q.k;
      if (q.axis == RECT_XY) { b[0] = a0; b[1] = b0; b[2] = k - 0.0001; b[3] = a1; b[4] = b1; b[5] = k + 0.0001; }
      else if (q.axis == RECT_XZ) { b[0] = a0; b[1] = k - 0.0001; b[2] = b0; b[3] = a1; b[4] = k + 0.0001; b[5] = b1; }
      else { b[0] = k - 0.0001; b[1] = a0; b[2] = b0; b[3] = k + 0.0001; b[4] = a1; b[5] = b1; }
      break;
    }
    case PRIM_TRIANGLE: {  // hit.rs:164-177
      const FlatTriangle& t = triangles[idx];
      for (int a = 0; a < 3; ++a) {
        b[a] = rt_fmin(rt_fmin((double)t.v0[a], (double)t.v1[a]), (double)t.v2[a]);
        b[3 + a] = rt_fmax(rt_fmax((double)t.v0[a], (double)t.v1[a]), (double)t.v2[a]);
      }
      break;
    }
    default:  // a timed sphere: the EMPTY box, which a union ignores (callers refuse such a BVH before they get here)
      for (int a = 0; a < 3; ++a) { b[a] = __builtin_huge_val(); b[3 + a] = -__builtin_huge_val(); }
      break;
  }
}

// *box (lo xyz, hi xyz) grown by the ORDERED box of one primitive: each axis is ordered before the union, as the flattener
// orders a member's boxes (a plane pair that came out inverted must not empty the union).
RT_HD void grow_ordered(double* box, const double* pb) {
  for (int a = 0; a < 3; ++a) {
    box[a] = rt_fmin(box[a], rt_fmin(pb[a], pb[3 + a]));
    box[3 + a] = rt_fmax(box[3 + a], rt_fmax(pb[a], pb[3 + a]));
  }
}

// The f32 box of a plain top-level slot (FlatScene::top_box32, WorldDesc::box) from the reference box b of its static
// primitive: each axis ordered first (a sphere of negative radius has an inverted reference box, and "outward" must mean
// outward), then narrowed outward; an axis with a NaN plane is left unbounded.  THE rule of the flattener ("boxes of the plain
// static primitives") and of every update that moves such a primitive.
RT_HD void plain_slot_box32(PrimRef ref, const FlatSphere* spheres, const FlatRect* rects, const FlatTriangle* triangles, float* bx) {
  double b[6];
  static_prim_box(ref, spheres, rects, triangles, b);
  for (int a = 0; a < 3; ++a) {
    const double blo = rt_fmin(b[a], b[3 + a]), bhi = rt_fmax(b[a], b[3 + a]);
    if (b[a] == b[a] && b[3 + a] == b[3 + a]) { bx[a] = f32_narrow_down(blo); bx[3 + a] = f32_narrow_up(bhi); }
    else { bx[a] = -__builtin_huge_valf(); bx[3 + a] = __builtin_huge_valf(); }
  }
}

// The f32 box of a ConstantMedium whose boundary is one static sphere, untransformed (WorldDesc::box of such a slot): the
// rounded sums centre -+ |radius| narrowed outward, then ONE MORE step outward, because the sum itself rounded once already.
// false: a plane is not finite, and the slot goes without a box.
RT_HD bool medium_sphere_box32(const FlatSphere& sp, float* bx) {
  const double c[3] = {(double)sp.cx, (double)sp.cy, (double)sp.cz}, r = rt_fabs((double)sp.radius);
  bool finite = true;
  for (int a = 0; a < 3; ++a) {
    float lo = f32_narrow_down(c[a] - r), hi = f32_narrow_up(c[a] + r);
    if (rt_fabs(lo) < __builtin_huge_valf()) lo = f32_step_down(lo);  // (an infinite plane stays where it is)
    if (rt_fabs(hi) < __builtin_huge_valf()) hi = f32_step_up(hi);
    bx[a] = lo; bx[3 + a] = hi;
    finite = finite && rt_fabs(lo) < __builtin_huge_valf() && rt_fabs(hi) < __builtin_huge_valf();
  }
  return finite;
}

// cx cy cz radius -> the record (mat and pad stay), with the casts SceneGraph::sphere and the flattener make.
RT_HD void set_sphere_values(FlatSphere* s, const double* v) {
  s->cx = (real)v[0]; s->cy = (real)v[1]; s->cz = (real)v[2]; s->radius = (real)v[3];
}

// a0 a1 b0 b1 k -> the record (axis and mat stay): the constructor's (x0, x1, y0, y1, k), FlatRect's own order, with the casts
// the flattener makes.  No rule beyond that: an inverted or empty extent is what the constructor would have stored.
RT_HD void set_rect_values(FlatRect* q, const double* v) {
  q->a0 = (real)v[0]; q->a1 = (real)v[1]; q->b0 = (real)v[2]; q->b1 = (real)v[3]; q->k = (real)v[4];
}

// v0 v1 v2 -> the record's vertices and normal = unit((v1 - v0) x (v2 - v0)) (hit.rs:96-107), by the functions
// SceneGraph::triangle calls; mat and pad stay.  A zero-area triangle gets the NaN normal a fresh build gives it.
RT_HD void set_triangle_vertices(FlatTriangle* t, const double* v) {
  const Vec3 a0 = v3((real)v[0], (real)v[1], (real)v[2]), a1 = v3((real)v[3], (real)v[4], (real)v[5]), a2 = v3((real)v[6], (real)v[7], (real)v[8]);
  const Vec3 n = unit(cross(a1 - a0, a2 - a0));
  for (int i = 0; i < 3; ++i) { t->v0[i] = (real)v[i]; t->v1[i] = (real)v[3 + i]; t->v2[i] = (real)v[6 + i]; }
  t->normal[0] = n.x; t->normal[1] = n.y; t->normal[2] = n.z;
}

}  // namespace rt
