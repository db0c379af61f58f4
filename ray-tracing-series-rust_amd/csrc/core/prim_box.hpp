// The reference bounding box of one STATIC flattened primitive (hit.rs bounding_box impls): a sphere (with |radius|: see
// host/flatten.cpp, prim_box), a rectangle (+-0.0001 on the thin axis) or a triangle.  ONE text for the flattener
// (host/flatten.cpp), the host refit of rtx_flat_set_triangles (host/set_triangles.hpp) and the device refit of
// rtx_scene_set_triangles (hip/mesh_update.inc): a refitted BVH is judged bit for bit against one flattened from scratch, so
// all three must round alike.  Sums and differences of two doubles, min and max: exact or correctly rounded in either build.
#pragma once
#include "flat_types.hpp"

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

// v0 v1 v2 -> the record's vertices and normal = unit((v1 - v0) x (v2 - v0)) (hit.rs:96-107), by the functions
// SceneGraph::triangle calls; mat and pad stay.  A zero-area triangle gets the NaN normal a fresh build gives it.
RT_HD void set_triangle_vertices(FlatTriangle* t, const double* v) {
  const Vec3 a0 = v3((real)v[0], (real)v[1], (real)v[2]), a1 = v3((real)v[3], (real)v[4], (real)v[5]), a2 = v3((real)v[6], (real)v[7], (real)v[8]);
  const Vec3 n = unit(cross(a1 - a0, a2 - a0));
  for (int i = 0; i < 3; ++i) { t->v0[i] = (real)v[i]; t->v1[i] = (real)v[3 + i]; t->v2[i] = (real)v[6 + i]; }
  t->normal[0] = n.x; t->normal[1] = n.y; t->normal[2] = n.z;
}

}  // namespace rt
