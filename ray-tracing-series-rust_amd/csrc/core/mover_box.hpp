// What is derived from the values of a MovingSphere (c0, c1, radius; time0, time1 given), ONE text for the host twin of
// rtx_*_set_moving_spheres (host/set_triangles.hpp), the device refit (hip/mesh_update.inc: k_refit_timed_bvh, k_slot_boxes)
// and the upload (hip/trace_world.inc: build_world_desc):
//   moving_sphere_box     the reference box of a mover over [ta, tb]            (host/flatten.cpp: prim_box, hit.rs:317-327)
//   motion_child_planes   a child's two f64 end boxes -> lo0, dlo, hi0, dhi     (host/flatten.cpp: build_motion_boxes)
//   mover_slot_box32      the f32 box of a plain mover in the world list        (WD_TIME_BOX of build_world_desc)
// host/flatten.cpp keeps its own text of the first two (prim_box, motion_box_at, build_motion_boxes): a flat scene built from
// scratch, top-down, is the judge the bottom-up refits are held to.  Sums, differences and products of two doubles, min, max and
// casts: correctly rounded in either build, and the project compiles without contraction (-ffp-contract=off).
#pragma once
#include "geometry.hpp"  // moving_sphere_center
#include "prim_box.hpp"

namespace rt {

// c0 xyz, c1 xyz, radius -> the record (time0, time1, mat and pad stay), with the casts SceneGraph::moving_sphere and the
// flattener make.
RT_HD void set_moving_sphere_values(FlatMovingSphere* s, const double* v) {
  for (int i = 0; i < 3; ++i) { s->c0[i] = (real)v[i]; s->c1[i] = (real)v[3 + i]; }
  s->radius = (real)v[6];
}

// b = lo xyz, hi xyz: the min / max of the mover's boxes at ta and at tb, each centre -+ |radius| (see host/flatten.cpp, prim_box,
// for |radius|).  ta == tb gives two equal boxes and so the box at that one instant.  A mover with time0 == time1 has no finite
// centre; min and max ignore a NaN operand, as the flattener's do.
RT_HD void moving_sphere_box(const FlatMovingSphere& s, double ta, double tb, double* b) {
  const double ar = rt_fabs((double)s.radius);
  const Vec3 r = v3((real)ar, (real)ar, (real)ar);
  const Vec3 ca = moving_sphere_center(s, (real)ta), cb = moving_sphere_center(s, (real)tb);
  const Vec3 lo0 = ca - r, hi0 = ca + r, lo1 = cb - r, hi1 = cb + r;
  b[0] = rt_fmin((double)lo0.x, (double)lo1.x); b[1] = rt_fmin((double)lo0.y, (double)lo1.y); b[2] = rt_fmin((double)lo0.z, (double)lo1.z);
  b[3] = rt_fmax((double)hi0.x, (double)hi1.x); b[4] = rt_fmax((double)hi0.y, (double)hi1.y); b[5] = rt_fmax((double)hi0.z, (double)hi1.z);
}

// The time-aware planes of ONE child (FlatMotion32::lo0[c], dlo[c], hi0[c], dhi[c]; 3 floats each) from the unions b0 AT the
// BVH's time0 and b1 AT its time1 (lo xyz, hi xyz): per axis both end boxes are pushed outward by 2^-21 of the axis' largest
// magnitude (+ 1e-30 for an axis at 0), narrowed outward to f32, and the slope is ONE f32 subtraction of the narrowed ends.
// mag * 0x1.0p-21 is exact (a power of two, no underflow that matters next to 1e-30), so a contracted fma of the margin could
// not differ from the product and the sum; the project compiles without contraction all the same.
// Returns the axes on which a slope it wrote is not zero: bit 0 x, bit 1 y, bit 2 z (LdsPlan::motion_axis is planned from the OR).
RT_HD uint32_t motion_child_planes(const double* b0, const double* b1, float* lo0, float* dlo, float* hi0, float* dhi) {
  uint32_t moves = 0u;
  for (int a = 0; a < 3; ++a) {
    const double mag = rt_fmax(rt_fmax(rt_fabs(b0[a]), rt_fabs(b0[3 + a])), rt_fmax(rt_fabs(b1[a]), rt_fabs(b1[3 + a])));
    const double margin = mag * 0x1.0p-21 + 1e-30;
    const float lo_a = f32_narrow_down(b0[a] - margin), lo_b = f32_narrow_down(b1[a] - margin);
    const float hi_a = f32_narrow_up(b0[3 + a] + margin), hi_b = f32_narrow_up(b1[3 + a] + margin);
    lo0[a] = lo_a; dlo[a] = lo_b - lo_a;
    hi0[a] = hi_a; dhi[a] = hi_b - hi_a;
    if (dlo[a] != 0.0f || dhi[a] != 0.0f) moves |= 1u << a;
  }
  return moves;
}

// The same axis bits read back from n finished records: what motion_child_planes returned, ORed, when it wrote them.
RT_HD uint32_t motion_slope_mask(const FlatMotion32* m, size_t n) {
  uint32_t moves = 0u;
  for (size_t i = 0; i < n; ++i)
    for (int c = 0; c < 2; ++c)
      for (int a = 0; a < 3; ++a)
        if (m[i].dlo[c][a] != 0.0f || m[i].dhi[c][a] != 0.0f) moves |= 1u << a;
  return moves;
}

// nextafterf(f, -inf) / (f, +inf) for ANY f (f32_step_* of member_box.hpp take a finite f or the far infinity only).
RT_HD float f32_next_down(float f) { return (f != f || f == -__builtin_huge_valf()) ? f : f32_step_down(f); }
RT_HD float f32_next_up(float f) { return (f != f || f == __builtin_huge_valf()) ? f : f32_step_up(f); }

// The f32 box of a plain MovingSphere in the world list (WorldDesc::box under WD_TIME_BOX): centre(t) is linear in t
// (hit.rs:275-278), so the boxes at time0 and time1 bound every time between them; the (float) cast rounds to nearest, and two
// steps outward cover it and the rounding of the f64 sum.  Axis by axis, stopping at the first plane that is not finite: the
// planes behind it keep what box[] held (the slot's unbounded top_box32).  true: all six are finite and time0 < time1, and the
// slot may carry WD_TIME_BOX.
RT_HD bool mover_slot_box32(const FlatMovingSphere& ms, float* box) {
  const double r = rt_fabs((double)ms.radius);
  bool finite = (double)ms.time0 < (double)ms.time1;
  for (int a = 0; a < 3 && finite; ++a) {
    const double mn = rt_fmin((double)ms.c0[a], (double)ms.c1[a]) - r, mx = rt_fmax((double)ms.c0[a], (double)ms.c1[a]) + r;
    float lo = f32_next_down((float)mn), hi = f32_next_up((float)mx);
    lo = f32_next_down(lo); hi = f32_next_up(hi);
    box[a] = lo; box[3 + a] = hi;
    finite = rt_fabs(lo) < __builtin_huge_valf() && rt_fabs(hi) < __builtin_huge_valf();
  }
  return finite;
}

}  // namespace rt
