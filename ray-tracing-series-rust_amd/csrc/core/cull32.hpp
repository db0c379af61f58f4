// Conservative single-precision box culling for BVH walks.
//
// The reference decides every hit with f64 primitive tests (hit.rs) and uses Aabb::hit
// (aabb.rs:23-61) only to skip subtrees.  Skipping is an optimisation: if a box test never says
// "miss" for a box the ray really enters, the set of primitive tests that can win is unchanged
// and so is the closest hit (with its tie rule).  This header provides such a test in f32:
//
//   * child boxes are rounded outward to f32 on the host (lo down, hi up);
//   * the ray is rounded to f32 once per bounce: o32 = fl(o), i32 ~ 1/d, oi = fl(o32*i32).  On the device
//     i32 = v_rcp_f32(fl(d)) (1 ulp; an f64 division here cost 45 VALU per bounce), on the host fl(1/d): with
//     u = 2^-24, i32 = (1/d)(1 + e1), |e1| <= 3u in the worse (device) case;
//   * per axis t = fma(plane, i32, -oi); the slab interval is [min, max] of the two planes;
//   * first-order error of each t against the real-arithmetic value T = (plane - o)/d:
//         t - T = T e1 - (o/d)(e2 + e3) + t e4     (e2: rounding of o, e3: of the product oi, e4: of the fma)
//         |t - T| <= 4u |t| + 2u |oi|
//     so the interval is widened by |t| * 2^-21 + E with E = 2^-21 * max_axis |oi| (8u |t| + 8u |oi|: twice and
//     four times the bound, which also swallows the second-order terms and the rounding of the widening
//     itself).  Because f(t) = t - |t| eps is monotone the widening is applied once, after the max / min over axes,
//     and as ONE comparison: "widened near > widened far"  <=>  tn - tf > (|tn| + |tf|) 2^-21 + 2E
//     (4 instructions per box instead of 6; the rounding of the difference, <= u (|tn| + |tf|), sits inside the slack);
//   * t_min is rounded down, the running closest distance is rounded up;
//   * a box passes unless the widened interval is provably empty (NaNs pass).
// A zero direction component gives i32 = inf and NaN/inf slab values; fminf/fmaxf ignore NaN so
// that axis simply stops culling (still conservative).  Host and device need not agree bit for bit
// here -- any conservative answer gives the same final hit -- so FMA use is fine.
//
// Boxes of transformed members (instance trees, host/flatten.cpp: member_world_box).  There the f64 decision is taken in the
// member's own frame, on a ray that went through up to RT_MAX_XFORM_OPS Translate / RotateY ops, while the box that culls it
// stands in world space: the rotated corners' min / max plus the offsets, computed in f64.  Two more errors enter:
//   * the box: each rotation is two products and a sum, each translation a sum: <= 3 * 2^-53 relative to the largest
//     magnitude M met on the way, per op;
//   * the ray: xform_ray rounds the same way, so the point the member test accepts lies within about 12 * 2^-53 (|o| + t|d| + M)
//     of a point of the exact member, mapped to world space.
// The first is covered on the box: every plane is pushed out by M * 2^-22, at least two f32 ulps of the plane whatever its own
// value (rounding outward alone gives an exactly representable plane no slack) and 2^31 times the f64 error of the ops.  The
// second scales with the ray, not with the box, and is covered where the ray's own errors are: the widening above is
// 2^-21 (|tn| + |tf|) + 2E in t, i.e. at least 2^-21 (|o| + t|d|) in space, 2^29 times larger.
#pragma once
#include "flat_types.hpp"

namespace rt {

struct Ray32 {
  float ix, iy, iz;     // fl(1/d)
  float oix, oiy, oiz;  // fl(o32 * i32)
  float err2;           // 2E, E = 2^-21 * max |oi| over axes with finite slope
  float t_min;          // rounded down
};

// Which plane of an axis is the near one, for the forms below that take the planes already picked (cull32_may_hit_nf,
// cull32_may_hit_nf_pos; the wide step's slab_interval_nf gets the same answer from the direction's sign bit, trace_vote.inc:
// wide_sign_pack): bit a set = the hi plane of axis a is the near one.  The sign is
// taken from the SLOPE the planes are multiplied by, not from the f64 direction: for every direction but -0.0 the two agree
// (a reciprocal keeps the sign, also where the narrowing underflows to -0.0f; an infinite component has a slope of +-0,
// whose planes all lie at +-0 or NaN whichever is picked), and for -0.0 -- slope -inf, or
// -2^60 under RT_F32 -- `d < 0` is false and picked lo as the near plane, whose distance then came out as +inf: a miss for a
// ray that runs inside the slab.  With the slope's sign near / far are min / max of the two plane distances for every input.
RT_HD uint32_t ray32_dir_neg(const Ray32& q) {
  return (q.ix < 0.0f ? 1u : 0u) | (q.iy < 0.0f ? 2u : 0u) | (q.iz < 0.0f ? 4u : 0u);
}

RT_HD float cull_round_up(real x) {  // an f32 >= x (inf stays inf)
  return (float)x * (x >= 0.0 ? 1.00000012f : 0.99999988f);
}

RT_HD Ray32 make_ray32(const Ray& r, real t_min) {
  Ray32 q;
  float ox = (float)r.origin.x, oy = (float)r.origin.y, oz = (float)r.origin.z;
#if defined(__HIP_DEVICE_COMPILE__)
  q.ix = __builtin_amdgcn_rcpf((float)r.direction.x);
  q.iy = __builtin_amdgcn_rcpf((float)r.direction.y);
  q.iz = __builtin_amdgcn_rcpf((float)r.direction.z);
#else
  q.ix = (float)(1.0 / r.direction.x);
  q.iy = (float)(1.0 / r.direction.y);
  q.iz = (float)(1.0 / r.direction.z);
#endif
#if defined(RT_F32)
  // Single-precision rays do have direction components of exactly 0 (a cancellation leaves nothing below one ulp), a few in
  // every 10^8 rays.  With 1/d = inf the planes of that axis come out as +-inf or NaN, the widening below becomes inf and no
  // box can be ruled out any more: such a ray walked the WHOLE tree, alone in its wave (the dragon room: 4 rays, 0.4 s).
  // The fast mode gives such an axis a finite slope of 2^60 instead: a ray outside the slab sees both planes at the same huge
  // distance and is culled, a ray inside sees (-huge, +huge).  The axis is left out of the error term like an infinite one
  // (its distances only matter through their sign; 2^60 is a power of two, so its products are exact).
  // Only a slope that is NOT finite is replaced (d = +-0, a denormal d, NaN -> -2^60): a finite slope, however steep, is the
  // ray's own and stays -- capping it too (as a clamp into +-2^60 did) shortened every plane distance of a component below
  // 2^-60 and culled boxes such a ray enters.  A steep finite slope counts in the error term like any other, which switches
  // culling off for that ray (|o| 2^60 2^-20 and more): rarer than the zeros, and correct.
  // What the replacement gives up: an origin EXACTLY on a plane of a zero-component axis sees that plane at t = 0
  // (fma(p, 2^60, -p 2^60) = 0) instead of "inside for all t", so a ray that runs in a face of the box (closed box: a touch) is
  // culled when the plane is the far one and t_min > 0.  A touch of measure zero; the float CPU oracle shares this code and
  // the verdict (tests/test_cull_conservative.py counts the class and excepts nothing else).
  // (Two compares and two selects per axis and bounce.  Not free: the fast mode's C2 is 1.3 % slower for it, Book-2 0.6 %; a clamp
  // taken only where the slope is not finite measured worse on C2, -1.9 %.  DESIGN.md 5.6.)
  const float slope_cap = 0x1.0p60f;
  q.ix = __builtin_fabsf(q.ix) < __builtin_huge_valf() ? q.ix : (q.ix > 0.0f ? slope_cap : -slope_cap);
  q.iy = __builtin_fabsf(q.iy) < __builtin_huge_valf() ? q.iy : (q.iy > 0.0f ? slope_cap : -slope_cap);
  q.iz = __builtin_fabsf(q.iz) < __builtin_huge_valf() ? q.iz : (q.iz > 0.0f ? slope_cap : -slope_cap);
  q.oix = ox * q.ix; q.oiy = oy * q.iy; q.oiz = oz * q.iz;
  float ax = __builtin_fabsf(q.ix) != slope_cap ? __builtin_fabsf(q.oix) : 0.0f;
  float ay = __builtin_fabsf(q.iy) != slope_cap ? __builtin_fabsf(q.oiy) : 0.0f;
  float az = __builtin_fabsf(q.iz) != slope_cap ? __builtin_fabsf(q.oiz) : 0.0f;
#else
  const float finite_slope = 1e30f;
  q.oix = ox * q.ix; q.oiy = oy * q.iy; q.oiz = oz * q.iz;
  float ax = __builtin_fabsf(q.ix) < finite_slope ? __builtin_fabsf(q.oix) : 0.0f;
  float ay = __builtin_fabsf(q.iy) < finite_slope ? __builtin_fabsf(q.oiy) : 0.0f;
  float az = __builtin_fabsf(q.iz) < finite_slope ? __builtin_fabsf(q.oiz) : 0.0f;
#endif
  q.err2 = __builtin_fmaxf(ax, __builtin_fmaxf(ay, az)) * 0x1.0p-20f;
  // rounded DOWN whatever the sign (a medium's second boundary query may start at a negative t)
  q.t_min = (float)t_min * (t_min >= 0.0 ? 0.99999988f : 1.00000012f);
  return q;
}

// true unless the ray provably misses the box within (t_min, t_max32]
RT_HD bool cull32_may_hit(const float* lo, const float* hi, const Ray32& q, float t_max32) {
  float ax = __builtin_fmaf(lo[0], q.ix, -q.oix), bx = __builtin_fmaf(hi[0], q.ix, -q.oix);
  float ay = __builtin_fmaf(lo[1], q.iy, -q.oiy), by = __builtin_fmaf(hi[1], q.iy, -q.oiy);
  float az = __builtin_fmaf(lo[2], q.iz, -q.oiz), bz = __builtin_fmaf(hi[2], q.iz, -q.oiz);
  float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(ax, bx), __builtin_fminf(ay, by)),
                             __builtin_fmaxf(__builtin_fminf(az, bz), q.t_min));
  float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(ax, bx), __builtin_fmaxf(ay, by)),
                             __builtin_fminf(__builtin_fmaxf(az, bz), t_max32));
  return !(tn - tf > __builtin_fmaf(__builtin_fabsf(tn) + __builtin_fabsf(tf), 0x1.0p-21f, q.err2));
}

// The same test with the near / far plane of every axis already picked by the sign of the ray's slope (ray32_dir_neg: near =
// lo where the ray travels towards +axis, hi otherwise).  For a finite slope the near value IS min(a, b) and the far value
// max(a, b) of cull32_may_hit, so tn / tf -- and the verdict -- are the same numbers; for a zero direction component
// both are NaN and fmaxf / fminf drop them, exactly as there.  What it saves is the six min / max per box that only
// sorted the two planes: on gfx950 v_min_f32 / v_max_f32 issue in 4 clocks, twice a v_fma_f32.
RT_HD bool cull32_may_hit_nf(float nx, float fx, float ny, float fy, float nz, float fz, const Ray32& q, float t_max32) {
  const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(__builtin_fmaf(nx, q.ix, -q.oix), __builtin_fmaf(ny, q.iy, -q.oiy)),
                                                   __builtin_fmaf(nz, q.iz, -q.oiz)), q.t_min);
  const float tf = __builtin_fminf(__builtin_fminf(__builtin_fminf(__builtin_fmaf(fx, q.ix, -q.oix), __builtin_fmaf(fy, q.iy, -q.oiy)),
                                                   __builtin_fmaf(fz, q.iz, -q.oiz)), t_max32);
  return !(tn - tf > __builtin_fmaf(__builtin_fabsf(tn) + __builtin_fabsf(tf), 0x1.0p-21f, q.err2));
}

// The same verdict for queries whose t_min is POSITIVE (every ray_color query: world.hit(r, 0.001, inf), world.rs:77 -- not the
// second boundary query of a medium), written so that it costs three instructions after the min / max: with tn >= t_min > 0,
//     tn - tf > (tn + |tf|) e + 2E   <=>   tn (1 - e) - 2E  >  tf + |tf| e            (e = 2^-21; 1 - e is an exact f32)
// one fma per side (|tf| is a free source modifier) and one compare; the roundings of the two fmas are of the size of the one
// the difference had (<= u (tn + |tf|)), inside the same slack.
RT_HD bool cull32_may_hit_nf_pos(float nx, float fx, float ny, float fy, float nz, float fz, const Ray32& q, float t_max32) {
  const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(__builtin_fmaf(nx, q.ix, -q.oix), __builtin_fmaf(ny, q.iy, -q.oiy)),
                                                   __builtin_fmaf(nz, q.iz, -q.oiz)), q.t_min);
  const float tf = __builtin_fminf(__builtin_fminf(__builtin_fminf(__builtin_fmaf(fx, q.ix, -q.oix), __builtin_fmaf(fy, q.iy, -q.oiy)),
                                                   __builtin_fmaf(fz, q.iz, -q.oiz)), t_max32);
  return !(__builtin_fmaf(tn, 1.0f - 0x1.0p-21f, -q.err2) > __builtin_fmaf(__builtin_fabsf(tf), 0x1.0p-21f, tf));
}

// Both children of a node at once.  Same arithmetic as two cull32_may_hit calls; on the device the twelve plane
// fmas are written as four 2-wide ones (x and y of a plane set) plus four scalar ones for z, so that the pairs
// issue as v_pk_fma_f32 -- an fma gives the same value whichever instruction carries it.
RT_HD void cull32_may_hit2(const float* lo0, const float* hi0, const float* lo1, const float* hi1, const Ray32& q,
                           float t_max32, bool* hit0, bool* hit1) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef float f2 __attribute__((ext_vector_type(2)));
  const f2 ixy = {q.ix, q.iy}, oxy = {-q.oix, -q.oiy};
  const float noz = -q.oiz;
  // x and y of one plane set are adjacent in memory (they arrive as one register pair): pack those
  const f2 a0 = __builtin_elementwise_fma((f2){lo0[0], lo0[1]}, ixy, oxy), b0 = __builtin_elementwise_fma((f2){hi0[0], hi0[1]}, ixy, oxy);
  const f2 a1 = __builtin_elementwise_fma((f2){lo1[0], lo1[1]}, ixy, oxy), b1 = __builtin_elementwise_fma((f2){hi1[0], hi1[1]}, ixy, oxy);
  const float az0 = __builtin_fmaf(lo0[2], q.iz, noz), bz0 = __builtin_fmaf(hi0[2], q.iz, noz);
  const float az1 = __builtin_fmaf(lo1[2], q.iz, noz), bz1 = __builtin_fmaf(hi1[2], q.iz, noz);
  float tn0 = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(a0.x, b0.x), __builtin_fminf(a0.y, b0.y)),
                              __builtin_fmaxf(__builtin_fminf(az0, bz0), q.t_min));
  float tf0 = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(a0.x, b0.x), __builtin_fmaxf(a0.y, b0.y)),
                              __builtin_fminf(__builtin_fmaxf(az0, bz0), t_max32));
  float tn1 = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(a1.x, b1.x), __builtin_fminf(a1.y, b1.y)),
                              __builtin_fmaxf(__builtin_fminf(az1, bz1), q.t_min));
  float tf1 = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(a1.x, b1.x), __builtin_fmaxf(a1.y, b1.y)),
                              __builtin_fminf(__builtin_fmaxf(az1, bz1), t_max32));
  *hit0 = !(tn0 - tf0 > __builtin_fmaf(__builtin_fabsf(tn0) + __builtin_fabsf(tf0), 0x1.0p-21f, q.err2));
  *hit1 = !(tn1 - tf1 > __builtin_fmaf(__builtin_fabsf(tn1) + __builtin_fabsf(tf1), 0x1.0p-21f, q.err2));
#else
  *hit0 = cull32_may_hit(lo0, hi0, q, t_max32);
  *hit1 = cull32_may_hit(lo1, hi1, q, t_max32);
#endif
}

}  // namespace rt
