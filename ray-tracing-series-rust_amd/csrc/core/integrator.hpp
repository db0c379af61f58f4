// One camera path = one (pixel, sample) of render_scene's inner loop.
//
// Reference: /root/reference/src/world.rs:1211-1215 (jitter, primary ray,
// accumulate) and world.rs:52-93 (ray_color's iterative bounce loop).  The path
// is exposed as begin/step so the device can interleave many paths per lane
// (regeneration) while the CPU checker simply loops step() to completion; both
// execute the same arithmetic in the same order.
#pragma once
#include "shading.hpp"

namespace rt {

struct PathState {
  Ray ray;
  Color product;  // world.rs:59
  Color output;   // world.rs:60
  int32_t depth;  // world.rs:56 (counts down)
  Rng rng;
};

// world.rs:1212-1214: u = (i + rand)/(w-1), v = (j + rand)/(h-1), cam.get_ray(u, v).
// (i, j) = (column, row) with j = 0 the BOTTOM row, as the reference's Screen stores it.
RT_HD void path_begin(const RenderParams& rp, uint32_t i, uint32_t j, uint32_t sample, PathState* ps) {
  uint64_t pixel_index = (uint64_t)j * (uint64_t)rp.image_width + (uint64_t)i;
  ps->rng = rng_for_sample(rp.seed, pixel_index, sample);
  real ru = rng_f64(ps->rng);
  real u = ((real)i + ru) / (real)(rp.image_width - 1);
  real rv = rng_f64(ps->rng);
  real v = ((real)j + rv) / (real)(rp.image_height - 1);
  ps->ray = camera_get_ray(rp.cam, u, v, ps->rng);
  ps->product = v3(1, 1, 1);
  ps->output = v3(0, 0, 0);
  ps->depth = rp.max_depth;
}

// One iteration of ray_color's loop, in two halves around the world.hit() query so the device
// can run the query as a resumable walk:
//   path_bounce_begin   world.rs:64-67  depth -= 1; exhausted paths end with what they gathered
//   path_bounce_end     world.rs:68-90  miss -> background; hit -> scatter (draws), emitted, update
// Both return true when the path has ended and ps->output holds the sample's radiance.
RT_HD bool path_bounce_begin(PathState* ps) {
  ps->depth -= 1;
#if defined(RT_F32)
  // A ray that is not finite (a plane hit at t = inf behind a direction component of exactly 0 -- single-precision rays
  // have those -- leaves a NaN hit point) can hit nothing, yet no box test can rule it out: it would visit every node and
  // every primitive of every BVH, alone in its wave.  The fast mode ends such a path with what it has gathered.
  const real mag = rt_fabs(ps->ray.origin.x) + rt_fabs(ps->ray.origin.y) + rt_fabs(ps->ray.origin.z) +
                   rt_fabs(ps->ray.direction.x) + rt_fabs(ps->ray.direction.y) + rt_fabs(ps->ray.direction.z);
  if (!(mag < RT_INFINITY)) return true;
#endif
  return ps->depth < 0;
}

template <uint32_t F, bool COUNT>
RT_HD bool path_bounce_end(const SceneView& sv, const RenderParams& rp, PathState* ps, bool hit,
                           const HitRecord& rec, TraceCounters* cnt) {
  if (!hit) {
    ps->output += ps->product * rp.background;  // world.rs:86-89
    return true;
  }
  const FlatMaterial& m = sv.materials[rec.mat];
  Ray scattered;
  Color attenuation;
  // world.rs:69-84: scatter first (it draws from the stream), then emitted.
  bool did_scatter = material_scatter<F, COUNT>(sv, m, ps->ray, rec, ps->rng, &scattered, &attenuation, cnt);
  Color emitted = material_emitted<F, COUNT>(sv, m, rec, cnt);
  ps->output += emitted * ps->product;
  if (!did_scatter) return true;
  ps->product *= attenuation;
  ps->ray = scattered;
  return false;
}

// ---- next-event estimation with multiple importance sampling (opt-in; rtx_render_ex) ------------
// A statistical extension, not the reference's estimator: at every Lambertian / Isotropic vertex the path also connects to a
// point drawn on one of the scene's sampled lights (plain top-level rectangles and static spheres of DiffuseLight, the table
// host/light_table.hpp builds), and both that connection and a scattered ray that hits the same light are weighted with the
// power heuristic.  With an empty table the functions below draw and add exactly what path_bounce_end does.
enum LightKind : int32_t { LIGHT_RECT = 0, LIGHT_SPHERE = 1 };
struct FlatLight {  // 40 B
  int32_t kind;  // LightKind
  int32_t slot;  // its top-level slot
  int32_t prim;  // index into rects / spheres
  int32_t mat;   // its DiffuseLight material
  real area;     // rectangle: |a1 - a0| |b1 - b0|; sphere: 4 pi r^2 (the census)
  real cdf;      // the light draw u picks the first light with u < cdf (the last one's is 1)
  real pmf;      // cdf minus the previous light's cdf: the exact probability of picking this light
};
struct LightView {
  const FlatLight* lights;
  const int32_t* slot_light;  // per top-level slot: the index of its light, -1 when the slot is not a sampled light
  int32_t n_lights;
  int32_t pad;
};

// The shadow ray covers t in [ray_t_min, 1 - RT_NEE_SHADOW_EPS] of q - p: the sampled point itself lies at t = 1.
#define RT_NEE_SHADOW_EPS real(1e-6)

// Power heuristic (beta = 2) of the strategy with pdf a against the one with pdf b.
RT_HD real mis_power(real a, real b) {
  const real a2 = a * a, b2 = b * b;
  return a2 / (a2 + b2);
}

// Solid-angle pdf of the uniform area sample of a rectangle seen along d = q - p: d^2 / (|cos theta_l| A) = |d|^3 / (|d.n| A).
// Both faces emit (DiffuseLight ignores the face, Q6), hence |cos|.
RT_HD real light_pdf_rect(const FlatRect& q, real area, Vec3 d) {
  const real dn = rt_fabs(q.axis == RECT_XY ? d.z : (q.axis == RECT_XZ ? d.y : d.x));
  const real d2 = length_squared(d);
  return d2 * rt_sqrt(d2) / (dn * area);
}
// 1 - cos(theta_max) of the cone a sphere (centre c, radius r) subtends from p, without cancellation; 0 when p is inside.
RT_HD real sphere_cone_one_minus(const FlatSphere& s, Point3 p) {
  const Vec3 oc = v3(s.cx, s.cy, s.cz) - p;
  const real d2 = length_squared(oc), r2 = s.radius * s.radius;
  if (!(d2 > r2)) return real(0.0);
  const real k = r2 / d2;
  return k / (real(1.0) + rt_sqrt(real(1.0) - k));
}
// Solid-angle pdf of the uniform cone sample of a sphere from p (0 from inside it).
RT_HD real light_pdf_sphere(const FlatSphere& s, Point3 p) {
  const real om = sphere_cone_one_minus(s, p);
  return om > real(0.0) ? real(1.0) / (real(2.0) * RT_PI * om) : real(0.0);
}
// Probability density (solid angle at p, light choice included) that next-event estimation samples the point q of light k.
RT_HD real light_pdf(const SceneView& sv, const LightView& lv, int32_t k, Point3 p, Point3 q) {
  const FlatLight& L = lv.lights[k];
  const real ps = L.kind == LIGHT_RECT ? light_pdf_rect(sv.rects[L.prim], L.area, q - p) : light_pdf_sphere(sv.spheres[L.prim], p);
  return L.pmf * ps;
}

// The solid-angle pdf with which the material scattered towards dir: Lambertian cos / pi about rec.normal (normal +
// random_unit_vector is exactly that lobe), Isotropic 1 / (4 pi).  Negative: the vertex does not take part (weight 1).
RT_HD real nee_bsdf_pdf(int32_t kind, const HitRecord& rec, Vec3 dir) {
  if (kind == MAT_ISOTROPIC) return real(1.0) / (real(4.0) * RT_PI);
  const real c = dot(rec.normal, dir) / length(dir);
  return c > real(0.0) ? c / RT_PI : real(0.0);
}

// One light connection from the vertex rec (material kind `kind`, albedo = scatter's attenuation).  Draws the light, then
// two uniforms for its point, then whatever the shadow ray's media draw.  Returns what it adds to the path's output.
template <uint32_t F, bool COUNT, class STACK>
RT_HD Color nee_connect(const SceneView& sv, const LightView& lv, const PathState* ps, const HitRecord& rec, int32_t kind,
                        Color albedo, Rng& rng, STACK& stack, TraceCounters* cnt) {
  const real ul = rng_f64(rng);
  int32_t k = 0;
  while (k + 1 < lv.n_lights && !(ul < lv.lights[k].cdf)) ++k;
  const FlatLight& L = lv.lights[k];
  const real u1 = rng_f64(rng), u2 = rng_f64(rng);
  const Point3 p = rec.p;
  Point3 q;
  real pdf_sa;
  HitRecord lrec;  // the light's (u, v, p) for its texture
  lrec.u = real(0.0); lrec.v = real(0.0);
  if (L.kind == LIGHT_RECT) {
    const FlatRect& r = sv.rects[L.prim];
    const real a = r.a0 + u1 * (r.a1 - r.a0), b = r.b0 + u2 * (r.b1 - r.b0);
    q = r.axis == RECT_XY ? v3(a, b, r.k) : (r.axis == RECT_XZ ? v3(a, r.k, b) : v3(r.k, a, b));
    if (F & F_IMAGE) {
      lrec.u = (a - r.a0) / (r.a1 - r.a0);
      lrec.v = (b - r.b0) / (r.b1 - r.b0);
    }
    pdf_sa = light_pdf_rect(r, L.area, q - p);
  } else {
    const FlatSphere& s = sv.spheres[L.prim];
    const Point3 c = v3(s.cx, s.cy, s.cz);
    const real om = sphere_cone_one_minus(s, p);
    if (!(om > real(0.0))) return v3(0, 0, 0);  // p is inside the sphere: pdf 0
    const Vec3 w = unit(c - p);
    const Vec3 a = rt_fabs(w.x) > real(0.9) ? v3(0, 1, 0) : v3(1, 0, 0);
    const Vec3 vv = unit(cross(w, a));
    const Vec3 uu = cross(w, vv);
    const real z = real(1.0) - u2 * om;
    const real phi = real(2.0) * RT_PI * u1;
    const real st = rt_sqrt(rt_fmax(real(0.0), real(1.0) - z * z));
    const Vec3 dir = uu * (rt_cos(phi) * st) + vv * (rt_sin(phi) * st) + w * z;
    const Vec3 po = p - c;
    const real hb = dot(po, dir);
    const real disc = rt_fmax(real(0.0), hb * hb - (length_squared(po) - s.radius * s.radius));
    q = p + (-hb - rt_sqrt(disc)) * dir;
    if (F & F_IMAGE) {
      if (sv.materials[L.mat].needs_uv) get_sphere_uv((q - c) / s.radius, &lrec.u, &lrec.v);
    }
    pdf_sa = real(1.0) / (real(2.0) * RT_PI * om);
  }
  const real p_light = L.pmf * pdf_sa;
  if (!(p_light > real(0.0)) || !(p_light < RT_INFINITY)) return v3(0, 0, 0);
  const Vec3 d = q - p;
  Color f;
  real p_bsdf;
  if (kind == MAT_ISOTROPIC) {
    p_bsdf = real(1.0) / (real(4.0) * RT_PI);
    f = albedo * p_bsdf;
  } else {
    const real c = dot(rec.normal, d) / length(d);
    if (!(c > real(0.0))) return v3(0, 0, 0);
    p_bsdf = c / RT_PI;
    f = albedo * p_bsdf;
  }
  const Ray shadow = make_ray(p, d, ps->ray.time);
  HitRecord srec;
  if (world_hit<F, COUNT>(sv, shadow, ray_t_min(shadow), real(1.0) - RT_NEE_SHADOW_EPS, &srec, rng, stack, cnt))
    return v3(0, 0, 0);
  lrec.p = q;
  const Color le = material_texture_value<F, COUNT>(sv, sv.materials[L.mat], lrec, cnt);
  return ps->product * f * le * (mis_power(p_light, p_bsdf) / p_light);
}

// path_bounce_end with next-event estimation.  hit_slot: the top-level slot of the hit (world_hit<..., SLOT = true>);
// *last_pdf: the pdf with which the previous vertex scattered this ray when that vertex took part, else negative.
template <uint32_t F, bool COUNT, class STACK>
RT_HD bool path_bounce_end_nee(const SceneView& sv, const LightView& lv, const RenderParams& rp, PathState* ps, real* last_pdf,
                               bool hit, const HitRecord& rec, int32_t hit_slot, STACK& stack, TraceCounters* cnt) {
  if (!hit) {
    ps->output += ps->product * rp.background;  // world.rs:86-89
    return true;
  }
  const FlatMaterial& m = sv.materials[rec.mat];
  Ray scattered;
  Color attenuation = v3(0, 0, 0);
  bool did_scatter = material_scatter<F, COUNT>(sv, m, ps->ray, rec, ps->rng, &scattered, &attenuation, cnt);
  Color emitted = material_emitted<F, COUNT>(sv, m, rec, cnt);
  if (*last_pdf >= real(0.0)) {
    const int32_t k = lv.slot_light[hit_slot];
    if (k >= 0) {  // a sampled light reached by the material's own sampling: weight against the light strategy
      const real pl = light_pdf(sv, lv, k, ps->ray.origin, rec.p);
      if (pl > real(0.0)) emitted = emitted * mis_power(*last_pdf, pl);
    }
  }
  ps->output += emitted * ps->product;
  if (!did_scatter) return true;
  *last_pdf = real(-1.0);
  // the connection counts as the next hit: only where path_bounce_begin would still allow one (depth - 1 >= 0)
  if (lv.n_lights > 0 && ps->depth >= 1 && (m.kind == MAT_LAMBERTIAN || m.kind == MAT_ISOTROPIC)) {
    ps->output += nee_connect<F, COUNT>(sv, lv, ps, rec, m.kind, attenuation, ps->rng, stack, cnt);
    *last_pdf = nee_bsdf_pdf(m.kind, rec, scattered.direction);
  }
  ps->product *= attenuation;
  ps->ray = scattered;
  return false;
}

template <uint32_t F, bool COUNT, class STACK>
RT_HD bool path_step_nee(const SceneView& sv, const LightView& lv, const RenderParams& rp, PathState* ps, real* last_pdf,
                         STACK& stack, TraceCounters* cnt) {
  if (path_bounce_begin(ps)) return true;
  HitRecord rec;
  int32_t slot = -1;
  bool hit = world_hit<F, COUNT, STACK, true>(sv, ps->ray, ray_t_min(ps->ray), RT_INFINITY, &rec, ps->rng, stack, cnt, &slot);
  return path_bounce_end_nee<F, COUNT>(sv, lv, rp, ps, last_pdf, hit, rec, slot, stack, cnt);
}

// Whole next-event-estimation sample on one thread (the host checker; k_trace_nee runs the same steps).
template <uint32_t F, bool COUNT, class STACK>
RT_HD Color trace_sample_nee(const SceneView& sv, const LightView& lv, const RenderParams& rp, uint32_t i, uint32_t j,
                             uint32_t sample, STACK& stack, TraceCounters* cnt) {
  PathState ps;
  path_begin(rp, i, j, sample, &ps);
  if (COUNT) cnt->samples++;
  real last_pdf = real(-1.0);
  while (!path_step_nee<F, COUNT>(sv, lv, rp, &ps, &last_pdf, stack, cnt)) {
  }
  return ps.output;
}

template <uint32_t F, bool COUNT, class STACK>
RT_HD bool path_step(const SceneView& sv, const RenderParams& rp, PathState* ps, STACK& stack,
                     TraceCounters* cnt) {
  if (path_bounce_begin(ps)) return true;
  HitRecord rec;
  bool hit = world_hit<F, COUNT>(sv, ps->ray, ray_t_min(ps->ray), RT_INFINITY, &rec, ps->rng, stack, cnt);
  return path_bounce_end<F, COUNT>(sv, rp, ps, hit, rec, cnt);
}

// Whole sample on one thread (CPU checker; also the device's simplest kernel).
template <uint32_t F, bool COUNT, class STACK>
RT_HD Color trace_sample(const SceneView& sv, const RenderParams& rp, uint32_t i, uint32_t j,
                         uint32_t sample, STACK& stack, TraceCounters* cnt) {
  PathState ps;
  path_begin(rp, i, j, sample, &ps);
  if (COUNT) cnt->samples++;
  while (!path_step<F, COUNT>(sv, rp, &ps, stack, cnt)) {
  }
  return ps.output;
}

// ---- radiance queries: a path that starts from a caller's ray (rtx_scene_trace_rays*) ------------
// The ray is taken as given: no jitter, lens or shutter draw is made, so the first draw of the stream of
// (seed, ray_index, sample) belongs to the first bounce.  rp's camera and image size are not read.
RT_HD void path_begin_ray(const RenderParams& rp, const Ray& ray, uint64_t ray_index, uint32_t sample, PathState* ps) {
  ps->rng = rng_for_sample(rp.seed, ray_index, sample);
  ps->ray = ray;
  ps->product = v3(1, 1, 1);
  ps->output = v3(0, 0, 0);
  ps->depth = rp.max_depth;
}

// Whole sample of a given ray on one thread (the host checker; k_trace_rays runs the same steps).
template <uint32_t F, bool COUNT, class STACK>
RT_HD Color trace_ray_sample(const SceneView& sv, const RenderParams& rp, const Ray& ray, uint64_t ray_index, uint32_t sample,
                             STACK& stack, TraceCounters* cnt) {
  PathState ps;
  path_begin_ray(rp, ray, ray_index, sample, &ps);
  if (COUNT) cnt->samples++;
  while (!path_step<F, COUNT>(sv, rp, &ps, stack, cnt)) {
  }
  return ps.output;
}

template <uint32_t F, bool COUNT, class STACK>
RT_HD Color trace_ray_sample_nee(const SceneView& sv, const LightView& lv, const RenderParams& rp, const Ray& ray,
                                 uint64_t ray_index, uint32_t sample, STACK& stack, TraceCounters* cnt) {
  PathState ps;
  path_begin_ray(rp, ray, ray_index, sample, &ps);
  if (COUNT) cnt->samples++;
  real last_pdf = real(-1.0);
  while (!path_step_nee<F, COUNT>(sv, lv, rp, &ps, &last_pdf, stack, cnt)) {
  }
  return ps.output;
}

// ---- gather queries: a path that starts AT a caller's point (rtx_scene_gather*) ------------------
// The start direction is drawn from the sample's own stream, so its first draws are random_unit_vector's rejection loop.
// Surface form: the path leaves p as if it had just scattered off a white Lambertian surface with the given normal
// (Lambertian::scatter's rule, hit.rs:1039-1051: normal + unit vector, the normal itself when that sum is near zero); the
// normal is taken as given, not normalised.  Probe form: the unit vector itself, uniform over the sphere.
RT_HD Vec3 gather_direction(Rng& rng, bool surface, Vec3 normal) {
  const Vec3 u = random_unit_vector(rng);
  if (!surface) return u;
  Vec3 dir = normal + u;
  if (near_zero(dir)) dir = normal;
  return dir;
}

// The start direction of sample `sample` of point `point_index` alone (rtx_gather_directions, k_reduce_samples_sh's replay).
RT_HD Vec3 gather_sample_direction(uint64_t seed, uint64_t point_index, uint32_t sample, bool surface, Vec3 normal) {
  Rng rng = rng_for_sample(seed, point_index, sample);
  return gather_direction(rng, surface, normal);
}

// The ray leaves p with the path's own ray_t_min, so a point that lies on a surface does not hit that surface.
RT_HD void path_begin_gather(const RenderParams& rp, Point3 p, Vec3 normal, bool surface, real time, uint64_t point_index,
                             uint32_t sample, PathState* ps) {
  ps->rng = rng_for_sample(rp.seed, point_index, sample);
  const Vec3 dir = gather_direction(ps->rng, surface, normal);
  ps->ray = make_ray(p, dir, time);
  ps->product = v3(1, 1, 1);
  ps->output = v3(0, 0, 0);
  ps->depth = rp.max_depth;
}

// The surface form under next-event estimation: the start vertex makes the light connection a diffuse vertex makes (after the
// scatter draw, as path_bounce_end_nee orders them; max_depth >= 1, so the connection is always allowed) with albedo (1, 1, 1),
// and the first ray carries the Lambertian pdf it was scattered with.
template <uint32_t F, bool COUNT, class STACK>
RT_HD void path_begin_gather_nee(const SceneView& sv, const LightView& lv, const RenderParams& rp, Point3 p, Vec3 normal, real time,
                                 uint64_t point_index, uint32_t sample, PathState* ps, real* last_pdf, STACK& stack,
                                 TraceCounters* cnt) {
  path_begin_gather(rp, p, normal, true, time, point_index, sample, ps);
  *last_pdf = real(-1.0);
  if (lv.n_lights > 0) {
    HitRecord rec;
    rec.p = p;
    rec.normal = normal;
    rec.t = real(0.0); rec.u = real(0.0); rec.v = real(0.0);
    rec.front_face = true;
    rec.mat = -1;
    ps->output += nee_connect<F, COUNT>(sv, lv, ps, rec, MAT_LAMBERTIAN, v3(1, 1, 1), ps->rng, stack, cnt);
    *last_pdf = nee_bsdf_pdf(MAT_LAMBERTIAN, rec, ps->ray.direction);
  }
}

// Whole gather sample on one thread (the host checker; k_gather runs the same steps).
template <uint32_t F, bool COUNT, class STACK>
RT_HD Color trace_gather_sample(const SceneView& sv, const RenderParams& rp, Point3 p, Vec3 normal, bool surface, real time,
                                uint64_t point_index, uint32_t sample, STACK& stack, TraceCounters* cnt) {
  PathState ps;
  path_begin_gather(rp, p, normal, surface, time, point_index, sample, &ps);
  if (COUNT) cnt->samples++;
  while (!path_step<F, COUNT>(sv, rp, &ps, stack, cnt)) {
  }
  return ps.output;
}

// surface = false: the probe form has no start vertex, so it is the plain start followed by path_step_nee.
template <uint32_t F, bool COUNT, class STACK>
RT_HD Color trace_gather_sample_nee(const SceneView& sv, const LightView& lv, const RenderParams& rp, Point3 p, Vec3 normal,
                                    bool surface, real time, uint64_t point_index, uint32_t sample, STACK& stack,
                                    TraceCounters* cnt) {
  PathState ps;
  real last_pdf = real(-1.0);
  if (surface) path_begin_gather_nee<F, COUNT>(sv, lv, rp, p, normal, time, point_index, sample, &ps, &last_pdf, stack, cnt);
  else path_begin_gather(rp, p, normal, false, time, point_index, sample, &ps);
  if (COUNT) cnt->samples++;
  while (!path_step_nee<F, COUNT>(sv, lv, rp, &ps, &last_pdf, stack, cnt)) {
  }
  return ps.output;
}

}  // namespace rt
