// The light table of next-event estimation (core/integrator.hpp: FlatLight, LightView), built on the host from a flattened
// scene so that the upload (render.hip), rtx_flat_lights (abi.cpp) and the tests' host checker all see the same table.
//
// A sampled light is a top-level ENTRY_PRIM slot whose primitive is a rectangle (any axis) or a static sphere and whose
// material is DiffuseLight.  Such a slot has, by construction of the flat entries, no transform and no medium around it.
// Every other emitter -- in a BVH or a group, under Translate / RotateY, a moving, gravity or triangle primitive -- is an
// unsampled emitter: the material's own sampling reaches it, with MIS weight 1.
// Lights are picked with probability proportional to area x the max channel of the emitted colour at the light's centre
// (uniformly if every such weight is 0); FlatLight::pmf is the exact probability the draw gives (cdf differences).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "../core/integrator.hpp"
#include "flat_scene.hpp"

namespace rt {

// ---- what the host builder below and rtx_scene_set_spheres' k_refresh_lights (hip/mesh_update.inc) share, so that a light
// table recomputed on the device equals the one built from scratch byte for byte.
// The area of light L and its centre, from the primitive as it now stands.
RT_HD real light_area_centre(const FlatLight& L, const FlatSphere* spheres, const FlatRect* rects, Point3* centre) {
  if (L.kind == LIGHT_RECT) {
    const FlatRect& r = rects[L.prim];
    const real a = (r.a0 + r.a1) * real(0.5), b = (r.b0 + r.b1) * real(0.5);
    *centre = r.axis == RECT_XY ? v3(a, b, r.k) : (r.axis == RECT_XZ ? v3(a, r.k, b) : v3(r.k, a, b));
    return (real)(rt_fabs((double)(r.a1 - r.a0)) * rt_fabs((double)(r.b1 - r.b0)));
  }
  const FlatSphere& sp = spheres[L.prim];
  *centre = v3(sp.cx, sp.cy, sp.cz);
  return (real)(4.0 * 3.14159265358979323846 * (double)sp.radius * (double)sp.radius);
}
// The pick weight of a light: its area times the max channel of the emitted colour at its centre -- Texture::value at
// (0.5, 0.5, centre) of the light's texture tree -- and 0 unless that is finite and positive.
RT_HD double light_pick_weight(const SceneView& sv, int32_t mat, real area, Point3 centre) {
  const Color c = texture_value<F_ALL, false>(sv, sv.materials[mat].tex, real(0.5), real(0.5), centre, nullptr);
  // (std::max's comparisons, spelled out: what a NaN channel does is part of the table's bytes)
  const double yz = (double)c.y < (double)c.z ? (double)c.z : (double)c.y;
  const double m = (double)c.x < yz ? yz : (double)c.x;
  const double inf = __builtin_huge_val();
  return rt_fabs(m) < inf && m > 0.0 && rt_fabs((double)area) < inf ? (double)area * m : 0.0;
}
// weight[0 .. n) -> cdf and pmf of lights[0 .. n): the serial sum, uniform weights when it is not positive and finite,
// cdf = 1 for the last light.  Serial on purpose: the order of the additions is part of the bytes.
RT_HD void light_cdf_pass(FlatLight* lights, double* weight, int32_t n) {
  double sum = 0.0;
  for (int32_t k = 0; k < n; ++k) sum += weight[k];
  if (!(sum > 0.0) || !(rt_fabs(sum) < __builtin_huge_val())) {
    for (int32_t k = 0; k < n; ++k) weight[k] = 1.0;
    sum = (double)n;
  }
  double acc = 0.0, prev = 0.0;
  for (int32_t k = 0; k < n; ++k) {
    acc += weight[k];
    const double cdf = k + 1 == n ? 1.0 : acc / sum;
    lights[k].cdf = (real)cdf;
    lights[k].pmf = (real)(cdf - prev);
    prev = cdf;
  }
}

}  // namespace rt

namespace rtx {

struct LightTable {
  std::vector<rt::FlatLight> lights;
  std::vector<int32_t> slot_light;  // one per top-level slot
  int32_t n_rect = 0, n_sphere = 0, n_unsampled = 0;
  double total_area = 0.0;
};

namespace light_detail {
inline bool is_light_mat(const FlatScene& fs, int32_t mat) {
  return mat >= 0 && (size_t)mat < fs.materials.size() && fs.materials[mat].kind == rt::MAT_DIFFUSE_LIGHT;
}
inline int32_t prim_mat(const FlatScene& fs, rt::PrimRef ref) {
  const uint32_t i = rt::primref_index(ref);
  switch (rt::primref_type(ref)) {
    case rt::PRIM_SPHERE: return fs.spheres[i].mat;
    case rt::PRIM_MOVING_SPHERE: return fs.moving_spheres[i].mat;
    case rt::PRIM_RECT: return fs.rects[i].mat;
    case rt::PRIM_TRIANGLE: return fs.triangles[i].mat;
    default: return fs.gravity_spheres[i].mat;
  }
}
// Does the geometry of entry e (any kind, transforms and media included) hold an emitting primitive?
inline bool entry_emits(const FlatScene& fs, int32_t e, int guard = 0) {
  if (guard > 16) return false;
  const rt::FlatEntry& E = fs.entries[e];
  switch (E.kind) {
    case rt::ENTRY_PRIM: return is_light_mat(fs, prim_mat(fs, (rt::PrimRef)E.a));
    case rt::ENTRY_GROUP:
    case rt::ENTRY_BVH: {
      const int32_t first = E.kind == rt::ENTRY_GROUP ? E.a : E.b, count = E.kind == rt::ENTRY_GROUP ? E.b : E.c;
      for (int32_t k = 0; k < count; ++k)
        if (is_light_mat(fs, prim_mat(fs, fs.refs[first + k]))) return true;
      return false;
    }
    case rt::ENTRY_XFORM: return entry_emits(fs, E.a, guard + 1);
    case rt::ENTRY_MEDIUM: return is_light_mat(fs, E.b) || entry_emits(fs, E.a, guard + 1);
    default: return false;
  }
}
}  // namespace light_detail

inline LightTable build_light_table(const FlatScene& fs) {
  using namespace light_detail;
  LightTable t;
  t.slot_light.assign(fs.top_level.size(), -1);
  std::vector<double> weight;
  const rt::SceneView sv = fs.view();
  for (size_t s = 0; s < fs.top_level.size(); ++s) {
    const int32_t e = fs.top_level[s];
    const rt::FlatEntry& E = fs.entries[e];
    bool sampled = false;
    if (E.kind == rt::ENTRY_PRIM) {
      const rt::PrimRef ref = (rt::PrimRef)E.a;
      const uint32_t type = rt::primref_type(ref), i = rt::primref_index(ref);
      const int32_t mat = prim_mat(fs, ref);
      if ((type == rt::PRIM_RECT || type == rt::PRIM_SPHERE) && is_light_mat(fs, mat)) {
        rt::FlatLight L;
        memset(&L, 0, sizeof(L));
        L.slot = (int32_t)s;
        L.prim = (int32_t)i;
        L.mat = mat;
        L.kind = type == rt::PRIM_RECT ? rt::LIGHT_RECT : rt::LIGHT_SPHERE;
        (type == rt::PRIM_RECT ? t.n_rect : t.n_sphere) += 1;
        rt::Point3 centre;
        L.area = rt::light_area_centre(L, fs.spheres.data(), fs.rects.data(), &centre);
        weight.push_back(rt::light_pick_weight(sv, mat, L.area, centre));
        t.total_area += (double)L.area;
        t.slot_light[s] = (int32_t)t.lights.size();
        t.lights.push_back(L);
        sampled = true;
      }
    }
    if (!sampled && entry_emits(fs, e)) t.n_unsampled += 1;
  }
  rt::light_cdf_pass(t.lights.data(), weight.data(), (int32_t)t.lights.size());
  return t;
}

}  // namespace rtx
