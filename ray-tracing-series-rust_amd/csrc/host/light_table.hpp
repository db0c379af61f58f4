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
        rt::Point3 centre;
        if (type == rt::PRIM_RECT) {
          const rt::FlatRect& r = fs.rects[i];
          L.kind = rt::LIGHT_RECT;
          L.area = (rt::real)(std::fabs((double)(r.a1 - r.a0)) * std::fabs((double)(r.b1 - r.b0)));
          const rt::real a = (r.a0 + r.a1) * rt::real(0.5), b = (r.b0 + r.b1) * rt::real(0.5);
          centre = r.axis == rt::RECT_XY ? rt::v3(a, b, r.k) : (r.axis == rt::RECT_XZ ? rt::v3(a, r.k, b) : rt::v3(r.k, a, b));
          t.n_rect += 1;
        } else {
          const rt::FlatSphere& sp = fs.spheres[i];
          L.kind = rt::LIGHT_SPHERE;
          L.area = (rt::real)(4.0 * M_PI * (double)sp.radius * (double)sp.radius);
          centre = rt::v3(sp.cx, sp.cy, sp.cz);
          t.n_sphere += 1;
        }
        // the emitted colour at the centre: Texture::value at (0.5, 0.5, centre) of the light's texture tree
        const rt::Color c = rt::texture_value<rt::F_ALL, false>(sv, fs.materials[mat].tex, rt::real(0.5), rt::real(0.5), centre,
                                                                 nullptr);
        const double m = std::max((double)c.x, std::max((double)c.y, (double)c.z));
        weight.push_back(std::isfinite(m) && m > 0.0 && std::isfinite((double)L.area) ? (double)L.area * m : 0.0);
        t.total_area += (double)L.area;
        t.slot_light[s] = (int32_t)t.lights.size();
        t.lights.push_back(L);
        sampled = true;
      }
    }
    if (!sampled && entry_emits(fs, e)) t.n_unsampled += 1;
  }
  double sum = 0.0;
  for (double w : weight) sum += w;
  if (!(sum > 0.0) || !std::isfinite(sum)) {
    for (double& w : weight) w = 1.0;
    sum = (double)weight.size();
  }
  double acc = 0.0, prev = 0.0;
  for (size_t k = 0; k < t.lights.size(); ++k) {
    acc += weight[k];
    const double cdf = k + 1 == t.lights.size() ? 1.0 : acc / sum;
    t.lights[k].cdf = (rt::real)cdf;
    t.lights[k].pmf = (rt::real)(cdf - prev);
    prev = cdf;
  }
  return t;
}

}  // namespace rtx
