// rtx_flat_set_spheres and rtx_flat_sphere_ids on the host, and the checks and the plan of an update that the flat entry and
// the two resident entries share.  Pure host code of the f64 side: abi.cpp, render.hip's f64 compilation and
// tests/set_spheres_host_check.cpp compile it.  The twin of host/set_triangles.hpp, whose shadow (MeshShadow) it extends: the
// BVH, member and leaf tables are the same; a static sphere adds sphere -> entries and the slots whose f32 box comes from one
// sphere.
//
// An update gives named static spheres a new centre and radius; the result must be the flat scene flatten_scene builds from
// scratch with those spheres, byte for byte where a value reaches: the sphere records (mat stays), the boxes in `nodes`,
// `nodes32` and the static copy in `motion32` of every BVH that holds an updated sphere, `member_local_box` and the instance
// tree above a touched member, and `top_box32` of a plain sphere slot.  A flat scene keeps no light table and no slot records:
// both are derived from these arrays when asked for (host/light_table.hpp) or at upload (hip/trace_world.inc).
//
// A sphere's id is its index in FlatScene::spheres: the flattener emits a static sphere once per handle and neither moves nor
// copies it, so one id names one record, however many entries refer to it.  No index is ever derived from a value: every
// index an update uses comes from the caller's ids (checked against the array size) or from the shadow.
#pragma once
#include "set_triangles.hpp"

namespace rtx {

// One update, resolved against the shadow: what to write and what to refit.
struct SpherePlan {
  std::vector<int32_t> pairs;    // 2 per id: flat sphere index, index of the caller's value quadruple
  std::vector<int32_t> bvhs;     // touched BVHs (indices in MeshShadow::bvhs), ascending
  std::vector<int32_t> members;  // touched members (indices in MeshShadow::members), ascending
  std::vector<int32_t> trees;    // instance trees that hold one, ascending
  std::vector<int32_t> slots;    // 2 per slot whose f32 box is derived again: the slot, 0 plain / 1 medium boundary; ascending
};

// The checks every entry makes before it looks at the scene or at a value: all four pointers are compared with NULL and never
// read.
inline bool check_sphere_args(const char* who, const void* scene, const int32_t* ids, int64_t n, const void* spheres, std::string* err) {
  if (!scene) { *err = std::string(who) + ": the scene is NULL"; return false; }
  if (n < 0) { *err = std::string(who) + ": n < 0"; return false; }
  if (!ids) { *err = std::string(who) + ": ids is NULL"; return false; }
  if (!spheres) { *err = std::string(who) + ": spheres is NULL"; return false; }
  return true;
}
// ids[0 .. n), n > 0, against the scene's shadow.
inline bool check_sphere_ids(const char* who, const MeshShadow* sh, const int32_t* ids, int64_t n, std::string* err) {
  if (!sh->broken.empty()) { *err = std::string(who) + ": " + sh->broken; return false; }
  const int64_t n_ids = (int64_t)sh->sph_first.size() - 1;
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= n_ids) {
      *err = std::string(who) + ": ids[" + std::to_string(i) + "] is out of range (the scene has " + std::to_string(n_ids) + " static spheres)";
      return false;
    }
  std::vector<int32_t> sorted(ids, ids + n);
  std::sort(sorted.begin(), sorted.end());
  for (size_t i = 1; i < sorted.size(); ++i)
    if (sorted[i] == sorted[i - 1]) { *err = std::string(who) + ": ids names sphere " + std::to_string(sorted[i]) + " twice"; return false; }
  return true;
}

// Host entries only.  The radius gets the rule rtx_sphere applies -- none -- beyond being finite: a negative one (the hollow
// glass ball) and zero are legal.
inline bool check_spheres_finite(const char* who, const double* spheres, int64_t n, std::string* err) {
  for (int64_t i = 0; i < 4 * n; ++i)
    if (!std::isfinite(spheres[i])) {
      *err = std::string(who) + ": spheres[" + std::to_string(i / 4) + "][" + std::to_string(i % 4) + "] is not finite";
      return false;
    }
  return true;
}

// ids (checked) -> what to write and refit.  RTX_EUNSUPPORTED when a touched BVH holds a Moving- or GravitySphere.
inline rtx_status plan_sphere_update(const char* who, const MeshShadow& sh, const int32_t* ids, int64_t n, SpherePlan* plan, std::string* err) {
  *plan = SpherePlan();
  std::vector<char> touched(sh.bvh_of_entry.size(), 0);
  for (int64_t i = 0; i < n; ++i) {
    plan->pairs.push_back(ids[i]);
    plan->pairs.push_back((int32_t)i);
    for (int32_t q = sh.sph_first[(size_t)ids[i]]; q < sh.sph_first[(size_t)ids[i] + 1]; ++q) touched[(size_t)sh.sph_entry[(size_t)q]] = 1;
  }
  const rtx_status st = plan_touched_entries(who, "sphere", sh, touched, &plan->bvhs, &plan->members, &plan->trees, err);
  if (st != RTX_OK) return st;
  for (size_t k = 0; k < sh.sphere_slot.size(); k += 4) {
    const int32_t next = sh.sphere_slot[k + 3];  // a plain slot before a medium: their "same sphere" flag hangs on either
    if (touched[(size_t)sh.sphere_slot[k + 1]] || (next >= 0 && touched[(size_t)next])) { plan->slots.push_back(sh.sphere_slot[k]); plan->slots.push_back(sh.sphere_slot[k + 2]); }
  }
  return RTX_OK;
}

// rtx_flat_set_spheres: every check first, then the edit.  Not RTX_OK: *err set and *fs untouched.
inline rtx_status flat_set_spheres(const char* who, FlatScene* fs, const int32_t* ids, int64_t n, const double* spheres, std::string* err) {
  if (!check_sphere_args(who, fs, ids, n, spheres, err)) return RTX_EINVAL;
  if (n == 0) return RTX_OK;
  const UpdateShadow us = build_update_shadow(*fs);
  const MeshShadow sh = build_mesh_shadow(*fs, us);
  if (!check_sphere_ids(who, &sh, ids, n, err)) return RTX_EINVAL;
  if (!check_spheres_finite(who, spheres, n, err)) return RTX_EINVAL;
  SpherePlan plan;
  const rtx_status st = plan_sphere_update(who, sh, ids, n, &plan, err);
  if (st != RTX_OK) return st;
  for (size_t k = 0; k < plan.pairs.size(); k += 2) rt::set_sphere_values(&fs->spheres[(size_t)plan.pairs[k]], spheres + 4 * (size_t)plan.pairs[k + 1]);
  for (int32_t b : plan.bvhs) refit_bvh(fs, sh.bvhs[(size_t)b]);
  for (int32_t m : plan.members)
    member_local_box_of(fs->entries[(size_t)sh.members[(size_t)m].geom], fs->nodes.data(), fs->refs.data(), fs->spheres.data(), fs->rects.data(),
                        fs->triangles.data(), &fs->member_local_box[6 * (size_t)m]);
  for (int32_t t : plan.trees) refit_instance_tree(fs, us.trees[(size_t)t]);
  for (size_t k = 0; k < plan.slots.size(); k += 2)
    if (plan.slots[k + 1] == 0)  // (a medium slot has no top_box32: its box lives in the slot record an upload derives)
      rt::plain_slot_box32((rt::PrimRef)fs->entries[(size_t)fs->top_level[(size_t)plan.slots[k]]].a, fs->spheres.data(), fs->rects.data(),
                           fs->triangles.data(), &fs->top_box32[6 * (size_t)plan.slots[k]]);
  return RTX_OK;
}

// rtx_flat_sphere_ids: the ids of the static spheres below `object`, in list order.  -1 with *err set.
inline int64_t flat_sphere_ids(const FlatScene& fs, const SceneGraph& g, int32_t object, int32_t* ids, int64_t cap, std::string* err) {
  if (!g.valid_hittable(object)) { *err = "rtx_flat_sphere_ids: bad object handle"; return -1; }
  int64_t count = 0;
  std::vector<std::pair<int32_t, int>> todo{{object, 0}};  // depth-first, children in list order
  while (!todo.empty()) {
    const std::pair<int32_t, int> at = todo.back();
    todo.pop_back();
    if (at.second > 80) { *err = "rtx_flat_sphere_ids: objects nested deeper than 80"; return -1; }
    if ((size_t)at.first >= fs.handle_sphere_id.size()) { *err = "rtx_flat_sphere_ids: the object was made after this flat scene was flattened"; return -1; }
    const GHittable& o = g.hittables[(size_t)at.first];
    if (o.kind == H_SPHERE) {
      const int32_t id = fs.handle_sphere_id[(size_t)at.first];
      if (id < 0) { *err = "rtx_flat_sphere_ids: this flat scene did not flatten the object (a sphere below it has no id)"; return -1; }
      if (ids && count < cap) ids[count] = id;
      ++count;
      continue;
    }
    // (a MovingSphere or GravitySphere has no children and no id: skipped)
    for (size_t c = o.children.size(); c-- > 0;) todo.push_back({o.children[c], at.second + 1});
  }
  return count;
}

}  // namespace rtx
