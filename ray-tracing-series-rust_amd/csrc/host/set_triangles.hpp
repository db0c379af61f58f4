// rtx_flat_set_triangles, rtx_flat_set_spheres and the two rtx_flat_*_ids on the host, the shadow a scene keeps for the resident
// entries, and the ONE update path "new records for named static primitives" that all six entries share: argument check, id
// check, finiteness, plan, edit.  A kind (PrimKind: a triangle, a static sphere) is a constant; where the kinds differ in code
// and not in data, the shared function asks which one it has.  Pure host code of the f64 side: abi.cpp, render.hip's f64
// compilation and tests/set_{triangles,spheres}_host_check.cpp compile it.  The twin of host/set_transforms.hpp.
//
// An update gives named primitives new values -- a triangle v0 v1 v2, a static sphere cx cy cz radius (mat stays) -- and the
// result must be the flat scene flatten_scene builds from scratch with those values, byte for byte where a value reaches: the
// records (every flat copy of a triangle id), the boxes in `nodes`, `nodes32` and the static copy in `motion32` of every BVH
// that holds an updated primitive, `member_local_box` and the instance tree above a touched member, and `top_box32` of a plain
// slot of the kind.  Topology (child, axis, pad), refs, entries, sah_cost and every other array stay as they are; a fresh build
// may choose another topology, which is culling only.  A flat scene keeps no light table and no slot records: both are derived
// from these arrays when asked for (host/light_table.hpp) or at upload (hip/trace_world.inc).
//
// rtx_flat_set_moving_spheres (KIND_MOVING_SPHERE: c0 xyz, c1 xyz, radius; time0, time1, mat stay) runs the same path; what
// differs is the refit: a BVH that holds a mover keeps the unions over its own interval in `nodes` and, where the flattener gives
// it time-aware boxes, planes and slopes in `motion32` derived from the unions at the interval's two ends (refit_timed_bvh,
// core/mover_box.hpp).  Only a BVH that also holds a GravitySphere is refused there.
//
// rtx_flat_set_rects (KIND_RECT: a0 a1 b0 b1 k; axis and mat stay) runs the static path as a triangle does: a rectangle's id is
// its index in FlatScene::rects, a plain rectangle slot gets top_box32 like a triangle slot, and rtx_flat_rect_ids lists what
// the flattener emitted from a handle (FlatScene::handle_rect_first / _id: a RectPrism is six rectangles per emission).
//
// A triangle's id is the ordinal of its first emission (FlatScene::triangle_id: a BVH stores copies in leaf order).  A sphere's
// id is its index in FlatScene::spheres: the flattener emits a static sphere once per handle and neither moves nor copies it.
// No index is ever derived from a value: every index an update uses comes from the caller's ids (checked against the shadow)
// or from the shadow, which build_mesh_shadow validates against the array sizes.  A value only ever becomes a coordinate, a
// radius, a normal or a box plane.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "../core/mover_box.hpp"
#include "../core/prim_box.hpp"
#include "set_transforms.hpp"

namespace rtx {

struct BvhShadow {
  int32_t entry, root;          // the ENTRY_BVH record; its root: a node, or a leaf code when the BVH has no node
  int32_t first_ref, n_refs;
  int32_t node_base, n_nodes;   // its nodes are nodes[node_base .. node_base + n_nodes): a builder appends a tree in one piece
  int32_t node_first;           // index of its first node in the per-node tables (MeshShadow::node_parent, the arrival counters)
  int32_t leaf_first, n_leaves; // its leaves in MeshShadow::leaves
  int32_t timed;                // holds a MovingSphere or GravitySphere: its boxes depend on a time interval, no refit by
                                // rtx_*_set_triangles / _set_spheres
  // rtx_*_set_moving_spheres: it holds a MovingSphere; it holds a GravitySphere (refused: that centre is not linear in time);
  // it gets time-aware boxes -- the flattener's condition (flatten.cpp: build_motion_boxes): a root that is a node, time0 < time1,
  // a mover, no gravity sphere
  int32_t has_mover, has_gravity, time_boxes;
  double t0, t1;                // its own interval (FlatEntry::f)
};
struct MemberGeom {
  int32_t slot, geom, tree;     // a member of an instance tree: its slot, its PRIM / GROUP / BVH entry, its tree
};
struct MeshShadow {
  int32_t n_ids = 0;
  std::vector<int32_t> id_first, id_flat;        // id -> its flat triangles: id_flat[id_first[id] .. id_first[id + 1])
  std::vector<int32_t> tri_first, tri_entry;     // flat triangle -> the PRIM / GROUP / BVH entries that refer to it
  std::vector<BvhShadow> bvhs;
  std::vector<int32_t> bvh_of_entry;             // per entry: index in bvhs, -1
  std::vector<int32_t> leaves;                   // 3 per leaf: leaf code, the node that holds its box, which child
  std::vector<int32_t> node_parent;              // 2 per BVH node: parent (absolute node index, -1 for a root), which child
  std::vector<MemberGeom> members;               // in the order of member_local_box
  // a static sphere's id is its flat index, so there is no id table
  std::vector<int32_t> sph_first, sph_entry;     // flat sphere -> the PRIM / GROUP / BVH entries that refer to it
  // 4 per top-level slot whose f32 box comes from ONE triangle, static sphere or rectangle: the slot; the primitive's PRIM entry; 0 a plain
  // slot (top_box32 and the slot record's box), 1 the boundary sphere of a medium without a chain (the slot record's box); for
  // a plain sphere slot whose next slot is such a medium, that medium's PRIM entry (the slot record says whether both hold the
  // same sphere), else -1.  A plain triangle or rectangle slot is (slot, entry, 0, -1).
  std::vector<int32_t> slot_box;
  // a moving sphere's id is its flat index too (the flattener emits a mover once per handle)
  std::vector<int32_t> mov_first, mov_entry;     // flat moving sphere -> the PRIM / GROUP / BVH entries that refer to it
  std::vector<int32_t> mover_slot;               // 2 per plain top-level slot whose record is one mover: the slot, its PRIM entry
  // a rectangle's id is its flat index as well (a rectangle is neither copied nor permuted); a plain rectangle slot sits in
  // slot_box as (slot, entry, 0, -1), like a triangle's
  std::vector<int32_t> rect_first, rect_entry;   // flat rectangle -> the PRIM / GROUP / BVH entries that refer to it
  std::string broken;                            // not empty: the arrays are not what the flattener emits; the message says how
};

// A kind of primitive an update can name.  Data only; code that differs asks `type`.
struct PrimKind {
  uint32_t type;             // rt::PRIM_TRIANGLE / rt::PRIM_SPHERE / rt::PRIM_MOVING_SPHERE
  int width;                 // doubles per record of the caller's values
  const char* noun;          // in messages
  const char* count_phrase;  // "the scene has N ..."
  const char *arg, *d_arg;   // the values' argument name in the host and in the device entry
};
constexpr PrimKind KIND_TRIANGLE = {rt::PRIM_TRIANGLE, 9, "triangle", "triangle ids", "vertices", "d_vertices"};
constexpr PrimKind KIND_SPHERE = {rt::PRIM_SPHERE, 4, "sphere", "static spheres", "spheres", "d_spheres"};
constexpr PrimKind KIND_MOVING_SPHERE = {rt::PRIM_MOVING_SPHERE, 7, "moving sphere", "moving spheres", "movers", "d_movers"};
constexpr PrimKind KIND_RECT = {rt::PRIM_RECT, 5, "rectangle", "rectangles", "rects", "d_rects"};

// One update, resolved against the shadow: what to write and what to refit.
struct UpdatePlan {
  std::vector<int32_t> pairs;    // 2 per flat record: its index in triangles / spheres, index of the caller's record of values
  std::vector<int32_t> bvhs;     // touched BVHs (indices in MeshShadow::bvhs), ascending
  std::vector<int32_t> members;  // touched members (indices in MeshShadow::members), ascending
  std::vector<int32_t> trees;    // instance trees that hold one, ascending
  std::vector<int32_t> slots;    // 2 per slot whose f32 box is derived again: the slot, 0 plain / 1 medium boundary / 2 a plain mover; ascending
};

inline MeshShadow build_mesh_shadow(const FlatScene& fs, const UpdateShadow& us) {
  MeshShadow sh;
  auto broken = [&](const char* what) { sh.broken = what; return sh; };
  const size_t n_tri = fs.triangles.size(), n_ent = fs.entries.size(), n_ref = fs.refs.size(), n_node = fs.nodes.size();
  if (!us.broken.empty()) return broken(us.broken.c_str());
  if (fs.triangle_id.size() != n_tri) return broken("triangle_id does not hold one id per flat triangle");
  // ---- id -> flat triangles
  int32_t n_ids = 0;
  for (int32_t id : fs.triangle_id) {
    if (id < 0 || (size_t)id >= n_tri) return broken("triangle_id holds an id outside [0, number of triangles)");
    n_ids = std::max(n_ids, id + 1);
  }
  sh.n_ids = n_ids;
  sh.id_first.assign((size_t)n_ids + 1, 0);
  for (int32_t id : fs.triangle_id) sh.id_first[(size_t)id + 1]++;
  for (int32_t i = 0; i < n_ids; ++i) {
    if (sh.id_first[(size_t)i + 1] == 0) return broken("triangle_id skips an id");
    sh.id_first[(size_t)i + 1] += sh.id_first[(size_t)i];
  }
  sh.id_flat.resize(n_tri);
  {
    std::vector<int32_t> at(sh.id_first.begin(), sh.id_first.end() - 1);
    for (size_t t = 0; t < n_tri; ++t) sh.id_flat[(size_t)at[(size_t)fs.triangle_id[t]]++] = (int32_t)t;
  }
  // ---- flat triangle -> entries, in two passes over the entries' reference runs
  auto run_of = [&](const rt::FlatEntry& e, int64_t* first, int64_t* count) {
    if (e.kind == rt::ENTRY_GROUP) { *first = e.a; *count = e.b; return true; }
    if (e.kind == rt::ENTRY_BVH) { *first = e.b; *count = e.c; return true; }
    return false;
  };
  // (the same two passes give flat sphere -> entries)
  const size_t n_sph = fs.spheres.size(), n_mov = fs.moving_spheres.size(), n_rect = fs.rects.size();
  sh.tri_first.assign(n_tri + 1, 0);
  sh.sph_first.assign(n_sph + 1, 0);
  sh.mov_first.assign(n_mov + 1, 0);
  sh.rect_first.assign(n_rect + 1, 0);
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<int32_t> at, sph_at, mov_at, rect_at;
    if (pass == 1) {
      for (size_t t = 0; t < n_rect; ++t) sh.rect_first[t + 1] += sh.rect_first[t];
      sh.rect_entry.resize((size_t)sh.rect_first[n_rect]);
      rect_at.assign(sh.rect_first.begin(), sh.rect_first.end() - 1);
      for (size_t t = 0; t < n_tri; ++t) sh.tri_first[t + 1] += sh.tri_first[t];
      sh.tri_entry.resize((size_t)sh.tri_first[n_tri]);
      at.assign(sh.tri_first.begin(), sh.tri_first.end() - 1);
      for (size_t t = 0; t < n_sph; ++t) sh.sph_first[t + 1] += sh.sph_first[t];
      sh.sph_entry.resize((size_t)sh.sph_first[n_sph]);
      sph_at.assign(sh.sph_first.begin(), sh.sph_first.end() - 1);
      for (size_t t = 0; t < n_mov; ++t) sh.mov_first[t + 1] += sh.mov_first[t];
      sh.mov_entry.resize((size_t)sh.mov_first[n_mov]);
      mov_at.assign(sh.mov_first.begin(), sh.mov_first.end() - 1);
    }
    for (size_t k = 0; k < n_ent; ++k) {
      const rt::FlatEntry& e = fs.entries[k];
      auto note = [&](rt::PrimRef r) {
        const uint32_t ty = rt::primref_type(r), t = rt::primref_index(r);
        if (ty == rt::PRIM_SPHERE) {
          if (t >= n_sph) return false;
          if (pass == 0) sh.sph_first[(size_t)t + 1]++;
          else sh.sph_entry[(size_t)sph_at[t]++] = (int32_t)k;
          return true;
        }
        if (ty == rt::PRIM_MOVING_SPHERE) {
          if (t >= n_mov) return false;
          if (pass == 0) sh.mov_first[(size_t)t + 1]++;
          else sh.mov_entry[(size_t)mov_at[t]++] = (int32_t)k;
          return true;
        }
        if (ty == rt::PRIM_RECT) {
          if (t >= n_rect) return false;
          if (pass == 0) sh.rect_first[(size_t)t + 1]++;
          else sh.rect_entry[(size_t)rect_at[t]++] = (int32_t)k;
          return true;
        }
        if (ty != rt::PRIM_TRIANGLE) return true;
        if (t >= n_tri) return false;
        if (pass == 0) sh.tri_first[(size_t)t + 1]++;
        else sh.tri_entry[(size_t)at[t]++] = (int32_t)k;
        return true;
      };
      int64_t first = 0, count = 0;
      if (e.kind == rt::ENTRY_PRIM) {
        if (!note((rt::PrimRef)e.a)) return broken("a primitive entry names a triangle outside the triangle array, or a sphere outside the sphere array");
      } else if (run_of(e, &first, &count)) {
        if (first < 0 || count < 0 || (uint64_t)(first + count) > n_ref) return broken("an entry's references lie outside the reference array");
        for (int64_t i = 0; i < count; ++i)
          if (!note(fs.refs[(size_t)(first + i)])) return broken("a reference names a triangle outside the triangle array, or a sphere outside the sphere array");
      }
    }
  }
  // every other primitive a refit reads a box of
  for (rt::PrimRef r : fs.refs) {
    const uint32_t ty = rt::primref_type(r), i = rt::primref_index(r);
    if ((ty == rt::PRIM_SPHERE && i >= fs.spheres.size()) || (ty == rt::PRIM_RECT && i >= fs.rects.size()))
      return broken("a reference names a sphere or a rectangle outside its array");
  }
  // ---- the BVHs: leaves and the way up
  sh.bvh_of_entry.assign(n_ent, -1);
  std::vector<char> node_seen(n_node, 0);
  for (size_t k = 0; k < n_ent; ++k) {
    const rt::FlatEntry& e = fs.entries[k];
    if (e.kind != rt::ENTRY_BVH) continue;
    BvhShadow b;
    b.entry = (int32_t)k; b.root = e.a; b.first_ref = e.b; b.n_refs = e.c;
    b.node_first = (int32_t)(sh.node_parent.size() / 2);
    b.leaf_first = (int32_t)(sh.leaves.size() / 3);
    b.node_base = 0; b.n_nodes = 0; b.timed = 0; b.has_mover = 0; b.has_gravity = 0;
    b.t0 = (double)e.f[0]; b.t1 = (double)e.f[1];
    for (int32_t i = 0; i < e.c; ++i) {
      const uint32_t ty = rt::primref_type(fs.refs[(size_t)e.b + (size_t)i]);
      if (ty == rt::PRIM_MOVING_SPHERE || ty == rt::PRIM_GRAVITY_SPHERE) b.timed = 1;
      if (ty == rt::PRIM_MOVING_SPHERE) b.has_mover = 1;
      if (ty == rt::PRIM_GRAVITY_SPHERE) b.has_gravity = 1;
    }
    b.time_boxes = (e.a >= 0 && b.t0 < b.t1 && b.has_mover && !b.has_gravity) ? 1 : 0;
    auto leaf_ok = [&](int32_t code) { return (int64_t)rt::leaf_first(code) + (int64_t)rt::leaf_count(code) <= (int64_t)e.c; };
    if (rt::node_child_is_leaf(e.a)) {
      if (!leaf_ok(e.a)) return broken("a BVH's leaf names references outside its run");
    } else {
      if ((size_t)e.a >= n_node) return broken("a BVH names a root outside the node array");
      int32_t lo = e.a, hi = e.a;
      std::vector<int32_t> piece{e.a};
      node_seen[(size_t)e.a] = 1;
      for (size_t q = 0; q < piece.size(); ++q)
        for (int c = 0; c < 2; ++c) {
          const int32_t code = fs.nodes[(size_t)piece[q]].child[c];
          if (rt::node_child_is_leaf(code)) continue;
          if ((size_t)code >= n_node) return broken("a BVH names a node outside the node array");
          if (node_seen[(size_t)code]) return broken("a BVH node has two parents");
          node_seen[(size_t)code] = 1;
          lo = std::min(lo, code); hi = std::max(hi, code);
          piece.push_back(code);
        }
      if ((size_t)(hi - lo + 1) != piece.size()) return broken("a BVH's nodes are not one piece of the node array");
      b.node_base = lo; b.n_nodes = (int32_t)piece.size();
      sh.node_parent.resize(2 * (size_t)(b.node_first + b.n_nodes), -1);
      for (int32_t n : piece)
        for (int c = 0; c < 2; ++c) {
          const int32_t code = fs.nodes[(size_t)n].child[c];
          if (rt::node_child_is_leaf(code)) {
            if (!leaf_ok(code)) return broken("a BVH's leaf names references outside its run");
            sh.leaves.push_back(code); sh.leaves.push_back(n); sh.leaves.push_back(c);
          } else {
            sh.node_parent[2 * (size_t)(b.node_first + code - lo)] = n;
            sh.node_parent[2 * (size_t)(b.node_first + code - lo) + 1] = c;
          }
        }
    }
    b.n_leaves = (int32_t)(sh.leaves.size() / 3) - b.leaf_first;
    sh.bvh_of_entry[k] = (int32_t)sh.bvhs.size();
    sh.bvhs.push_back(b);
  }
  // ---- members of instance trees
  auto geom_of_slot = [&](size_t slot) -> int32_t {
    int32_t x = fs.top_level[slot];
    if (x < 0 || (size_t)x >= n_ent) return -1;
    if (fs.entries[(size_t)x].kind == rt::ENTRY_XFORM) x = fs.entries[(size_t)x].a;
    if (x < 0 || (size_t)x >= n_ent) return -1;
    const int32_t kind = fs.entries[(size_t)x].kind;
    return kind == rt::ENTRY_PRIM || kind == rt::ENTRY_GROUP || kind == rt::ENTRY_BVH ? x : -1;
  };
  for (size_t t = 0; t < us.trees.size(); ++t)
    for (int32_t m = 0; m < us.trees[t].n_slots; ++m) {
      const size_t slot = (size_t)us.trees[t].first_slot + (size_t)m;
      if (slot >= fs.top_level.size()) return broken("an instance tree names a slot outside the world list");
      const int32_t g = geom_of_slot(slot);
      if (g < 0) return broken("a member of an instance tree is not a primitive, a group or a BVH under a chain");
      sh.members.push_back({(int32_t)slot, g, (int32_t)t});
    }
  if (fs.member_local_box.size() != 6 * sh.members.size()) return broken("member_local_box does not hold 6 doubles per member of an instance tree");
  if (fs.top_box32.size() != 6 * fs.top_level.size()) return broken("top_box32 does not hold 6 floats per slot");
  for (size_t k = 0; k < fs.top_level.size(); ++k) {
    const int32_t x = fs.top_level[k];
    if (x < 0 || (size_t)x >= n_ent) return broken("the world list names an entry outside the entry array");
  }
  // ---- slots whose f32 box comes from one triangle or static sphere (flatten.cpp: "boxes of the plain static primitives";
  // trace_world.inc: build_world_desc, the boundary sphere of a medium)
  auto prim_of = [&](int32_t x, uint32_t ty) { return fs.entries[(size_t)x].kind == rt::ENTRY_PRIM && rt::primref_type((rt::PrimRef)fs.entries[(size_t)x].a) == ty; };
  auto medium_sphere = [&](size_t k) -> int32_t {  // the PRIM entry of the boundary sphere of slot k, -1
    if (k >= fs.top_level.size()) return -1;
    const rt::FlatEntry& e = fs.entries[(size_t)fs.top_level[k]];
    if (e.kind != rt::ENTRY_MEDIUM || e.a < 0 || (size_t)e.a >= n_ent) return -1;
    return prim_of(e.a, rt::PRIM_SPHERE) ? e.a : -1;
  };
  for (size_t k = 0; k < fs.top_level.size(); ++k) {
    const int32_t x = fs.top_level[k], m = medium_sphere(k);
    if (prim_of(x, rt::PRIM_TRIANGLE) || prim_of(x, rt::PRIM_RECT)) sh.slot_box.insert(sh.slot_box.end(), {(int32_t)k, x, 0, -1});
    else if (prim_of(x, rt::PRIM_SPHERE)) sh.slot_box.insert(sh.slot_box.end(), {(int32_t)k, x, 0, medium_sphere(k + 1)});
    else if (m >= 0) sh.slot_box.insert(sh.slot_box.end(), {(int32_t)k, m, 1, -1});
    if (prim_of(x, rt::PRIM_MOVING_SPHERE)) sh.mover_slot.insert(sh.mover_slot.end(), {(int32_t)k, x});
  }
  if (!fs.motion32.empty() && fs.motion32.size() != n_node) return broken("motion32 does not hold one record per node");
  return sh;
}

// The checks every entry makes before it looks at the scene or at a value: all four pointers are compared with NULL and never
// read.
inline bool check_prim_args(const PrimKind& K, const char* who, const void* scene, const int32_t* ids, int64_t n, const void* values, std::string* err) {
  if (!scene) { *err = std::string(who) + ": the scene is NULL"; return false; }
  if (n < 0) { *err = std::string(who) + ": n < 0"; return false; }
  if (!ids) { *err = std::string(who) + ": ids is NULL"; return false; }
  if (!values) { *err = std::string(who) + ": " + K.arg + " is NULL"; return false; }
  return true;
}
// ids[0 .. n), n > 0, against the scene's shadow.
inline bool check_prim_ids(const PrimKind& K, const char* who, const MeshShadow& sh, const int32_t* ids, int64_t n, std::string* err) {
  if (!sh.broken.empty()) { *err = std::string(who) + ": " + sh.broken; return false; }
  const int64_t n_ids = K.type == rt::PRIM_TRIANGLE ? (int64_t)sh.n_ids
                        : K.type == rt::PRIM_SPHERE ? (int64_t)sh.sph_first.size() - 1
                        : K.type == rt::PRIM_RECT ? (int64_t)sh.rect_first.size() - 1 : (int64_t)sh.mov_first.size() - 1;
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= n_ids) {
      *err = std::string(who) + ": ids[" + std::to_string(i) + "] is out of range (the scene has " + std::to_string(n_ids) + " " + K.count_phrase + ")";
      return false;
    }
  std::vector<int32_t> sorted(ids, ids + n);
  std::sort(sorted.begin(), sorted.end());
  for (size_t i = 1; i < sorted.size(); ++i)
    if (sorted[i] == sorted[i - 1]) { *err = std::string(who) + ": ids names " + K.noun + " " + std::to_string(sorted[i]) + " twice"; return false; }
  return true;
}

// Host entries only.  A sphere's radius gets the rule rtx_sphere applies -- none -- beyond being finite: a negative one (the
// hollow glass ball) and zero are legal.
inline bool check_prims_finite(const PrimKind& K, const char* who, const double* values, int64_t n, std::string* err) {
  for (int64_t i = 0; i < K.width * n; ++i)
    if (!std::isfinite(values[i])) {
      *err = std::string(who) + ": " + K.arg + "[" + std::to_string(i / K.width) + "][" + std::to_string(i % K.width) + "] is not finite";
      return false;
    }
  return true;
}

// From the touched entries (one flag per entry) to the BVHs to refit, the members whose local box changes and the instance
// trees above them.  what: the kind's noun, for the message.  RTX_EUNSUPPORTED when a touched BVH holds a Moving- or GravitySphere;
// movers (an update OF MovingSpheres, which refits the time-aware boxes too): only when it holds a GravitySphere.
inline rtx_status plan_touched_entries(const char* who, const char* what, const MeshShadow& sh, const std::vector<char>& touched,
                                       std::vector<int32_t>* bvhs, std::vector<int32_t>* members, std::vector<int32_t>* trees, std::string* err,
                                       bool movers = false) {
  for (size_t b = 0; b < sh.bvhs.size(); ++b) {
    if (!touched[(size_t)sh.bvhs[b].entry]) continue;
    if (movers && sh.bvhs[b].has_gravity) {
      *err = std::string(who) + ": ids name a " + what + " of a BVH that also holds a GravitySphere (entry " + std::to_string(sh.bvhs[b].entry) +
             "): a GravitySphere's centre is not linear in time and its box needs its height table, which a refit does not read. Flatten the scene anew";
      return RTX_EUNSUPPORTED;
    }
    if (!movers && sh.bvhs[b].timed) {
      *err = std::string(who) + ": ids name a " + what + " of a BVH that holds a MovingSphere or GravitySphere (entry " + std::to_string(sh.bvhs[b].entry) +
             "): its time-aware boxes would have to be derived again. Flatten the scene anew";
      return RTX_EUNSUPPORTED;
    }
    bvhs->push_back((int32_t)b);
  }
  for (size_t m = 0; m < sh.members.size(); ++m) {
    if (!touched[(size_t)sh.members[m].geom]) continue;
    members->push_back((int32_t)m);
    if (trees->empty() || trees->back() != sh.members[m].tree) trees->push_back(sh.members[m].tree);
  }
  return RTX_OK;
}

// ids (checked) -> what to write and refit.  RTX_EUNSUPPORTED when a touched BVH holds a Moving- or GravitySphere.
inline rtx_status plan_prim_update(const PrimKind& K, const char* who, const MeshShadow& sh, const int32_t* ids, int64_t n, UpdatePlan* plan,
                                   std::string* err) {
  *plan = UpdatePlan();
  std::vector<char> touched(sh.bvh_of_entry.size(), 0);
  // The one loop of an update that runs per id on the caller's thread (871 200 ids in scripts/bench_set_triangles.py): each kind
  // keeps its own, on its own tables -- one loop that picks the tables per kind measured 2 % to 11 % slower a call.
  if (K.type == rt::PRIM_TRIANGLE) {  // an id names every flat copy of the triangle
    for (int64_t i = 0; i < n; ++i)
      for (int32_t k = sh.id_first[(size_t)ids[i]]; k < sh.id_first[(size_t)ids[i] + 1]; ++k) {
        const int32_t t = sh.id_flat[(size_t)k];
        plan->pairs.push_back(t);
        plan->pairs.push_back((int32_t)i);
        for (int32_t q = sh.tri_first[(size_t)t]; q < sh.tri_first[(size_t)t + 1]; ++q) touched[(size_t)sh.tri_entry[(size_t)q]] = 1;
      }
  } else if (K.type == rt::PRIM_SPHERE) {  // an id is the flat index of the sphere
    for (int64_t i = 0; i < n; ++i) {
      plan->pairs.push_back(ids[i]);
      plan->pairs.push_back((int32_t)i);
      for (int32_t q = sh.sph_first[(size_t)ids[i]]; q < sh.sph_first[(size_t)ids[i] + 1]; ++q) touched[(size_t)sh.sph_entry[(size_t)q]] = 1;
    }
  } else if (K.type == rt::PRIM_RECT) {  // ... of the rectangle
    for (int64_t i = 0; i < n; ++i) {
      plan->pairs.push_back(ids[i]);
      plan->pairs.push_back((int32_t)i);
      for (int32_t q = sh.rect_first[(size_t)ids[i]]; q < sh.rect_first[(size_t)ids[i] + 1]; ++q) touched[(size_t)sh.rect_entry[(size_t)q]] = 1;
    }
  } else {  // ... of the moving sphere
    for (int64_t i = 0; i < n; ++i) {
      plan->pairs.push_back(ids[i]);
      plan->pairs.push_back((int32_t)i);
      for (int32_t q = sh.mov_first[(size_t)ids[i]]; q < sh.mov_first[(size_t)ids[i] + 1]; ++q) touched[(size_t)sh.mov_entry[(size_t)q]] = 1;
    }
  }
  const bool movers = K.type == rt::PRIM_MOVING_SPHERE;
  const rtx_status st = plan_touched_entries(who, K.noun, sh, touched, &plan->bvhs, &plan->members, &plan->trees, err, movers);
  if (st != RTX_OK) return st;
  if (movers) {  // a plain mover in the world list: the slot record's box and WD_TIME_BOX (no top_box32, no medium, no pair rule)
    for (size_t k = 0; k < sh.mover_slot.size(); k += 2)
      if (touched[(size_t)sh.mover_slot[k + 1]]) { plan->slots.push_back(sh.mover_slot[k]); plan->slots.push_back(2); }
    return RTX_OK;
  }
  for (size_t k = 0; k < sh.slot_box.size(); k += 4) {
    const int32_t next = sh.slot_box[k + 3];  // a plain sphere slot before a medium: their "same sphere" flag hangs on either
    if (touched[(size_t)sh.slot_box[k + 1]] || (next >= 0 && touched[(size_t)next])) { plan->slots.push_back(sh.slot_box[k]); plan->slots.push_back(sh.slot_box[k + 2]); }
  }
  return RTX_OK;
}

// The box of a BVH leaf: the union of its primitives' boxes, in the builder's own arithmetic (bvh_build.cpp: Box::grow).
RT_HD void bvh_leaf_box(int32_t code, const rt::PrimRef* refs, const rt::FlatSphere* spheres, const rt::FlatRect* rects,
                        const rt::FlatTriangle* triangles, double* b) {
  const double inf = __builtin_huge_val();
  for (int a = 0; a < 3; ++a) { b[a] = inf; b[3 + a] = -inf; }
  const uint32_t first = rt::leaf_first(code), count = rt::leaf_count(code);
  for (uint32_t i = 0; i < count; ++i) {
    double pb[6];
    rt::static_prim_box(refs[first + i], spheres, rects, triangles, pb);
    for (int a = 0; a < 3; ++a) { b[a] = rt::rt_fmin(b[a], pb[a]); b[3 + a] = rt::rt_fmax(b[3 + a], pb[3 + a]); }
  }
}

// The box of a leaf of a BVH that holds MovingSpheres, over [ta, tb] (ta == tb: at that instant): a mover gives
// core/mover_box.hpp's box, a static member its static box whatever the times (flatten.cpp: prim_box).  No GravitySphere: its
// reference would get the empty box (plan_touched_entries refuses such a BVH first).
RT_HD void timed_leaf_box(int32_t code, const rt::PrimRef* refs, const rt::FlatSphere* spheres, const rt::FlatMovingSphere* movers,
                          const rt::FlatRect* rects, const rt::FlatTriangle* triangles, double ta, double tb, double* b) {
  const double inf = __builtin_huge_val();
  for (int a = 0; a < 3; ++a) { b[a] = inf; b[3 + a] = -inf; }
  const uint32_t first = rt::leaf_first(code), count = rt::leaf_count(code);
  for (uint32_t i = 0; i < count; ++i) {
    double pb[6];
    const rt::PrimRef ref = refs[first + i];
    if (rt::primref_type(ref) == rt::PRIM_MOVING_SPHERE) rt::moving_sphere_box(movers[rt::primref_index(ref)], ta, tb, pb);
    else rt::static_prim_box(ref, spheres, rects, triangles, pb);
    for (int a = 0; a < 3; ++a) { b[a] = rt::rt_fmin(b[a], pb[a]); b[3 + a] = rt::rt_fmax(b[3 + a], pb[3 + a]); }
  }
}

// The box of a member of an instance tree BEFORE its ops (FlatScene::member_local_box).  flatten.cpp (member_world_box) takes
// the ordered union of ALL the member's primitive boxes.  For a primitive or a group this does the same; for a BVH with nodes
// it unites the root's two child boxes instead, which a refit has just made the exact unions of those same primitive boxes:
// min and max are exact and associative, and a static box is ordered (|radius|, min / max of the vertices, a rectangle given low edge first), so the two give
// the same planes -- the sign of a plane that is exactly zero aside, which follows the order of the unions.
RT_HD void member_local_box_of(const rt::FlatEntry& G, const rt::FlatNode* nodes, const rt::PrimRef* refs, const rt::FlatSphere* spheres,
                               const rt::FlatRect* rects, const rt::FlatTriangle* triangles, double* b) {
  const double inf = __builtin_huge_val();
  for (int a = 0; a < 3; ++a) { b[a] = inf; b[3 + a] = -inf; }
  if (G.kind == rt::ENTRY_BVH && !rt::node_child_is_leaf(G.a)) {
    const rt::FlatNode& nd = nodes[G.a];
    for (int c = 0; c < 2; ++c) {
      double pb[6];
      for (int a = 0; a < 3; ++a) { pb[a] = (double)nd.bmin[c][a]; pb[3 + a] = (double)nd.bmax[c][a]; }
      rt::grow_ordered(b, pb);
    }
    return;
  }
  double pb[6];
  if (G.kind == rt::ENTRY_PRIM) {
    rt::static_prim_box((rt::PrimRef)G.a, spheres, rects, triangles, pb);
    rt::grow_ordered(b, pb);
    return;
  }
  const int32_t first = G.kind == rt::ENTRY_GROUP ? G.a : G.b, count = G.kind == rt::ENTRY_GROUP ? G.b : G.c;
  for (int32_t i = 0; i < count; ++i) {
    rt::static_prim_box(refs[first + i], spheres, rects, triangles, pb);
    rt::grow_ordered(b, pb);
  }
}

// BVH b of fs refitted whole, bottom-up: nodes, nodes32 and, where the scene has one, motion32's static copy.
inline void refit_bvh(FlatScene* fs, const BvhShadow& b) {
  if (rt::node_child_is_leaf(b.root)) return;  // no node: only its triangles changed
  const rt::PrimRef* refs = fs->refs.data() + b.first_ref;
  refit_tree_piece(fs, b.root, b.node_base, b.n_nodes, [&](int32_t code, double* box) {
    bvh_leaf_box(code, refs, fs->spheres.data(), fs->rects.data(), fs->triangles.data(), box);
  });
}

// BVH b of fs, which holds MovingSpheres, refitted whole and bottom-up after their values changed.  nodes and nodes32 get the
// unions over the BVH's own interval [t0, t1], as refit_bvh gives a static BVH its boxes; motion32 gets the static copy without
// slopes where b gets no time-aware boxes, else -- a second climb, carrying the unions AT t0 and AT t1 -- the planes
// core/mover_box.hpp makes of a child's two end boxes.  flatten.cpp derives the same top-down (motion_box_at): unions are exact
// min / max, so the order does not show.
inline void refit_timed_bvh(FlatScene* fs, const BvhShadow& b) {
  if (rt::node_child_is_leaf(b.root)) return;  // no node: only its records changed
  const rt::PrimRef* refs = fs->refs.data() + b.first_ref;
  auto leaf_at = [&](int32_t code, double ta, double tb, double* box) {
    timed_leaf_box(code, refs, fs->spheres.data(), fs->moving_spheres.data(), fs->rects.data(), fs->triangles.data(), ta, tb, box);
  };
  refit_tree_piece(fs, b.root, b.node_base, b.n_nodes, [&](int32_t code, double* box) { leaf_at(code, b.t0, b.t1, box); });
  if (!b.time_boxes || fs->motion32.empty()) return;
  struct Ends { double b[2][6]; };
  std::vector<int32_t> order{b.root};  // children before parents: breadth-first from the root, walked backwards
  for (size_t k = 0; k < order.size(); ++k)
    for (int c = 0; c < 2; ++c)
      if (!rt::node_child_is_leaf(fs->nodes[(size_t)order[k]].child[c])) order.push_back(fs->nodes[(size_t)order[k]].child[c]);
  std::vector<Ends> whole((size_t)b.n_nodes);  // the two end unions of a node's whole subtree, by node - node_base
  for (size_t k = order.size(); k-- > 0;) {
    const int32_t n = order[k];
    const rt::FlatNode& nd = fs->nodes[(size_t)n];
    rt::FlatMotion32& m = fs->motion32[(size_t)n];
    Ends u;
    for (int c = 0; c < 2; ++c) {
      Ends cb;
      if (rt::node_child_is_leaf(nd.child[c])) { leaf_at(nd.child[c], b.t0, b.t0, cb.b[0]); leaf_at(nd.child[c], b.t1, b.t1, cb.b[1]); }
      else cb = whole[(size_t)(nd.child[c] - b.node_base)];
      (void)rt::motion_child_planes(cb.b[0], cb.b[1], m.lo0[c], m.dlo[c], m.hi0[c], m.dhi[c]);
      if (c == 0) u = cb;
      else
        for (int e = 0; e < 2; ++e)
          for (int a = 0; a < 3; ++a) { u.b[e][a] = rt::rt_fmin(u.b[e][a], cb.b[e][a]); u.b[e][3 + a] = rt::rt_fmax(u.b[e][3 + a], cb.b[e][3 + a]); }
    }
    whole[(size_t)(n - b.node_base)] = u;
  }
}

// rtx_flat_set_triangles / rtx_flat_set_spheres / rtx_flat_set_moving_spheres: every check first, then the edit.  Not RTX_OK: *err
// set and *fs untouched.
inline rtx_status flat_set_prims(const PrimKind& K, const char* who, FlatScene* fs, const int32_t* ids, int64_t n, const double* values, std::string* err) {
  if (!check_prim_args(K, who, fs, ids, n, values, err)) return RTX_EINVAL;
  if (n == 0) return RTX_OK;
  const UpdateShadow us = build_update_shadow(*fs);
  const MeshShadow sh = build_mesh_shadow(*fs, us);
  if (!check_prim_ids(K, who, sh, ids, n, err)) return RTX_EINVAL;
  if (!check_prims_finite(K, who, values, n, err)) return RTX_EINVAL;
  UpdatePlan plan;
  const rtx_status st = plan_prim_update(K, who, sh, ids, n, &plan, err);
  if (st != RTX_OK) return st;
  for (size_t k = 0; k < plan.pairs.size(); k += 2) {
    const double* v = values + (size_t)K.width * (size_t)plan.pairs[k + 1];
    if (K.type == rt::PRIM_TRIANGLE) rt::set_triangle_vertices(&fs->triangles[(size_t)plan.pairs[k]], v);
    else if (K.type == rt::PRIM_SPHERE) rt::set_sphere_values(&fs->spheres[(size_t)plan.pairs[k]], v);
    else if (K.type == rt::PRIM_RECT) rt::set_rect_values(&fs->rects[(size_t)plan.pairs[k]], v);
    else rt::set_moving_sphere_values(&fs->moving_spheres[(size_t)plan.pairs[k]], v);
  }
  for (int32_t b : plan.bvhs) {
    if (K.type == rt::PRIM_MOVING_SPHERE) refit_timed_bvh(fs, sh.bvhs[(size_t)b]);
    else refit_bvh(fs, sh.bvhs[(size_t)b]);
  }
  for (int32_t m : plan.members)
    member_local_box_of(fs->entries[(size_t)sh.members[(size_t)m].geom], fs->nodes.data(), fs->refs.data(), fs->spheres.data(), fs->rects.data(),
                        fs->triangles.data(), &fs->member_local_box[6 * (size_t)m]);
  for (int32_t t : plan.trees) refit_instance_tree(fs, us.trees[(size_t)t]);
  for (size_t k = 0; k < plan.slots.size(); k += 2)
    if (plan.slots[k + 1] == 0)  // (a medium or a plain mover slot has no top_box32: its box lives in the slot record an upload derives)
      rt::plain_slot_box32((rt::PrimRef)fs->entries[(size_t)fs->top_level[(size_t)plan.slots[k]]].a, fs->spheres.data(), fs->rects.data(),
                           fs->triangles.data(), &fs->top_box32[6 * (size_t)plan.slots[k]]);
  return RTX_OK;
}
inline rtx_status flat_set_triangles(const char* who, FlatScene* fs, const int32_t* ids, int64_t n, const double* vertices, std::string* err) {
  return flat_set_prims(KIND_TRIANGLE, who, fs, ids, n, vertices, err);
}
inline rtx_status flat_set_spheres(const char* who, FlatScene* fs, const int32_t* ids, int64_t n, const double* spheres, std::string* err) {
  return flat_set_prims(KIND_SPHERE, who, fs, ids, n, spheres, err);
}
// movers: n x 7 doubles, c0 xyz, c1 xyz, radius; time0, time1 and mat stay.
inline rtx_status flat_set_moving_spheres(const char* who, FlatScene* fs, const int32_t* ids, int64_t n, const double* movers, std::string* err) {
  return flat_set_prims(KIND_MOVING_SPHERE, who, fs, ids, n, movers, err);
}
// rects: n x 5 doubles a0 a1 b0 b1 k; axis and mat stay.
inline rtx_status flat_set_rects(const char* who, FlatScene* fs, const int32_t* ids, int64_t n, const double* rects, std::string* err) {
  return flat_set_prims(KIND_RECT, who, fs, ids, n, rects, err);
}

// rtx_flat_triangle_ids / rtx_flat_sphere_ids / rtx_flat_moving_sphere_ids (`who`): the ids of the primitives of the kind below
// `object`, in list order.  -1 with *err set.  (A primitive of another kind has no children and no id of this kind: skipped.  The
// flattener emits a handle once -- prim_of in flatten.cpp -- so a handle has one record and is returned once per place it is listed.)
inline int64_t flat_prim_ids(const PrimKind& K, const char* who, const FlatScene& fs, const SceneGraph& g, int32_t object, int32_t* ids, int64_t cap,
                             std::string* err) {
  const std::vector<int32_t>& handle_id = K.type == rt::PRIM_TRIANGLE ? fs.handle_triangle_id
                                          : K.type == rt::PRIM_SPHERE ? fs.handle_sphere_id : fs.handle_moving_sphere_id;
  const int32_t h_kind = K.type == rt::PRIM_TRIANGLE ? H_TRIANGLE : K.type == rt::PRIM_SPHERE ? H_SPHERE : H_MOVING_SPHERE;
  if (!g.valid_hittable(object)) { *err = std::string(who) + ": bad object handle"; return -1; }
  int64_t count = 0;
  std::vector<std::pair<int32_t, int>> todo{{object, 0}};  // depth-first, children in list order
  while (!todo.empty()) {
    const std::pair<int32_t, int> at = todo.back();
    todo.pop_back();
    if (at.second > 80) { *err = std::string(who) + ": objects nested deeper than 80"; return -1; }
    if ((size_t)at.first >= handle_id.size()) { *err = std::string(who) + ": the object was made after this flat scene was flattened"; return -1; }
    const GHittable& o = g.hittables[(size_t)at.first];
    if (o.kind == h_kind) {
      const int32_t id = handle_id[(size_t)at.first];
      if (id < 0) { *err = std::string(who) + ": this flat scene did not flatten the object (a " + K.noun + " below it has no id)"; return -1; }
      if (ids && count < cap) ids[count] = id;
      ++count;
      continue;
    }
    for (size_t c = o.children.size(); c-- > 0;) todo.push_back({o.children[c], at.second + 1});
  }
  return count;
}

// rtx_flat_rect_ids: the ids of every rectangle the flattener emitted from the handles below `object`, handle by handle in list
// order, a handle's rectangles in emission order (FlatScene::handle_rect_first / _id).  A rectangle handle owns one id however
// often it is listed; a RectPrism owns six per emission, in the order of emit_prism, and is emitted once per place it is reached
// from -- so a prism under two Translates gives twelve, from the world and from the prism's own handle alike.  Every id is
// returned once, with the first reach of its handle: what rtx_*_set_rects takes (it refuses an id named twice).  -1 with *err set.
inline int64_t flat_rect_ids(const char* who, const FlatScene& fs, const SceneGraph& g, int32_t object, int32_t* ids, int64_t cap, std::string* err) {
  if (!g.valid_hittable(object)) { *err = std::string(who) + ": bad object handle"; return -1; }
  int64_t count = 0;
  std::vector<char> seen(g.hittables.size(), 0);
  std::vector<std::pair<int32_t, int>> todo{{object, 0}};  // depth-first, children in list order
  while (!todo.empty()) {
    const std::pair<int32_t, int> at = todo.back();
    todo.pop_back();
    if (at.second > 80) { *err = std::string(who) + ": objects nested deeper than 80"; return -1; }
    if ((size_t)at.first + 1 >= fs.handle_rect_first.size()) { *err = std::string(who) + ": the object was made after this flat scene was flattened"; return -1; }
    const GHittable& o = g.hittables[(size_t)at.first];
    if (o.kind == H_XY_RECT || o.kind == H_XZ_RECT || o.kind == H_YZ_RECT || o.kind == H_RECT_PRISM) {
      const int32_t first = fs.handle_rect_first[(size_t)at.first], end = fs.handle_rect_first[(size_t)at.first + 1];
      if (first == end) { *err = std::string(who) + ": this flat scene did not flatten the object (a rectangle below it has no id)"; return -1; }
      if (seen[(size_t)at.first]) continue;
      seen[(size_t)at.first] = 1;
      for (int32_t k = first; k < end; ++k) {
        if (ids && count < cap) ids[count] = fs.handle_rect_id[(size_t)k];
        ++count;
      }
      continue;
    }
    for (size_t c = o.children.size(); c-- > 0;) todo.push_back({o.children[c], at.second + 1});
  }
  return count;
}

}  // namespace rtx
