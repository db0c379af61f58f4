// rtx_flat_set_triangles on the host, the shadow a scene keeps for rtx_scene_set_triangles, and the checks and the plan of an
// update that all three entries share.  Pure host code of the f64 side: abi.cpp, render.hip's f64 compilation and
// tests/set_triangles_host_check.cpp compile it.  The twin of host/set_transforms.hpp.
//
// An update gives named triangles new vertices; the result must be the flat scene flatten_scene builds from scratch with those
// vertices, byte for byte where a vertex reaches: the triangle records (every flat copy of an id), the boxes in `nodes`,
// `nodes32` and the static copy in `motion32` of every BVH that holds an updated triangle, `member_local_box` and the
// instance tree above a touched member, and `top_box32` of a plain triangle slot.  Topology (child, axis, pad), refs, entries,
// sah_cost and every other array stay as they are; a fresh build may choose another topology, which is culling only.
//
// No index is ever derived from a vertex: every index an update uses comes from the caller's ids (checked against the id
// table) or from the shadow, which build_mesh_shadow validates against the array sizes.  A vertex only ever becomes a
// coordinate, a normal or a box plane.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "../core/prim_box.hpp"
#include "set_transforms.hpp"

namespace rtx {

struct BvhShadow {
  int32_t entry, root;          // the ENTRY_BVH record; its root: a node, or a leaf code when the BVH has no node
  int32_t first_ref, n_refs;
  int32_t node_base, n_nodes;   // its nodes are nodes[node_base .. node_base + n_nodes): a builder appends a tree in one piece
  int32_t node_first;           // index of its first node in the per-node tables (MeshShadow::node_parent, the arrival counters)
  int32_t leaf_first, n_leaves; // its leaves in MeshShadow::leaves
  int32_t timed;                // holds a MovingSphere or GravitySphere: its boxes depend on a time interval, no refit
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
  std::vector<int32_t> prim_slot;                // 2 per plain top-level slot whose entry is one triangle: the slot, the entry
  // rtx_*_set_spheres (host/set_spheres.hpp): a static sphere's id is its flat index, so there is no id table
  std::vector<int32_t> sph_first, sph_entry;     // flat sphere -> the PRIM / GROUP / BVH entries that refer to it
  // 4 per top-level slot whose f32 box comes from ONE static sphere: the slot; the sphere's PRIM entry; 0 a plain slot
  // (top_box32 and the slot record's box), 1 the boundary of a medium without a chain (the slot record's box); for a plain slot
  // whose next slot is such a medium, that medium's PRIM entry (the slot record says whether both hold the same sphere), else -1
  std::vector<int32_t> sphere_slot;
  std::string broken;                            // not empty: the arrays are not what the flattener emits; the message says how
};

// One update, resolved against the shadow: what to write and what to refit.
struct TrianglePlan {
  std::vector<int32_t> pairs;    // 2 per flat copy: flat triangle index, index of the caller's vertex triple
  std::vector<int32_t> bvhs;     // touched BVHs (indices in MeshShadow::bvhs), ascending
  std::vector<int32_t> members;  // touched members (indices in MeshShadow::members), ascending
  std::vector<int32_t> trees;    // instance trees that hold one, ascending
  std::vector<int32_t> slots;    // touched plain triangle slots, ascending
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
  const size_t n_sph = fs.spheres.size();
  sh.tri_first.assign(n_tri + 1, 0);
  sh.sph_first.assign(n_sph + 1, 0);
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<int32_t> at, sph_at;
    if (pass == 1) {
      for (size_t t = 0; t < n_tri; ++t) sh.tri_first[t + 1] += sh.tri_first[t];
      sh.tri_entry.resize((size_t)sh.tri_first[n_tri]);
      at.assign(sh.tri_first.begin(), sh.tri_first.end() - 1);
      for (size_t t = 0; t < n_sph; ++t) sh.sph_first[t + 1] += sh.sph_first[t];
      sh.sph_entry.resize((size_t)sh.sph_first[n_sph]);
      sph_at.assign(sh.sph_first.begin(), sh.sph_first.end() - 1);
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
    b.node_base = 0; b.n_nodes = 0; b.timed = 0;
    for (int32_t i = 0; i < e.c; ++i) {
      const uint32_t ty = rt::primref_type(fs.refs[(size_t)e.b + (size_t)i]);
      if (ty == rt::PRIM_MOVING_SPHERE || ty == rt::PRIM_GRAVITY_SPHERE) b.timed = 1;
    }
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
  // ---- members of instance trees, plain triangle slots
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
    const rt::FlatEntry& e = fs.entries[(size_t)x];
    if (e.kind == rt::ENTRY_PRIM && rt::primref_type((rt::PrimRef)e.a) == rt::PRIM_TRIANGLE) { sh.prim_slot.push_back((int32_t)k); sh.prim_slot.push_back(x); }
  }
  // ---- slots whose f32 box comes from one static sphere (flatten.cpp: "boxes of the plain static primitives"; trace_world.inc:
  // build_world_desc, the boundary sphere of a medium)
  auto sphere_prim = [&](int32_t x) { return fs.entries[(size_t)x].kind == rt::ENTRY_PRIM && rt::primref_type((rt::PrimRef)fs.entries[(size_t)x].a) == rt::PRIM_SPHERE; };
  auto medium_sphere = [&](size_t k) -> int32_t {  // the PRIM entry of the boundary sphere of slot k, -1
    if (k >= fs.top_level.size()) return -1;
    const rt::FlatEntry& e = fs.entries[(size_t)fs.top_level[k]];
    if (e.kind != rt::ENTRY_MEDIUM || e.a < 0 || (size_t)e.a >= n_ent) return -1;
    return sphere_prim(e.a) ? e.a : -1;
  };
  for (size_t k = 0; k < fs.top_level.size(); ++k) {
    const int32_t x = fs.top_level[k], m = medium_sphere(k);
    if (sphere_prim(x)) { sh.sphere_slot.push_back((int32_t)k); sh.sphere_slot.push_back(x); sh.sphere_slot.push_back(0); sh.sphere_slot.push_back(medium_sphere(k + 1)); }
    else if (m >= 0) { sh.sphere_slot.push_back((int32_t)k); sh.sphere_slot.push_back(m); sh.sphere_slot.push_back(1); sh.sphere_slot.push_back(-1); }
  }
  return sh;
}

// The checks every entry makes before it looks at a vertex.  `scene`, `vertices`: compared with NULL, never read.
inline bool check_triangle_ids(const char* who, const void* scene, const MeshShadow* sh, const int32_t* ids, int64_t n, const void* vertices,
                               std::string* err) {
  if (!scene) { *err = std::string(who) + ": the scene is NULL"; return false; }
  if (n < 0) { *err = std::string(who) + ": n < 0"; return false; }
  if (!ids) { *err = std::string(who) + ": ids is NULL"; return false; }
  if (!vertices) { *err = std::string(who) + ": vertices is NULL"; return false; }
  if (n == 0) return true;
  if (!sh->broken.empty()) { *err = std::string(who) + ": " + sh->broken; return false; }
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= sh->n_ids) {
      *err = std::string(who) + ": ids[" + std::to_string(i) + "] is out of range (the scene has " + std::to_string(sh->n_ids) + " triangle ids)";
      return false;
    }
  std::vector<int32_t> sorted(ids, ids + n);
  std::sort(sorted.begin(), sorted.end());
  for (size_t i = 1; i < sorted.size(); ++i)
    if (sorted[i] == sorted[i - 1]) { *err = std::string(who) + ": ids names triangle " + std::to_string(sorted[i]) + " twice"; return false; }
  return true;
}

// Host entries only.
inline bool check_vertices_finite(const char* who, const double* vertices, int64_t n, std::string* err) {
  for (int64_t i = 0; i < 9 * n; ++i)
    if (!std::isfinite(vertices[i])) {
      *err = std::string(who) + ": vertices[" + std::to_string(i / 9) + "][" + std::to_string(i % 9) + "] is not finite";
      return false;
    }
  return true;
}

// From the touched entries (one flag per entry) to the BVHs to refit, the members whose local box changes and the instance
// trees above them: the half of a plan the triangle and the sphere updates share.  what: "triangle" / "sphere", for the
// message.  RTX_EUNSUPPORTED when a touched BVH holds a Moving- or GravitySphere.
inline rtx_status plan_touched_entries(const char* who, const char* what, const MeshShadow& sh, const std::vector<char>& touched,
                                       std::vector<int32_t>* bvhs, std::vector<int32_t>* members, std::vector<int32_t>* trees, std::string* err) {
  for (size_t b = 0; b < sh.bvhs.size(); ++b) {
    if (!touched[(size_t)sh.bvhs[b].entry]) continue;
    if (sh.bvhs[b].timed) {
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
inline rtx_status plan_triangle_update(const char* who, const MeshShadow& sh, const int32_t* ids, int64_t n,
                                       TrianglePlan* plan, std::string* err) {
  *plan = TrianglePlan();
  std::vector<char> touched(sh.bvh_of_entry.size(), 0);
  for (int64_t i = 0; i < n; ++i)
    for (int32_t k = sh.id_first[(size_t)ids[i]]; k < sh.id_first[(size_t)ids[i] + 1]; ++k) {
      const int32_t t = sh.id_flat[(size_t)k];
      plan->pairs.push_back(t);
      plan->pairs.push_back((int32_t)i);
      for (int32_t q = sh.tri_first[(size_t)t]; q < sh.tri_first[(size_t)t + 1]; ++q) touched[(size_t)sh.tri_entry[(size_t)q]] = 1;
    }
  const rtx_status st = plan_touched_entries(who, "triangle", sh, touched, &plan->bvhs, &plan->members, &plan->trees, err);
  if (st != RTX_OK) return st;
  for (size_t k = 0; k < sh.prim_slot.size(); k += 2)
    if (touched[(size_t)sh.prim_slot[k + 1]]) plan->slots.push_back(sh.prim_slot[k]);
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

// rtx_flat_set_triangles: every check first, then the edit.  Not RTX_OK: *err set and *fs untouched.
inline rtx_status flat_set_triangles(const char* who, FlatScene* fs, const int32_t* ids, int64_t n, const double* vertices, std::string* err) {
  MeshShadow sh;
  UpdateShadow us;
  if (fs && n > 0) {
    us = build_update_shadow(*fs);
    sh = build_mesh_shadow(*fs, us);
  }
  if (!check_triangle_ids(who, fs, &sh, ids, n, vertices, err)) return RTX_EINVAL;
  if (n == 0) return RTX_OK;
  if (!check_vertices_finite(who, vertices, n, err)) return RTX_EINVAL;
  TrianglePlan plan;
  const rtx_status st = plan_triangle_update(who, sh, ids, n, &plan, err);
  if (st != RTX_OK) return st;
  for (size_t k = 0; k < plan.pairs.size(); k += 2)
    rt::set_triangle_vertices(&fs->triangles[(size_t)plan.pairs[k]], vertices + 9 * (size_t)plan.pairs[k + 1]);
  for (int32_t b : plan.bvhs) refit_bvh(fs, sh.bvhs[(size_t)b]);
  for (int32_t m : plan.members)
    member_local_box_of(fs->entries[(size_t)sh.members[(size_t)m].geom], fs->nodes.data(), fs->refs.data(), fs->spheres.data(), fs->rects.data(),
                        fs->triangles.data(), &fs->member_local_box[6 * (size_t)m]);
  for (int32_t t : plan.trees) refit_instance_tree(fs, us.trees[(size_t)t]);
  for (int32_t slot : plan.slots)
    rt::plain_slot_box32((rt::PrimRef)fs->entries[(size_t)fs->top_level[(size_t)slot]].a, nullptr, nullptr, fs->triangles.data(), &fs->top_box32[6 * (size_t)slot]);
  return RTX_OK;
}

// rtx_flat_triangle_ids: the ids of the triangles below `object`, in list order.  -1 with *err set.
inline int64_t flat_triangle_ids(const FlatScene& fs, const SceneGraph& g, int32_t object, int32_t* ids, int64_t cap, std::string* err) {
  if (!g.valid_hittable(object)) { *err = "rtx_flat_triangle_ids: bad object handle"; return -1; }
  int64_t count = 0;
  std::vector<std::pair<int32_t, int>> todo{{object, 0}};  // depth-first, children in list order
  while (!todo.empty()) {
    const std::pair<int32_t, int> at = todo.back();
    todo.pop_back();
    if (at.second > 80) { *err = "rtx_flat_triangle_ids: objects nested deeper than 80"; return -1; }
    if ((size_t)at.first >= fs.handle_triangle_id.size()) { *err = "rtx_flat_triangle_ids: the object was made after this flat scene was flattened"; return -1; }
    const GHittable& o = g.hittables[(size_t)at.first];
    if (o.kind == H_TRIANGLE) {
      const int32_t id = fs.handle_triangle_id[(size_t)at.first];
      if (id < 0) { *err = "rtx_flat_triangle_ids: this flat scene did not flatten the object (a triangle below it has no id)"; return -1; }
      if (ids && count < cap) ids[count] = id;
      ++count;
      continue;
    }
    for (size_t c = o.children.size(); c-- > 0;) todo.push_back({o.children[c], at.second + 1});
  }
  return count;
}

}  // namespace rtx
