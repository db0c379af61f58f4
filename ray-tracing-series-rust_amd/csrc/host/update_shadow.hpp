// What rtx_flat_set_transforms and rtx_scene_set_transforms know about a flattened scene besides its arrays: which slots carry
// a Translate / RotateY chain and of what shape, and for every instance tree the way UP -- node to parent, member slot to the
// node that holds its box.  Derived from the arrays (and FlatScene::member_local_box) alone, so a flat scene builds it on the
// fly and a device scene keeps it from its upload.  Pure host code, compiled by both compilations of render.hip: nothing here
// reads a `real`.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include "../../../include/rtx_abi.h"
#include "../core/member_box.hpp"
#include "flat_scene.hpp"

namespace rtx {

struct SlotChain {
  int32_t xform = -1;  // index in `entries` of the slot's ENTRY_XFORM (the slot's own entry, or the boundary of its medium); -1: none
  int32_t n_ops = 0;
  int32_t kinds[RT_MAX_XFORM_OPS] = {0, 0, 0, 0};
  int32_t tree = -1;   // the instance tree the slot is a member of
};
struct TreeShadow {
  int32_t root, first_slot, n_slots;
  int32_t node_base, n_nodes;  // its nodes are nodes[node_base .. node_base + n_nodes): the builder appends a tree in one piece
  int32_t member_first;        // index of its first member in the per-member tables
  int32_t node_first;          // index of its first node in the per-node tables
};
struct UpdateShadow {
  std::vector<SlotChain> slots;
  std::vector<TreeShadow> trees;
  std::vector<int32_t> leaf_parent;  // 2 per member: the node whose child box is the member's, and which child
  std::vector<int32_t> node_parent;  // 2 per tree node: its parent (absolute node index, -1 for a root) and which child it is
  std::string broken;                // not empty: the arrays are not what the flattener emits; the message says how
};

inline UpdateShadow build_update_shadow(const FlatScene& fs) {
  UpdateShadow sh;
  sh.slots.resize(fs.top_level.size());
  for (size_t k = 0; k < fs.top_level.size(); ++k) {
    const rt::FlatEntry* E = &fs.entries[(size_t)fs.top_level[k]];
    int32_t x = fs.top_level[k];
    if (E->kind == rt::ENTRY_MEDIUM) { x = E->a; E = &fs.entries[(size_t)E->a]; }
    if (E->kind != rt::ENTRY_XFORM) continue;
    SlotChain& c = sh.slots[k];
    c.xform = x;
    c.n_ops = E->b;
    for (int i = 0; i < E->b && i < RT_MAX_XFORM_OPS; ++i) c.kinds[i] = E->ops[i].op;
  }
  int32_t members = 0, nodes = 0;
  for (const rt::FlatEntry& e : fs.entries) {
    if (e.kind != rt::ENTRY_INSTANCE || e.a < 0) continue;
    TreeShadow t;
    t.root = e.a; t.first_slot = e.b; t.n_slots = e.c;
    t.member_first = members; t.node_first = nodes;
    t.n_nodes = e.c - 1;
    // a binary tree of n leaves has n - 1 nodes; its root is wherever the builder put it inside the piece
    int32_t lo = e.a, hi = e.a;
    std::vector<int32_t> todo{e.a};
    size_t seen = 0;
    while (!todo.empty() && seen <= (size_t)e.c) {
      const int32_t n = todo.back();
      todo.pop_back();
      ++seen;
      if (n < 0 || (size_t)n >= fs.nodes.size()) { sh.broken = "an instance tree names a node outside the node array"; return sh; }
      lo = n < lo ? n : lo; hi = n > hi ? n : hi;
      for (int c = 0; c < 2; ++c)
        if (!rt::node_child_is_leaf(fs.nodes[(size_t)n].child[c])) todo.push_back(fs.nodes[(size_t)n].child[c]);
    }
    if (seen != (size_t)t.n_nodes || hi - lo + 1 != t.n_nodes) { sh.broken = "an instance tree's nodes are not one piece of n_slots - 1 nodes"; return sh; }
    t.node_base = lo;
    sh.leaf_parent.resize(2 * (size_t)(members + e.c), -1);
    sh.node_parent.resize(2 * (size_t)(nodes + t.n_nodes), -1);
    for (int32_t n = lo; n <= hi; ++n)
      for (int c = 0; c < 2; ++c) {
        const int32_t code = fs.nodes[(size_t)n].child[c];
        if (rt::node_child_is_leaf(code)) {
          const int64_t m = (int64_t)rt::leaf_first(code) - e.b;
          if (m < 0 || m >= e.c || rt::leaf_count(code) != 1u) { sh.broken = "an instance tree's leaf names a slot outside its run"; return sh; }
          sh.leaf_parent[2 * (size_t)(members + m)] = n;
          sh.leaf_parent[2 * (size_t)(members + m) + 1] = c;
        } else {
          if (code < lo || code > hi) { sh.broken = "an instance tree's child lies outside its piece"; return sh; }
          sh.node_parent[2 * (size_t)(nodes + code - lo)] = n;
          sh.node_parent[2 * (size_t)(nodes + code - lo) + 1] = c;
        }
      }
    for (int32_t m = 0; m < e.c; ++m) {
      if (sh.leaf_parent[2 * (size_t)(members + m)] < 0) { sh.broken = "an instance tree has a member without a leaf"; return sh; }
      if ((size_t)(e.b + m) < sh.slots.size()) sh.slots[(size_t)(e.b + m)].tree = (int32_t)sh.trees.size();
    }
    members += e.c;
    nodes += t.n_nodes;
    sh.trees.push_back(t);
  }
  if (fs.member_local_box.size() != 6 * (size_t)members) sh.broken = "member_local_box does not hold 6 doubles per member of an instance tree";
  return sh;
}

// The checks of an update that need the scene (the others: host/set_transforms.hpp, check_slot_ops_shape).  u holds RESOLVED
// ops: a rotate_y as v[0] = sin, v[1] = cos.  local_box: FlatScene::member_local_box.  false with *err naming the field.
inline bool check_slot_ops_scene(const char* who, const UpdateShadow& sh, const double* local_box, const RtxSlotOps* u, int64_t n,
                                 std::string* err) {
  auto bad = [&](int64_t i, const std::string& what) { *err = std::string(who) + ": updates[" + std::to_string(i) + "]" + what; return false; };
  if (!sh.broken.empty()) { *err = std::string(who) + ": " + sh.broken; return false; }
  for (int64_t i = 0; i < n; ++i) {
    if ((size_t)u[i].slot >= sh.slots.size()) return bad(i, ".slot is out of range (the world list has " + std::to_string(sh.slots.size()) + " slots)");
    const SlotChain& c = sh.slots[(size_t)u[i].slot];
    if (c.xform < 0) return bad(i, ".slot has no Translate / RotateY chain");
    if (u[i].n_ops != c.n_ops) return bad(i, ".n_ops is " + std::to_string(u[i].n_ops) + ", the slot's chain has " + std::to_string(c.n_ops) + " ops");
    for (int k = 0; k < c.n_ops; ++k)
      if (u[i].ops[k].op != c.kinds[k]) return bad(i, ".ops[" + std::to_string(k) + "].op is not the kind the slot's chain has there");
    if (c.tree >= 0) {
      const TreeShadow& t = sh.trees[(size_t)c.tree];
      static_assert(sizeof(u[i].ops[0]) == sizeof(rt::XformOp64), "RtxSlotOps::ops is rt::XformOp64");
      rt::XformOp64 ops[RT_MAX_XFORM_OPS];
      memcpy(ops, u[i].ops, sizeof(ops));
      double b[6];
      rt::member_box_through_ops(local_box + 6 * (size_t)(t.member_first + u[i].slot - t.first_slot), ops, c.n_ops, b);
      if (!rt::box_is_finite(b)) return bad(i, ".ops give the member a bounding box that is not finite");
    }
  }
  return true;
}

// ---- what a rebuild of an instance tree shares between the host (host/rebuild_instances.hpp) and the device
// (hip/scene_rebuild.inc): the stack rule, the depth walk, the check of the tree list and the sum of the cost.
// The launchers accept stack_bytes(max_stack + 1) <= 64 KB of LDS, one KB per level (render.hip: stack_bytes).
constexpr int32_t kMaxWalkStack = 63;

// The scene's max_stack from its parts (flatten.cpp: inst_depth + 1 + out.max_stack): a member's own BVH is walked above the
// slot walk on one stack, one marker between them.
inline int32_t instance_max_stack(int32_t member_stack, const std::vector<int32_t>& tree_depth) {
  int32_t deepest = 0;
  for (int32_t d : tree_depth) deepest = std::max(deepest, d);
  return deepest + 1 + member_stack;
}

// The height of a tree in nodes, as the builders count it (the stack entries a walk can hold).  NODE: FlatNode of either
// precision.
template <class NODE>
inline int32_t instance_tree_depth(const NODE* nodes, int32_t root) {
  int32_t depth = 0;
  std::vector<std::pair<int32_t, int32_t>> todo{{root, 1}};
  while (!todo.empty()) {
    const std::pair<int32_t, int32_t> n = todo.back();
    todo.pop_back();
    depth = std::max(depth, n.second);
    for (int c = 0; c < 2; ++c)
      if (!rt::node_child_is_leaf(nodes[(size_t)n.first].child[c])) todo.push_back({nodes[(size_t)n.first].child[c], n.second + 1});
  }
  return depth;
}

// The list of trees of one rebuild call -> *out (ascending as given; every tree when trees is NULL).  false with *err naming
// the field: NULL scene, n < 0, an index out of range or named twice.
inline bool check_rebuild_list(const char* who, const void* scene, size_t n_trees, const int32_t* trees, int32_t n, std::vector<int32_t>* out,
                               std::string* err) {
  out->clear();
  if (!scene) { *err = std::string(who) + ": the scene is NULL"; return false; }
  if (n < 0) { *err = std::string(who) + ": n < 0"; return false; }
  if (!trees) {
    for (size_t k = 0; k < n_trees; ++k) out->push_back((int32_t)k);
    return true;
  }
  std::vector<char> seen(n_trees, 0);
  for (int32_t i = 0; i < n; ++i) {
    if (trees[i] < 0 || (size_t)trees[i] >= n_trees) {
      *err = std::string(who) + ": trees[" + std::to_string(i) + "] is out of range (the scene has " + std::to_string(n_trees) + " instance trees)";
      return false;
    }
    if (seen[(size_t)trees[i]]) { *err = std::string(who) + ": trees names tree " + std::to_string(trees[i]) + " twice"; return false; }
    seen[(size_t)trees[i]] = 1;
    out->push_back(trees[i]);
  }
  return true;
}

// rtx_*_instance_tree_cost from f64 planes: the sum, over the tree's nodes in ascending node index, of the areas of the node's
// two child boxes, over the area of the union of the root's two child boxes.  term[i] is node node_base + i's.
inline double instance_tree_cost_from_terms(const double* term, int32_t n_nodes, double root_area) {
  double sum = 0.0;
  for (int32_t i = 0; i < n_nodes; ++i) sum += term[i];
  return sum / root_area;
}
}  // namespace rtx
