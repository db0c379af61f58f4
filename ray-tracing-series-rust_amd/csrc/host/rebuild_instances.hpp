// rtx_flat_rebuild_instance_trees and rtx_flat_instance_tree_cost on the host.  Pure host code of the f64 side: abi.cpp and
// tests/rebuild_host_check.cpp compile it.  What a rebuild shares with the device side -- the check of the tree list, the stack
// rule, the depth walk, the sum of the cost -- is at the end of host/update_shadow.hpp, which both compilations of render.hip
// include.
//
// A rebuild replaces the TOPOLOGY of an instance tree with one built from its members' world boxes at the ops now in
// `entries`.  The members stay the same n_slots consecutive slots and the tree keeps its piece of n_slots - 1 nodes, so no
// array grows or moves: nodes / nodes32 / the static copy in motion32 of that piece are written, the root in the tree's
// ENTRY_INSTANCE record, and max_stack.  Two builders:
//   RTX_REBUILD_MORTON  the host restatement of the device rebuild (hip/scene_rebuild.inc), step for step: member boxes in
//                       f64, 63-bit Morton codes of their centroids, a stable sort, Karras' radix tree (core/karras.hpp), exact
//                       unions bottom-up.  Node i of the radix tree is node node_base + i; the root is node_base.
//   RTX_REBUILD_SAH     the flattener's own build_bvh with max_leaf = 1 on the same boxes: the flat scene then equals a fresh
//                       rtx_flatten of the pose byte for byte.
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>
#include "../core/karras.hpp"
#include "f32_layout.hpp"
#include "tree_refit.hpp"
#include "update_shadow.hpp"

namespace rtx {

inline double flat_instance_tree_cost(const FlatScene& fs, const TreeShadow& t) {
  std::vector<double> term((size_t)t.n_nodes);
  for (int32_t i = 0; i < t.n_nodes; ++i) {
    const rt::FlatNode& nd = fs.nodes[(size_t)(t.node_base + i)];
    term[(size_t)i] = rt::box_surface_area(nd.bmin[0], nd.bmax[0]) + rt::box_surface_area(nd.bmin[1], nd.bmax[1]);
  }
  const rt::FlatNode& r = fs.nodes[(size_t)t.root];
  double lo[3], hi[3];
  for (int a = 0; a < 3; ++a) { lo[a] = std::fmin(r.bmin[0][a], r.bmin[1][a]); hi[a] = std::fmax(r.bmax[0][a], r.bmax[1][a]); }
  return instance_tree_cost_from_terms(term.data(), t.n_nodes, rt::box_surface_area(lo, hi));
}

// The world boxes of tree t's members at the ops now in `entries` (6 doubles per member, slot order).
inline std::vector<double> member_boxes_now(const FlatScene& fs, const TreeShadow& t) {
  std::vector<double> boxes(6 * (size_t)t.n_slots);
  for (int32_t m = 0; m < t.n_slots; ++m)
    rt::member_world_box(fs.entries[(size_t)fs.top_level[(size_t)(t.first_slot + m)]], t.first_slot + m, nullptr,
                         &fs.member_local_box[6 * (size_t)(t.member_first + m)], &boxes[6 * (size_t)m]);
  return boxes;
}

// One tree as a builder leaves it: n_slots - 1 nodes with ABSOLUTE child indices (node_base + i), root at [0].
struct RebuiltTree {
  std::vector<rt::FlatNode> nodes;
  int32_t depth = 0;
};

// Steps 2 to 4 of the device rebuild on the host: Morton codes, stable sort, Karras tree, exact unions, split axes.
inline RebuiltTree rebuild_tree_morton(const std::vector<double>& boxes, const TreeShadow& t) {
  const int m = t.n_slots;
  double bounds[6] = {HUGE_VAL, HUGE_VAL, HUGE_VAL, -HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
  for (int k = 0; k < m; ++k)
    for (int a = 0; a < 3; ++a) {
      const double c = 0.5 * (boxes[6 * (size_t)k + a] + boxes[6 * (size_t)k + 3 + a]);
      bounds[a] = std::fmin(bounds[a], c); bounds[3 + a] = std::fmax(bounds[3 + a], c);
    }
  std::vector<unsigned long long> code((size_t)m), keys((size_t)m);
  for (int k = 0; k < m; ++k) code[(size_t)k] = rt::morton63(&boxes[6 * (size_t)k], bounds);
  std::vector<uint32_t> order((size_t)m);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return code[a] < code[b]; });
  for (int k = 0; k < m; ++k) keys[(size_t)k] = code[order[(size_t)k]];
  std::vector<rt::KarrasNode> kn((size_t)(m - 1));
  for (int i = 0; i < m - 1; ++i) kn[(size_t)i] = rt::karras_node(keys.data(), m, i);
  // children before parents: a breadth-first order from the root, walked backwards
  std::vector<int32_t> bfs{0}, level{1};
  RebuiltTree out;
  for (size_t k = 0; k < bfs.size(); ++k) {
    out.depth = std::max(out.depth, level[k]);
    for (int code_c : {kn[(size_t)bfs[k]].left, kn[(size_t)bfs[k]].right})
      if (code_c >= 0) { bfs.push_back(code_c); level.push_back(level[k] + 1); }
  }
  struct Box { double b[6]; };
  std::vector<Box> whole((size_t)(m - 1));
  out.nodes.resize((size_t)(m - 1));
  for (size_t k = bfs.size(); k-- > 0;) {
    const int i = bfs[k];
    const int ch[2] = {kn[(size_t)i].left, kn[(size_t)i].right};
    rt::FlatNode& nd = out.nodes[(size_t)i];
    Box cb[2];
    for (int c = 0; c < 2; ++c) {
      if (ch[c] >= 0) {
        cb[c] = whole[(size_t)ch[c]];
        nd.child[c] = t.node_base + ch[c];
      } else {
        const uint32_t member = order[(size_t)~ch[c]];
        for (int a = 0; a < 6; ++a) cb[c].b[a] = boxes[6 * (size_t)member + a];
        nd.child[c] = rt::make_leaf((uint32_t)t.first_slot + member, 1u);
      }
      for (int a = 0; a < 3; ++a) { nd.bmin[c][a] = cb[c].b[a]; nd.bmax[c][a] = cb[c].b[3 + a]; }
    }
    for (int a = 0; a < 3; ++a) { whole[(size_t)i].b[a] = std::fmin(cb[0].b[a], cb[1].b[a]); whole[(size_t)i].b[3 + a] = std::fmax(cb[0].b[3 + a], cb[1].b[3 + a]); }
    nd.pad[0] = rt::karras_split_axis(cb[0].b, cb[1].b);
    nd.pad[1] = 0;
  }
  return out;
}

// The flattener's build (flatten.cpp: emit_instance) on the current boxes.
inline bool rebuild_tree_sah(const std::vector<double>& boxes, const TreeShadow& t, const BuildOptions& opt, RebuiltTree* out, std::string* err) {
  BuildOptions bo = opt;
  bo.max_leaf = 1;
  // build_bvh appends to a vector and emits absolute indices: give it one that ends where the tree's piece begins
  std::vector<rt::FlatNode> tmp((size_t)t.node_base);
  std::vector<uint32_t> order;
  double sah = 0.0;
  const int32_t root = build_bvh(boxes, bo, &tmp, &order, &out->depth, &sah);
  if (root != t.node_base || tmp.size() != (size_t)(t.node_base + t.n_nodes)) { *err = "the SAH builder did not return one piece of n_slots - 1 nodes"; return false; }
  out->nodes.assign(tmp.begin() + t.node_base, tmp.end());
  for (rt::FlatNode& nd : out->nodes)
    for (int c = 0; c < 2; ++c) {
      const int32_t code = nd.child[c];
      if (!rt::node_child_is_leaf(code)) continue;
      if (rt::leaf_count(code) != 1u) { *err = "the SAH builder made a leaf of more than one slot"; return false; }
      nd.child[c] = rt::make_leaf((uint32_t)t.first_slot + order[rt::leaf_first(code)], 1u);
    }
  return true;
}

// The tree's piece of nodes / nodes32 / motion32 written from `r`, and its root (always node_base) into its record.
inline void commit_rebuilt_tree(FlatScene* fs, const TreeShadow& t, int32_t k, const RebuiltTree& r) {
  for (int32_t i = 0; i < t.n_nodes; ++i) {
    const size_t n = (size_t)(t.node_base + i);
    const rt::FlatNode& nd = r.nodes[(size_t)i];
    fs->nodes[n] = nd;
    narrow_node_planes(fs, n);
    rt::FlatNode32& m = fs->nodes32[n];
    m.child[0] = nd.child[0]; m.child[1] = nd.child[1];
    m.axis = nd.pad[0]; m.pad = 0;
  }
  int32_t seen = 0;
  for (rt::FlatEntry& e : fs->entries)
    if (e.kind == rt::ENTRY_INSTANCE && e.a >= 0 && seen++ == k) e.a = t.node_base;
}

// rtx_flat_rebuild_instance_trees: every check first, then every tree built aside, then the edit.  RTX_OK, or RTX_EINVAL /
// RTX_EUNSUPPORTED with *err set and *fs untouched.
inline rtx_status flat_rebuild_instance_trees(const char* who, FlatScene* fs, const BuildOptions& opt, const int32_t* trees, int32_t n,
                                              int32_t builder, std::string* err) {
  if (!fs) { *err = std::string(who) + ": the scene is NULL"; return RTX_EINVAL; }
  if (builder != RTX_REBUILD_MORTON && builder != RTX_REBUILD_SAH) { *err = std::string(who) + ": builder is neither RTX_REBUILD_MORTON nor RTX_REBUILD_SAH"; return RTX_EINVAL; }
  const UpdateShadow sh = build_update_shadow(*fs);
  if (!sh.broken.empty()) { *err = std::string(who) + ": " + sh.broken; return RTX_EINVAL; }
  std::vector<int32_t> list;
  if (!check_rebuild_list(who, fs, sh.trees.size(), trees, n, &list, err)) return RTX_EINVAL;
  if (list.empty()) return RTX_OK;
  std::vector<int32_t> depth(sh.trees.size());
  for (size_t k = 0; k < sh.trees.size(); ++k) depth[k] = instance_tree_depth(fs->nodes.data(), sh.trees[k].root);
  const int32_t member_stack = fs->max_stack - instance_max_stack(0, depth);
  std::vector<RebuiltTree> built(list.size());
  for (size_t i = 0; i < list.size(); ++i) {
    const TreeShadow& t = sh.trees[(size_t)list[i]];
    const std::vector<double> boxes = member_boxes_now(*fs, t);
    if (builder == RTX_REBUILD_MORTON) built[i] = rebuild_tree_morton(boxes, t);
    else if (!rebuild_tree_sah(boxes, t, opt, &built[i], err)) { *err = std::string(who) + ": " + *err; return RTX_EINVAL; }
    depth[(size_t)list[i]] = built[i].depth;
  }
  const int32_t max_stack = instance_max_stack(member_stack, depth);
  if (builder == RTX_REBUILD_MORTON && max_stack > kMaxWalkStack) {
    *err = std::string(who) + ": the rebuilt trees need a walk stack of " + std::to_string(max_stack + 1) + " levels, the launchers accept " +
           std::to_string(kMaxWalkStack + 1) + " (the scene is unchanged)";
    return RTX_EUNSUPPORTED;
  }
  for (size_t i = 0; i < list.size(); ++i) commit_rebuilt_tree(fs, sh.trees[(size_t)list[i]], list[i], built[i]);
  fs->max_stack = max_stack;
  fs->instance_depth = instance_max_stack(0, depth) - 1;
  return RTX_OK;
}

}  // namespace rtx
