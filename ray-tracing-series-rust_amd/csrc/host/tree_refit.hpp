// What the host twins of the scene updates share (host/set_transforms.hpp, host/set_triangles.hpp, host/rebuild_instances.hpp):
// the narrowed copies of a node's planes and the bottom-up refit of one binary tree piece.  Pure host code of the f64 side.
// host/flatten.cpp does not use it: a flat scene built from scratch is the judge these are held to.
#pragma once
#include <vector>
#include "../core/member_box.hpp"
#include "flat_scene.hpp"

namespace rtx {

// nodes32[n]'s planes from nodes[n]'s, narrowed outward with the device's text (rt::f32_narrow_*: the bits of f32_layout.hpp's
// narrow_*), and where the scene has time-aware boxes motion32[n] as the static box without slopes (flatten.cpp:
// build_motion_boxes gives that to an instance tree, which has no time interval, and to a BVH without a moving sphere).
inline void narrow_node_planes(FlatScene* fs, size_t n) {
  const rt::FlatNode& nd = fs->nodes[n];
  rt::FlatNode32& m = fs->nodes32[n];
  for (int c = 0; c < 2; ++c)
    for (int a = 0; a < 3; ++a) { m.lo[c][a] = rt::f32_narrow_down(nd.bmin[c][a]); m.hi[c][a] = rt::f32_narrow_up(nd.bmax[c][a]); }
  if (fs->motion32.empty()) return;
  rt::FlatMotion32& mo = fs->motion32[n];
  for (int c = 0; c < 2; ++c)
    for (int a = 0; a < 3; ++a) { mo.lo0[c][a] = m.lo[c][a]; mo.hi0[c][a] = m.hi[c][a]; mo.dlo[c][a] = 0.0f; mo.dhi[c][a] = 0.0f; }
}

// The tree below `root`, whose nodes are nodes[node_base .. node_base + n_nodes), refitted bottom-up: every child box of every
// node, in nodes, nodes32 and motion32.  leaf_box(code, b) gives the box of a leaf code (lo xyz, hi xyz); a node's box is the
// exact min / max union of its two child boxes, the device's rt_fmin / rt_fmax.  Topology is not touched.
template <class LeafBox>
inline void refit_tree_piece(FlatScene* fs, int32_t root, int32_t node_base, int32_t n_nodes, LeafBox leaf_box) {
  struct Box { double b[6]; };
  // children before parents: a breadth-first order from the root, walked backwards
  std::vector<int32_t> order{root};
  for (size_t k = 0; k < order.size(); ++k)
    for (int c = 0; c < 2; ++c)
      if (!rt::node_child_is_leaf(fs->nodes[(size_t)order[k]].child[c])) order.push_back(fs->nodes[(size_t)order[k]].child[c]);
  std::vector<Box> whole((size_t)n_nodes);  // the union of a node's two child boxes, by node - node_base
  for (size_t k = order.size(); k-- > 0;) {
    const int32_t n = order[k];
    rt::FlatNode& nd = fs->nodes[(size_t)n];
    Box u;
    for (int c = 0; c < 2; ++c) {
      Box cb;
      if (rt::node_child_is_leaf(nd.child[c])) leaf_box(nd.child[c], cb.b);
      else cb = whole[(size_t)(nd.child[c] - node_base)];
      for (int a = 0; a < 3; ++a) { nd.bmin[c][a] = cb.b[a]; nd.bmax[c][a] = cb.b[3 + a]; }
      if (c == 0) u = cb;
      else for (int a = 0; a < 3; ++a) { u.b[a] = rt::rt_fmin(u.b[a], cb.b[a]); u.b[3 + a] = rt::rt_fmax(u.b[3 + a], cb.b[3 + a]); }
    }
    whole[(size_t)(n - node_base)] = u;
    narrow_node_planes(fs, (size_t)n);
  }
}

}  // namespace rtx
