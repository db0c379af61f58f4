// The 4-wide culling tree: its record, the host collapse that builds it at upload and the stack a walk of it needs.
// Host code without a HIP dependency (render.hip includes it; tests/wide_tree_host_check.cpp runs it under sanitizers).
//
// On the dragon room the walk is bound by the latency of dependent node fetches (28 MB of culling tree: every step
// waits for L2 / MALL), not by VALU.  A 4-wide tree halves the length of that chain: built at upload by collapsing the
// binary SAH tree (the child with the largest area is opened until four slots are used), one 128-byte record = one
// cache line per step, boxes rounded outward to f32 exactly like FlatNode32.  Wide node i is binary node i opened
// up, so child codes (node index >= 0, leaf code < 0) are the binary tree's and leaves are untouched.  Culling
// structure only: every hit is still decided by the f64 primitive tests, so results do not change.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
#include "../core/flat_types.hpp"

namespace rtx {

struct FlatNode4 {  // 128 B, field-major so that one child's six planes are six scalar picks from float4 loads
  float lo[3][4];
  float hi[3][4];
  int32_t child[4];  // WALK_DONE marks an empty slot (its box is empty too)
  int32_t pad[4];
};
static_assert(sizeof(FlatNode4) == 128, "one cache line per wide node");

// Host: collapse fs.nodes below `root` into `out` (indexed like fs.nodes); returns the peak stack use of a walk.
// A BVH of at most max_leaf primitives has a leaf code for a root (bvh_build.cpp): nothing to collapse, no record, and a
// walk of it stacks nothing -- the walkers start at the leaf code.
static int build_wide_nodes(const std::vector<rt::FlatNode>& nodes, int32_t root, std::vector<FlatNode4>* out) {
  if (root < 0) return 0;
  struct Slot { int32_t code; double mn[3], mx[3]; };
  auto half_area = [](const Slot& s) {
    double dx = s.mx[0] - s.mn[0], dy = s.mx[1] - s.mn[1], dz = s.mx[2] - s.mn[2];
    return dx * dy + dy * dz + dz * dx;
  };
  auto slots_of = [&](int32_t n, Slot* dst) {
    for (int c = 0; c < 2; ++c) {
      dst[c].code = nodes[n].child[c];
      for (int a = 0; a < 3; ++a) { dst[c].mn[a] = nodes[n].bmin[c][a]; dst[c].mx[a] = nodes[n].bmax[c][a]; }
    }
  };
  struct Frame { int32_t node; int next; int nslots; int32_t kids[4]; int peak_kids; };
  std::vector<Frame> stack;
  std::vector<int> peak(nodes.size(), 0);
  auto open = [&](int32_t n) {
    Slot sl[4];
    int ns = 2;
    slots_of(n, sl);
    while (ns < 4) {
      int best = -1;
      double best_area = -1.0;
      for (int k = 0; k < ns; ++k)
        if (sl[k].code >= 0 && half_area(sl[k]) > best_area) { best_area = half_area(sl[k]); best = k; }
      if (best < 0) break;
      Slot two[2];
      slots_of(sl[best].code, two);
      sl[best] = two[0];
      sl[ns++] = two[1];
    }
    FlatNode4& w = (*out)[n];
    Frame f;
    f.node = n; f.next = 0; f.nslots = ns; f.peak_kids = 0;
    for (int k = 0; k < 4; ++k) {
      f.kids[k] = -1;
      if (k < ns) {
        for (int a = 0; a < 3; ++a) {
          float lo = (float)sl[k].mn[a];
          if ((double)lo > sl[k].mn[a]) lo = std::nextafterf(lo, -INFINITY);
          float hi = (float)sl[k].mx[a];
          if ((double)hi < sl[k].mx[a]) hi = std::nextafterf(hi, INFINITY);
          w.lo[a][k] = lo; w.hi[a][k] = hi;
        }
        w.child[k] = sl[k].code;
        if (sl[k].code >= 0) f.kids[k] = sl[k].code;
      } else {
        for (int a = 0; a < 3; ++a) { w.lo[a][k] = INFINITY; w.hi[a][k] = -INFINITY; }
        w.child[k] = 0x7fffffff;
      }
      w.pad[k] = 0;
    }
    stack.push_back(f);
  };
  open(root);
  while (!stack.empty()) {
    Frame& f = stack.back();
    if (f.next < 4) {
      int32_t kid = f.kids[f.next++];
      if (kid >= 0) open(kid);
      continue;
    }
    // all wide children done: a walk pushes up to nslots items here, pops one and descends with nslots - 1 left
    int pk = f.nslots;
    for (int k = 0; k < 4; ++k)
      if (f.kids[k] >= 0) pk = std::max(pk, f.nslots - 1 + peak[f.kids[k]]);
    peak[f.node] = pk;
    stack.pop_back();
  }
  return peak[root];
}

// Stack levels per lane for walks whose peak use (build_wide_nodes) is `peak`.  The spare level is the bottom slot of
// LdsStackB (render.hip), which holds "walk done": its walk starts at n = 1 and the highest slot a step writes is `peak`
// = levels - 1, exactly.  LdsStack starts at n = 0 and stays one slot lower.  walk_node_step4 needs no level of its own:
// the slot its unconditional stores dump into is a dead slot at or below that one.
static inline int wide_stack_levels(int peak) { return peak + 1; }

// The wide tree of every BVH of a scene: `wide` is indexed like `nodes` (records of nodes no wide walk reaches stay zero),
// `roots` are the ENTRY_BVH records' roots.  Returns the stack levels a walk of any of them needs.
static int build_wide_tree(const std::vector<rt::FlatNode>& nodes, const std::vector<int32_t>& roots, std::vector<FlatNode4>* wide) {
  wide->assign(nodes.size(), FlatNode4{});
  int peak = 0;
  for (int32_t root : roots) peak = std::max(peak, build_wide_nodes(nodes, root, wide));
  return wide_stack_levels(peak);
}

}  // namespace rtx
