// The arithmetic of a Morton-ordered Karras tree over the members of an instance tree, and the cost of such a tree.  ONE text for
// the device rebuild (hip/scene_rebuild.inc) and its host twin (host/rebuild_instances.hpp): a rebuilt resident tree is judged
// byte for byte against the host's, so the Morton codes, the node ranges, the split axis and the areas must round alike.
// Everything here is f64 or integer arithmetic whatever rt::real is.
//
// The Morton code and the node function restate hip/lbvh.hip's k_morton and k_radix_tree (cluster 1) so that they compile for
// the host as well; lbvh.hip keeps its own text and its kernels are untouched.
#pragma once
#include "flat_types.hpp"

namespace rt {

RT_HD unsigned long long morton_spread21(unsigned long long x) {  // bit k of x -> bit 3k
  x &= 0x1fffffull;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}

// 63-bit Morton code of the centroid of `box` (lo xyz, hi xyz) inside `bounds` (min xyz, max xyz of all centroids), 21 bits per
// axis.  An axis without extent (hi > lo is false) contributes 0.
RT_HD unsigned long long morton63(const double* box, const double* bounds) {
  unsigned long long code = 0;
  for (int a = 0; a < 3; ++a) {
    const double lo = bounds[a], hi = bounds[3 + a];
    const double c = 0.5 * (box[a] + box[3 + a]);
    double u = hi > lo ? (c - lo) / (hi - lo) : 0.0;
    u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
    if (!(u == u)) u = 0.0;
    const unsigned long long q = (unsigned long long)(u * 2097151.0);
    code |= morton_spread21(q) << (2 - a);
  }
  return code;
}

// Length of the common prefix of keys i and j; equal keys are told apart by their index (Karras 2012, sec. 4).
RT_HD int karras_delta(const unsigned long long* keys, int m, int i, int j) {
  if (j < 0 || j >= m) return -1;
  const unsigned long long a = keys[i], b = keys[j];
  if (a == b) return 64 + __builtin_clz((unsigned)(i ^ j));
  return __builtin_clzll(a ^ b);
}

// Internal node i (0 <= i < m - 1) of the binary radix tree over m >= 2 sorted keys.  A child code >= 0 is an internal node,
// < 0 is ~leaf where leaf is a position in the sorted order.  The root is node 0.
struct KarrasNode { int left, right; };
RT_HD KarrasNode karras_node(const unsigned long long* keys, int m, int i) {
  const int d = karras_delta(keys, m, i, i + 1) - karras_delta(keys, m, i, i - 1) >= 0 ? 1 : -1;
  const int dmin = karras_delta(keys, m, i, i - d);
  int lmax = 2;
  while (karras_delta(keys, m, i, i + lmax * d) > dmin) lmax <<= 1;
  int l = 0;
  for (int t = lmax >> 1; t >= 1; t >>= 1)
    if (karras_delta(keys, m, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = karras_delta(keys, m, i, j);
  int s = 0;
  for (int t = (l + 1) >> 1;; t = (t + 1) >> 1) {
    if (karras_delta(keys, m, i, i + (s + t) * d) > dnode) s += t;
    if (t == 1) break;
  }
  const int gamma = i + s * d + (d < 0 ? -1 : 0);
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  KarrasNode n;
  n.left = lo == gamma ? ~gamma : gamma;
  n.right = hi == gamma + 1 ? ~(gamma + 1) : gamma + 1;
  return n;
}

// lbvh.hip's k_emit_nodes rule: the axis on which the centres of the two child boxes (lo xyz, hi xyz) are farthest apart, the
// lowest such axis on a tie.  Always 0..2: the instance walk of world_hit picks the near child as (dir_neg >> axis) & 1, and
// the value 3 ("child 0 first, whatever the ray") is the SAH builder's own and is never produced here.
RT_HD int karras_split_axis(const double* b0, const double* b1) {
  int axis = 0;
  double sep = -1.0;
  for (int a = 0; a < 3; ++a) {
    const double d = rt_fabs(0.5 * (b0[a] + b0[3 + a]) - 0.5 * (b1[a] + b1[3 + a]));
    if (d > sep) { sep = d; axis = a; }
  }
  return axis;
}

// Surface area of a box from its planes (rtx_*_instance_tree_cost).  The build has -ffp-contract=off, so host and device
// evaluate the same three products and two sums.
RT_HD double box_surface_area(const double* lo, const double* hi) {
  const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
  return 2 * (dx * dy + dy * dz + dz * dx);
}

}  // namespace rt
