// The host collapse of the 4-wide culling tree (csrc/host/wide_tree.hpp: build_wide_tree as plan_wide calls it) as a
// stand-alone program, built with -fsanitize=address,undefined by tests/test_wide_tree.py and by `make -C oracle sanitize`.
//
//   wide_tree_host_check IN OUT   IN:  int32 n_nodes, int32 n_roots, n_roots x int32 root, n_nodes x FlatNode (f64, 112 B)
//                                 OUT: int32 levels, n_nodes x FlatNode4 (128 B)
//   wide_tree_host_check          a few trees of its own (a comb, three inner nodes, a root that is a leaf beside a tree)
//
// It judges nothing: the audit of the records is tests/test_wide_tree.py's, in numpy, written from the definition.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../ray-tracing-series-rust_amd/csrc/host/wide_tree.hpp"

static_assert(sizeof(rt::FlatNode) == 112, "the f64 node record");

static rt::FlatNode node(int32_t c0, int32_t c1, double x0, double x1, double x2) {
  rt::FlatNode n;
  memset(&n, 0, sizeof n);
  n.child[0] = c0; n.child[1] = c1;
  for (int a = 0; a < 3; ++a) { n.bmin[0][a] = x0; n.bmax[0][a] = x1; n.bmin[1][a] = x1; n.bmax[1][a] = x2; }
  return n;
}

static int self_run() {
  // a comb of 200 inner nodes: node i = (leaf i, node i + 1), the last one two leaves
  std::vector<rt::FlatNode> nodes;
  const int n = 200;
  for (int i = 0; i < n; ++i)
    nodes.push_back(node(rt::make_leaf((uint32_t)i, 1), i + 1 < n ? i + 1 : rt::make_leaf((uint32_t)n, 1), i, i + 0.1, n + 1.0));
  std::vector<rtx::FlatNode4> wide;
  int levels = rtx::build_wide_tree(nodes, {0}, &wide);
  printf("comb of %d: %d levels\n", n, levels);
  if (levels < 3 || wide.size() != nodes.size()) return 1;
  // a BVH whose root is a leaf (two triangles) beside that tree, and alone
  levels = rtx::build_wide_tree(nodes, {rt::make_leaf(0, 2), 0}, &wide);
  printf("root leaf beside the comb: %d levels\n", levels);
  const int alone = rtx::build_wide_tree(nodes, {rt::make_leaf(0, 2)}, &wide);
  printf("root leaf alone: %d levels\n", alone);
  if (alone != 1) return 1;
  for (const rtx::FlatNode4& w : wide)
    for (int k = 0; k < 4; ++k)
      if (w.child[k] != 0) return 1;
  // no BVH at all, no nodes at all
  std::vector<rt::FlatNode> none;
  if (rtx::build_wide_tree(none, {}, &wide) != 1 || !wide.empty()) return 1;
  printf("wide tree host check clean\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_run();
  if (argc != 3) { fprintf(stderr, "usage: %s [IN OUT]\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t head[2];
  if (fread(head, 4, 2, f) != 2 || head[0] < 0 || head[1] < 0) { fprintf(stderr, "bad header\n"); return 2; }
  std::vector<int32_t> roots((size_t)head[1]);
  std::vector<rt::FlatNode> nodes((size_t)head[0]);
  if (fread(roots.data(), 4, roots.size(), f) != roots.size() || fread(nodes.data(), sizeof(rt::FlatNode), nodes.size(), f) != nodes.size()) {
    fprintf(stderr, "short input\n");
    return 2;
  }
  fclose(f);
  std::vector<rtx::FlatNode4> wide;
  const int32_t levels = rtx::build_wide_tree(nodes, roots, &wide);
  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  fwrite(&levels, 4, 1, f);
  fwrite(wide.data(), sizeof(rtx::FlatNode4), wide.size(), f);
  fclose(f);
  printf("%zu nodes, %zu roots: %d levels\nwide tree host check clean\n", nodes.size(), roots.size(), (int)levels);
  return 0;
}
