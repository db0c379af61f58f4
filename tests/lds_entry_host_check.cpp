// lds_entry_pair (csrc/hip/lds_variant.inc) on the host: where a walk of k_trace_lds enters a tree, asked of a node table.
//   lds_entry_host_check <root> <child0> <child1> <axis> [<child0> <child1> <axis> ...]  -> "<entry_first> <entry_second>"
// One triple per node, in node order; children as the flattener codes them (core/flat_types.hpp: a node index, or make_leaf).
// Stand-alone: g++ tests/lds_entry_host_check.cpp && ./a.out 0 -2147483648 1 3 -2147483640 -2147483632 0
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ray-tracing-series-rust_amd/csrc/core/flat_types.hpp"
#define __host__
#define __device__
namespace rtx {
#include "../ray-tracing-series-rust_amd/csrc/hip/lds_layout.inc"
#include "../ray-tracing-series-rust_amd/csrc/hip/lds_variant.inc"
}

int main(int argc, char** argv) {
  if (argc < 5 || (argc - 2) % 3 != 0) {
    std::fprintf(stderr, "usage: see the head of tests/lds_entry_host_check.cpp\n");
    return 2;
  }
  std::vector<rt::FlatNode32> nodes((size_t)(argc - 2) / 3);
  for (size_t k = 0; k < nodes.size(); ++k) {
    nodes[k] = rt::FlatNode32{};
    nodes[k].child[0] = (int32_t)strtol(argv[2 + 3 * k], nullptr, 0);
    nodes[k].child[1] = (int32_t)strtol(argv[3 + 3 * k], nullptr, 0);
    nodes[k].axis = (int32_t)strtol(argv[4 + 3 * k], nullptr, 0);
  }
  const long root = strtol(argv[1], nullptr, 0);
  if (root < 0 || (size_t)root >= nodes.size()) { std::fprintf(stderr, "root %ld of %zu nodes\n", root, nodes.size()); return 2; }
  for (const rt::FlatNode32& n : nodes)
    for (int c = 0; c < 2; ++c)
      if (n.child[c] >= 0 && (size_t)n.child[c] >= nodes.size()) { std::fprintf(stderr, "child %d of %zu nodes\n", n.child[c], nodes.size()); return 2; }
  int32_t entry[2] = {0, 0};
  rtx::lds_entry_pair(nodes.data(), (int32_t)root, entry);
  std::printf("%d %d\n", (int)entry[0], (int)entry[1]);
  return 0;
}
