// The device step functions of csrc/hip/trace_vote.inc (walk_node_step32, wide_sign_pack, wide_key, slab_interval_nf,
// walk_node_step4) compiled for the HOST, for scripts/mutate_culling.py: one lane, TRACE_BLOCK 1, `__device__` defined away,
// float4 / int4 as plain structs, v_med3_f32 as the median with min3 when an operand is a NaN, the two stack types copied from
// render.hip.  Reads the input of tests/wide_step_host_check.cpp's `steps` mode and writes what rtx_device_walk_steps returns.
// steps.inc, CORE/ and HOST/ are made by the script (the step functions' text, copies of csrc/core and csrc/host).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#define __device__
#define __forceinline__ inline
#define __restrict__
struct float4 { float x, y, z, w; };
struct int4 { int x, y, z, w; };
static inline float emu_med3(float a, float b, float c) {
  if (a != a || b != b || c != c) return fminf(fminf(a, b), c);  // v_med3_f32 with a NaN: min3
  return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c));
}
#define __builtin_amdgcn_fmed3f emu_med3
#include "rtx_abi.h"
#include "CORE/cull32.hpp"
#include "CORE/vec3.hpp"
#include "HOST/wide_tree.hpp"
namespace rt { inline uint32_t ray_dir_neg(const Ray& r) { return (r.direction.x < 0 ? 1u : 0u) | (r.direction.y < 0 ? 2u : 0u) | (r.direction.z < 0 ? 4u : 0u); } }
using rtx::FlatNode4;
#define TRACE_BLOCK 1
#define WALK_DONE 0x7fffffff
struct LdsStack {
  int32_t* base; int n;
  static constexpr bool kBottom = false;
  void reset() { n = 0; }
  void push(int32_t v) { base[n * TRACE_BLOCK] = v; ++n; }
  int32_t pop() { --n; return base[n * TRACE_BLOCK]; }
  bool empty() const { return n == 0; }
};
struct LdsStackB {
  int32_t* base; int n;
  static constexpr bool kBottom = true;
  void reset() { base[0] = 0x7fffffff; n = 1; }
  void push(int32_t v) { base[n * TRACE_BLOCK] = v; ++n; }
  int32_t pop() { --n; return base[n * TRACE_BLOCK]; }
  int32_t top() const { return base[(n - 1) * TRACE_BLOCK]; }
  bool empty() const { return n <= 1; }
};
#include "steps.inc"
template <int KIND, class STACK>
static void run(const void* nodes, int levels, const RtxWalkStepItem& it, int32_t* o) {
  std::vector<int32_t> mem((size_t)levels + 128, 0x5ca1ab1e);  // wide margins: a mutated step may store far off, either way
  int32_t* col = mem.data() + 64;
  for (int l = 0; l < levels; ++l) col[l] = 0x0badf00d;
  STACK stack; stack.base = col;
  stack.reset();
  for (int k = 0; k < it.n_stack; ++k) stack.push(k + 4 < it.n_stack ? (0x40000000 | k) : it.stack[k - (it.n_stack > 4 ? it.n_stack - 4 : 0)]);
  rt::Ray32 q = {it.q[0], it.q[1], it.q[2], it.q[3], it.q[4], it.q[5], it.q[6], it.q[7]};
  rt::Ray r = rt::make_ray(rt::v3(0, 0, 0), rt::v3(it.dir[0], it.dir[1], it.dir[2]), 0);
  const uint32_t pick = KIND ? wide_sign_pack(r) : rt::ray_dir_neg(r);
  int32_t cur = it.node;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) { if (it.second_node < 0) break; stack.reset(); cur = it.second_node; }
    if (KIND) walk_node_step4((const FlatNode4*)nodes, q, pick, it.t_max32, &cur, stack);
    else walk_node_step32(((const rt::FlatNode32*)nodes)[cur], q, pick, it.t_max32, &cur, stack);
  }
  o[0] = cur; o[1] = stack.n;
  for (int l = 0; l < levels + 4; ++l) o[2 + l] = col[l];
  for (int l = -64; l < levels + 64; ++l) if ((l < 0 || l >= levels + 4) && col[l] != 0x5ca1ab1e) o[2 + levels] = 0x0bad0bad;  // far store: spoil a guard slot
}
int main(int argc, char** argv) {
  FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
  int32_t head[4]; int64_t n;
  if (fread(head, 4, 4, in) != 4 || fread(&n, 8, 1, in) != 1) return 2;
  const int kind = head[0], bottom = head[1], levels = head[2], n_nodes = head[3];
  std::vector<unsigned char> nodes((size_t)n_nodes * (kind ? 128 : 64));
  if (fread(nodes.data(), 1, nodes.size(), in) != nodes.size()) return 2;
  std::vector<RtxWalkStepItem> items((size_t)n);
  if (fread(items.data(), sizeof(RtxWalkStepItem), items.size(), in) != items.size()) return 2;
  std::vector<int32_t> o(2 + (size_t)levels + 4);
  for (const auto& it : items) {
    if (kind && bottom) run<1, LdsStackB>(nodes.data(), levels, it, o.data());
    else if (kind) run<1, LdsStack>(nodes.data(), levels, it, o.data());
    else if (bottom) run<0, LdsStackB>(nodes.data(), levels, it, o.data());
    else run<0, LdsStack>(nodes.data(), levels, it, o.data());
    fwrite(o.data(), 4, o.size(), out);
  }
  fclose(out);
  return 0;
}
