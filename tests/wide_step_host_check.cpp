// The f32 culling code on the host, for tests/test_cull_conservative.py and tests/test_gpu_cull_steps.py: a stand-alone program,
// built plain (real = double) and with -DRT_F32 -DRT_REAL=float (the fast mode's arithmetic), with -fsanitize=address,undefined.
//
//   wide_step_host_check verdicts IN OUT
//       IN  int64 n, n x (6 doubles box lo / hi, 8 doubles origin, direction, t_min, t_max)
//       OUT n x (8 floats Ray32, float key, uint32 verdict): what rtx_device_cull_verdicts returns (include/rtx_abi.h), from
//           the HOST side of core/cull32.hpp (make_ray32: 1 / d in f64 rounded, fminf / fmaxf for the slope cap) and a plain
//           restatement of the wide step's slab_interval_nf
//   wide_step_host_check steps IN OUT
//       IN  int32 kind, bottom, levels, n_nodes; int64 n; the records (64 B FlatNode32 / 128 B FlatNode4); n x RtxWalkStepItem
//       OUT n x (2 + levels) int32: the new item, the new n, the live slots [0, n) and 0x0badf00d above them
//           -- one step RESTATED: fmaf / fminf / fmaxf for the planes, the clamp as fminf(fmaxf()) (a NaN becomes t_min), a
//           stable sort of the hit children by key, a std::vector for the stack.  Nothing of trace_vote.inc is included.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/rtx_abi.h"
#include "../ray-tracing-series-rust_amd/csrc/core/cull32.hpp"
#include "../ray-tracing-series-rust_amd/csrc/core/vec3.hpp"
#include "../ray-tracing-series-rust_amd/csrc/host/wide_tree.hpp"

static const int32_t DONE = 0x7fffffff;

static float clamp_key(float entry, float t_min) { return fminf(fmaxf(entry, t_min), 3.0e38f); }

// the wide step's box test: near / far planes already picked
static bool slab_nf(const float* nr, const float* fr, const rt::Ray32& q, float t_max32, float* key) {
  const float tn = clamp_key(fmaxf(fmaxf(fmaf(nr[0], q.ix, -q.oix), fmaf(nr[1], q.iy, -q.oiy)), fmaf(nr[2], q.iz, -q.oiz)), q.t_min);
  const float tf = fminf(fminf(fminf(fmaf(fr[0], q.ix, -q.oix), fmaf(fr[1], q.iy, -q.oiy)), fmaf(fr[2], q.iz, -q.oiz)), t_max32);
  *key = tn;
  return !(tn - tf > fmaf(fabsf(tn) + fabsf(tf), 0x1.0p-21f, q.err2));
}

static int verdicts(FILE* in, FILE* out) {
  int64_t n;
  if (fread(&n, 8, 1, in) != 1 || n < 0) return 2;
  for (int64_t k = 0; k < n; ++k) {
    double v[14];
    if (fread(v, 8, 14, in) != 14) return 2;
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
      lo[a] = (float)v[a];
      if ((double)lo[a] > v[a]) lo[a] = std::nextafterf(lo[a], -INFINITY);
      hi[a] = (float)v[3 + a];
      if ((double)hi[a] < v[3 + a]) hi[a] = std::nextafterf(hi[a], INFINITY);
    }
    const rt::Ray r = rt::make_ray(rt::v3((rt::real)v[6], (rt::real)v[7], (rt::real)v[8]), rt::v3((rt::real)v[9], (rt::real)v[10], (rt::real)v[11]), rt::real(0));
    const rt::real t_min = (rt::real)v[12];
    const rt::Ray32 q = rt::make_ray32(r, t_min);
    const float t_max32 = rt::cull_round_up((rt::real)v[13]);
    const uint32_t neg = rt::ray32_dir_neg(q);
    float nr[3], fr[3];
    for (int a = 0; a < 3; ++a) { nr[a] = (neg >> a & 1u) ? hi[a] : lo[a]; fr[a] = (neg >> a & 1u) ? lo[a] : hi[a]; }
    uint32_t bits = 0;
    if (rt::cull32_may_hit(lo, hi, q, t_max32)) bits |= 1u;
    if (rt::cull32_may_hit_nf(nr[0], fr[0], nr[1], fr[1], nr[2], fr[2], q, t_max32)) bits |= 2u;
    if (t_min > rt::real(0)) {
      bits |= 64u;
      if (rt::cull32_may_hit_nf_pos(nr[0], fr[0], nr[1], fr[1], nr[2], fr[2], q, t_max32)) bits |= 4u;
    }
    bool h0, h1;
    rt::cull32_may_hit2(lo, hi, lo, hi, q, t_max32, &h0, &h1);
    if (h0) bits |= 8u;
    if (h1) bits |= 16u;
    float key;
    for (int a = 0; a < 3; ++a) {  // the wide step picks by the direction's sign bit
      const bool sgn = std::signbit(v[9 + a]);
      nr[a] = sgn ? hi[a] : lo[a]; fr[a] = sgn ? lo[a] : hi[a];
    }
    if (slab_nf(nr, fr, q, t_max32, &key)) bits |= 32u;
    const float o[9] = {q.ix, q.iy, q.iz, q.oix, q.oiy, q.oiz, q.err2, q.t_min, key};
    fwrite(o, 4, 9, out);
    fwrite(&bits, 4, 1, out);
  }
  return 0;
}

static rt::Ray32 ray32_of(const RtxWalkStepItem& it) {
  rt::Ray32 q;
  q.ix = it.q[0]; q.iy = it.q[1]; q.iz = it.q[2]; q.oix = it.q[3]; q.oiy = it.q[4]; q.oiz = it.q[5]; q.err2 = it.q[6]; q.t_min = it.q[7];
  return q;
}

// One wide step: the hit children, nearest first (ties: lower slot first), then onto the stack farthest first; the nearest is
// the next item.  Nothing hit: the top of the stack is, and "done" when the walk's own entries are used up.
static void step4(const rtx::FlatNode4& w, const RtxWalkStepItem& it, std::vector<int32_t>* st, int32_t* cur, bool bottom) {
  const rt::Ray32 q = ray32_of(it);
  struct Hit { float key; int32_t code; };
  std::vector<Hit> hits;
  for (int k = 0; k < 4; ++k) {
    float nr[3], fr[3];
    for (int a = 0; a < 3; ++a) {  // the direction's sign bit: -0.0 travels towards -axis, as its slope -inf says
      const bool neg = std::signbit(it.dir[a]);
      nr[a] = neg ? w.hi[a][k] : w.lo[a][k]; fr[a] = neg ? w.lo[a][k] : w.hi[a][k];
    }
    float key;
    if (slab_nf(nr, fr, q, it.t_max32, &key) && w.child[k] != DONE) hits.push_back({key, w.child[k]});
  }
  std::stable_sort(hits.begin(), hits.end(), [](const Hit& a, const Hit& b) { return a.key < b.key; });
  for (size_t k = hits.size(); k-- > 0;) st->push_back(hits[k].code);
  if (st->empty()) { *cur = DONE; return; }  // (never with a bottom: "done" is popped like any item)
  *cur = st->back();
  st->pop_back();
  (void)bottom;
}

// One binary step: the child that is near along the node's split axis first (axis 3: child 0 first for every ray, the
// builder's "big single leaf first" order).
static void step32(const rt::FlatNode32& nd, const RtxWalkStepItem& it, std::vector<int32_t>* st, int32_t* cur) {
  const rt::Ray32 q = ray32_of(it);
  const bool neg[3] = {it.dir[0] < 0.0, it.dir[1] < 0.0, it.dir[2] < 0.0};
  const int first = (nd.axis >= 0 && nd.axis < 3 && neg[nd.axis]) ? 1 : 0;
  const bool hf = rt::cull32_may_hit(nd.lo[first], nd.hi[first], q, it.t_max32);
  const bool hs = rt::cull32_may_hit(nd.lo[1 - first], nd.hi[1 - first], q, it.t_max32);
  if (hf && hs) { st->push_back(nd.child[1 - first]); *cur = nd.child[first]; }
  else if (hf) *cur = nd.child[first];
  else if (hs) *cur = nd.child[1 - first];
  else if (st->empty()) *cur = DONE;
  else { *cur = st->back(); st->pop_back(); }
}

static int steps(FILE* in, FILE* out) {
  int32_t head[4];
  int64_t n;
  if (fread(head, 4, 4, in) != 4 || fread(&n, 8, 1, in) != 1) return 2;
  const int kind = head[0], bottom = head[1], levels = head[2], n_nodes = head[3];
  if (n_nodes <= 0 || levels < 1 || n < 0) return 2;
  std::vector<rtx::FlatNode4> wide;
  std::vector<rt::FlatNode32> bin;
  if (kind) { wide.resize((size_t)n_nodes); if (fread(wide.data(), 128, wide.size(), in) != wide.size()) return 2; }
  else { bin.resize((size_t)n_nodes); if (fread(bin.data(), 64, bin.size(), in) != bin.size()) return 2; }
  std::vector<RtxWalkStepItem> items((size_t)n);
  if (fread(items.data(), sizeof(RtxWalkStepItem), items.size(), in) != items.size()) return 2;
  for (const RtxWalkStepItem& it : items) {
    if (it.node < 0 || it.node >= n_nodes || it.second_node >= n_nodes || it.n_stack < 0 || it.n_stack + bottom > levels) return 2;
    std::vector<int32_t> st;
    auto reset = [&] { st.clear(); if (bottom) st.push_back(DONE); };
    reset();
    const int base = it.n_stack > 4 ? it.n_stack - 4 : 0;
    for (int k = 0; k < it.n_stack; ++k) st.push_back(k < base ? (0x40000000 | k) : it.stack[k - base]);
    int32_t cur = it.node;
    for (int pass = 0; pass < 2; ++pass) {
      if (pass == 1) {
        if (it.second_node < 0) break;
        reset();
        cur = it.second_node;
      }
      if (kind) step4(wide[(size_t)cur], it, &st, &cur, bottom != 0);
      else step32(bin[(size_t)cur], it, &st, &cur);
    }
    std::vector<int32_t> o(2 + (size_t)levels, 0x0badf00d);
    o[0] = cur;
    o[1] = (int32_t)st.size();
    if ((int)st.size() > levels) return 3;
    for (size_t k = 0; k < st.size(); ++k) o[2 + k] = st[k];
    fwrite(o.data(), 4, o.size(), out);
  }
  return 0;
}

int main(int argc, char** argv) {
  static_assert(sizeof(RtxWalkStepItem) == 88, "the item as tests lay it out");
  if (argc != 4) { fprintf(stderr, "usage: %s verdicts|steps IN OUT\n", argv[0]); return 2; }
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) { perror("open"); return 2; }
  const int rc = strcmp(argv[1], "verdicts") == 0 ? verdicts(in, out) : steps(in, out);
  fclose(in);
  fclose(out);
  if (rc == 0) printf("wide step host check clean\n");
  else fprintf(stderr, "bad input (%d)\n", rc);
  return rc;
}
