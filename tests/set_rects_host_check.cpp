// Host checker of rtx_flat_set_rects and rtx_flat_rect_ids (tests/test_set_rects_host.py builds it with the product's host
// sources under -fsanitize=address,undefined and runs it).  A CPU program with its own main; nothing of it is loaded into Python.
// ONE world holds every place a rectangle can stand: plain slots (one of them an XZ DiffuseLight), a BVH of rectangles and
// spheres, an instance tree of Translate(RotateY(RectPrism)) members and a bare rectangle under a Translate, and one prism
// handle under two Translates.  It is built at rest and with every updatable rectangle moved; the host twin must turn the
// first into the second in every array a fresh build derives from values alone -- rects, top_box32, member_local_box, the light
// table -- full, in two halves and after rtx_flat_set_transforms; moved back, EVERY array must be what it was, byte for byte.
// Then the refusals, each of which must leave the scene untouched.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "../ray-tracing-series-rust_amd/csrc/host/light_table.hpp"
#include "../ray-tracing-series-rust_amd/csrc/host/set_triangles.hpp"

namespace rtx {
// the GPU builder lives in csrc/hip/lbvh.hip: not part of a CPU-only program
int32_t build_bvh_gpu(const std::vector<double>&, int, std::vector<rt::FlatNode>*, std::vector<uint32_t>*, int32_t*, double*, std::string* err) {
  if (err) *err = "no GPU builder in the sanitizer program";
  return -1;
}
}  // namespace rtx

namespace {
struct Val { double v[5]; };
typedef std::function<bool(int)> Moved;  // does the k-th updatable part (in creation order) take its moved values?

// k % 3 == 0: the rectangle leaves its old box; 1: it shrinks; 2: it moves along its thin axis and grows
Val moved_of(const Val& s, int k) {
  Val o = s;
  const double wa = s.v[1] - s.v[0], wb = s.v[3] - s.v[2];
  if (k % 3 == 0) { o.v[0] += 1.37 * wa; o.v[1] += 1.37 * wa; o.v[2] += 0.07 * wb; }
  else if (k % 3 == 1) { o.v[0] += 0.17 * wa; o.v[1] -= 0.13 * wa; o.v[2] += 0.21 * wb; }
  else { o.v[0] -= 0.19 * wa; o.v[3] += 0.23 * wb; o.v[4] += 0.31; }
  return o;
}

struct Part { int32_t handle; std::vector<Val> rest, moved; };  // one rectangle, or the 6 (12: shared) of a prism
struct Built {
  rtx::SceneGraph g{5};
  int32_t world = -1, timed_rect = -1;
  std::vector<Part> parts;
};

void prism_vals(const double* p0, const double* p1, std::vector<Val>* out) {  // RectPrism::new's six, as api.prism_rects spells them
  const Val six[6] = {{{p0[0], p1[0], p0[1], p1[1], p1[2]}}, {{p0[0], p1[0], p0[1], p1[1], p0[2]}}, {{p0[0], p1[0], p0[2], p1[2], p1[1]}},
                      {{p0[0], p1[0], p0[2], p1[2], p0[1]}}, {{p0[1], p1[1], p0[2], p1[2], p1[0]}}, {{p0[1], p1[1], p0[2], p1[2], p0[0]}}};
  out->insert(out->end(), six, six + 6);
}

struct Maker {
  Built* B;
  Moved on;
  int32_t rect(int32_t kind, double a0, double a1, double b0, double b1, double k, int32_t mat) {
    const Val s = {{a0, a1, b0, b1, k}};
    const int n = (int)B->parts.size();
    const Val m = moved_of(s, n);
    const Val& u = on(n) ? m : s;
    const int32_t h = B->g.rect(kind, u.v[0], u.v[1], u.v[2], u.v[3], u.v[4], mat);
    B->parts.push_back({h, {s}, {m}});
    return h;
  }
  int32_t prism(double x, double y, double z, double w, int32_t mat, int copies = 1) {
    const int n = (int)B->parts.size();
    const double p0[3] = {x, y, z}, p1[3] = {x + w, y + 1.3 * w, z + 0.8 * w};
    const double q0[3] = {x + 0.21, y + 0.07, z + 0.13}, q1[3] = {x + 0.21 + 1.4 * w, y + 0.07 + 0.9 * w, z + 0.13 + 1.1 * w};
    const int32_t h = on(n) ? B->g.rect_prism(q0, q1, mat) : B->g.rect_prism(p0, p1, mat);
    Part p{h, {}, {}};
    for (int c = 0; c < copies; ++c) { prism_vals(p0, p1, &p.rest); prism_vals(q0, q1, &p.moved); }
    B->parts.push_back(p);
    return h;
  }
  int32_t list(const std::vector<int32_t>& o) { const int32_t l = B->g.list_new(); for (int32_t x : o) B->g.list_add(l, x); return l; }
};

void make_world(Built* B, const Moved& on, bool with_movers) {
  rtx::SceneGraph& g = B->g;
  Maker m{B, on};
  const double c1[3] = {0.5, 0.5, 0.5}, c2[3] = {0.8, 0.8, 0.9}, le[3] = {7.0, 6.0, 5.0};
  const int32_t grey = g.lambertian(g.solid_color(c1)), metal = g.metal(c2, 0.2), lamp = g.diffuse_light(g.solid_color(le));
  auto ball = [&](double x, double y, double z, double r) { const double c[3] = {x, y, z}; return g.sphere(c, r, grey); };
  std::vector<int32_t> top = {ball(2.0, -500.0, 2.0, 500.0)};
  top.push_back(m.rect(rtx::H_XZ_RECT, 1.13, 2.87, 1.27, 2.93, 3.55, lamp));
  top.push_back(m.rect(rtx::H_YZ_RECT, 0.03, 3.61, 0.04, 4.12, 4.07, grey));
  top.push_back(m.rect(rtx::H_XY_RECT, 0.02, 4.07, 0.03, 3.61, 4.12, metal));
  std::vector<int32_t> in_bvh;
  for (int k = 0; k < 9; ++k) {
    const double x = 0.6 + 0.83 * (k % 3) + 0.017 * k, y = 0.7 + 0.21 * k, z = 0.5 + 0.79 * (k / 3) + 0.013 * k;
    in_bvh.push_back(m.rect(k % 3 == 0 ? rtx::H_XY_RECT : k % 3 == 1 ? rtx::H_XZ_RECT : rtx::H_YZ_RECT, x, x + 0.5 + 0.03 * k, y, y + 0.4, z, k % 2 ? grey : metal));
    if (k % 2) in_bvh.push_back(ball(x + 0.3, y + 1.9, z + 0.2, 0.2 + 0.01 * k));
  }
  top.push_back(g.bvh_from_list(m.list(in_bvh), 0.0, 1.0));
  const double t0[3] = {0.4, 0.2, 0.3}, t1[3] = {3.1, 0.3, 2.2}, t2[3] = {1.2, 0.4, 4.0}, t3[3] = {5.1, 0.2, 0.9}, t4[3] = {6.3, 0.3, 2.4};
  const int32_t a = g.translate(t0, g.rotate_y(20.0, m.prism(0.11, 0.13, 0.12, 0.7, grey)));
  const int32_t b = g.translate(t1, g.rotate_y(-35.0, m.prism(0.14, 0.12, 0.17, 0.5, metal)));
  const int32_t c = g.translate(t2, m.rect(rtx::H_XY_RECT, 0.12, 0.93, 0.11, 1.07, 0.41, grey));
  top.push_back(g.instance_bvh_from_list(m.list({a, b, c})));
  const int32_t shared = m.prism(0.12, 0.11, 0.13, 0.6, grey, 2);
  top.push_back(g.translate(t3, shared));
  top.push_back(g.translate(t4, shared));
  if (with_movers) {
    const double p[3] = {1.0, 6.5, 1.0}, q[3] = {1.0, 7.0, 1.0};
    B->timed_rect = g.rect(rtx::H_XY_RECT, 0.8, 1.9, 6.1, 6.9, 1.4, grey);
    top.push_back(g.bvh_from_list(m.list({B->timed_rect, g.moving_sphere(p, q, 0.0, 1.0, 0.3, grey), ball(3.0, 6.5, 1.0, 0.3)}), 0.0, 1.0));
  }
  B->world = m.list(top);
}

bool flatten(const Moved& on, Built* B, rtx::FlatScene* fs, bool with_movers = false) {
  make_world(B, on, with_movers);
  std::string err;
  if (B->world < 0 || !rtx::flatten_scene(B->g, B->world, rtx::BuildOptions(), fs, &err)) { fprintf(stderr, "flatten: %s %s\n", B->g.error.c_str(), err.c_str()); return false; }
  return true;
}

// ids (through flat_rect_ids) and values that give the parts chosen by `pick` their moved or rest values
bool update_for(const Built& B, const rtx::FlatScene& fs, const Moved& pick, bool to_moved, std::vector<int32_t>* ids, std::vector<double>* vals) {
  ids->clear(); vals->clear();
  for (size_t k = 0; k < B.parts.size(); ++k) {
    if (!pick((int)k)) continue;
    const Part& p = B.parts[k];
    std::string err;
    std::vector<int32_t> got(p.rest.size() + 1, -1);
    const int64_t n = rtx::flat_rect_ids("ids", fs, B.g, p.handle, got.data(), (int64_t)got.size(), &err);
    if (n != (int64_t)p.rest.size()) { fprintf(stderr, "part %zu: %lld ids, %zu expected (%s)\n", k, (long long)n, p.rest.size(), err.c_str()); return false; }
    for (int64_t i = 0; i < n; ++i) {
      ids->push_back(got[(size_t)i]);
      const Val& s = (to_moved ? p.moved : p.rest)[(size_t)i];
      vals->insert(vals->end(), s.v, s.v + 5);
    }
  }
  return true;
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }
bool same_lights(const rtx::FlatScene& a, const rtx::FlatScene& b) { return same(rtx::build_light_table(a).lights, rtx::build_light_table(b).lights); }
// every array
bool same_arrays(const rtx::FlatScene& a, const rtx::FlatScene& b, const char* what) {
  const bool ok = same(a.triangles, b.triangles) && same(a.entries, b.entries) && same(a.top_level, b.top_level) && same(a.nodes, b.nodes) &&
                  same(a.nodes32, b.nodes32) && same(a.motion32, b.motion32) && same(a.member_local_box, b.member_local_box) && same(a.refs, b.refs) &&
                  same(a.rects, b.rects) && same(a.spheres, b.spheres) && same(a.top_box32, b.top_box32) && same(a.handle_rect_first, b.handle_rect_first) &&
                  same(a.handle_rect_id, b.handle_rect_id) && same_lights(a, b);
  if (!ok) fprintf(stderr, "%s: the arrays differ\n", what);
  return ok;
}
// what a fresh build derives from the values alone (its BVHs may choose another topology)
bool same_derived(const rtx::FlatScene& a, const rtx::FlatScene& b, const char* what) {
  const bool ok = same(a.rects, b.rects) && same(a.top_box32, b.top_box32) && same(a.member_local_box, b.member_local_box) && same_lights(a, b) &&
                  a.nodes.size() == b.nodes.size();
  if (!ok) fprintf(stderr, "%s: rects, top_box32, member_local_box or the light table differ from the fresh build\n", what);
  return ok;
}

bool set(rtx::FlatScene* fs, const std::vector<int32_t>& ids, const std::vector<double>& vals, rtx_status want = RTX_OK) {
  std::string err;
  const rtx_status st = rtx::flat_set_rects("check", fs, ids.data(), (int64_t)ids.size(), vals.data(), &err);
  if (st != want) { fprintf(stderr, "flat_set_rects: status %d, expected %d (%s)\n", (int)st, (int)want, err.c_str()); return false; }
  return true;
}
}  // namespace

int main() {
  const Moved none = [](int) { return false; }, all = [](int) { return true; };
  Built B0, B1;
  rtx::FlatScene rest, fresh;
  if (!flatten(none, &B0, &rest) || !flatten(all, &B1, &fresh)) return 1;
  const rtx::FlatScene first = rest;
  std::vector<int32_t> ids;
  std::vector<double> vals;
  // the whole update, and back
  if (!update_for(B0, rest, all, true, &ids, &vals) || ids.size() != rest.rects.size() || !set(&rest, ids, vals) || !same_derived(rest, fresh, "full update")) return 1;
  if (same(rest.nodes, first.nodes)) { fprintf(stderr, "the update left every node as it was\n"); return 1; }
  if (!update_for(B0, rest, all, false, &ids, &vals) || !set(&rest, ids, vals) || !same_arrays(rest, first, "back at rest")) return 1;
  // partial: parts = 1 mod 3 against the world built with just those moved; then the rest of them in a second call
  const Moved some = [](int k) { return k % 3 == 1; }, others = [](int k) { return k % 3 != 1; };
  Built B2;
  rtx::FlatScene partial;
  if (!flatten(some, &B2, &partial)) return 1;
  if (!update_for(B0, rest, some, true, &ids, &vals) || !set(&rest, ids, vals) || !same_derived(rest, partial, "partial update")) return 1;
  if (!update_for(B0, rest, others, true, &ids, &vals) || !set(&rest, ids, vals) || !same_derived(rest, fresh, "second half")) return 1;
  // after rtx_flat_set_transforms of a member: the same ops on the fresh scene, then the way back through set_rects
  int32_t slot = -1;
  for (size_t k = 0; k < rest.top_level.size() && slot < 0; ++k)
    if (rest.entries[(size_t)rest.top_level[k]].kind == rt::ENTRY_XFORM && rest.entries[(size_t)rest.top_level[k]].b == 2) slot = (int32_t)k;
  RtxSlotOps ops;
  memset(&ops, 0, sizeof(ops));
  ops.slot = slot; ops.n_ops = 2;
  ops.ops[0].op = 0; ops.ops[0].v[0] = 0.9; ops.ops[0].v[1] = 0.4; ops.ops[0].v[2] = 1.3;
  ops.ops[1].op = 1; ops.ops[1].v[0] = 33.0;
  std::string err;
  if (slot < 0 || !rtx::flat_set_transforms("check", &rest, &ops, 1, &err) || !rtx::flat_set_transforms("check", &fresh, &ops, 1, &err)) { fprintf(stderr, "set_transforms: %s\n", err.c_str()); return 1; }
  if (!update_for(B0, rest, all, false, &ids, &vals) || !set(&rest, ids, vals)) return 1;
  if (!update_for(B0, rest, all, true, &ids, &vals) || !set(&rest, ids, vals) || !same_derived(rest, fresh, "after set_transforms")) return 1;
  // refusals: each leaves the scene as it is
  const rtx::FlatScene before = rest;
  const double nan = std::nan(""), good[10] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10}, bad[10] = {1, 2, 3, 4, 5, 6, 7, nan, 9, 10};
  const int32_t two[2] = {0, 1}, twice[2] = {1, 1}, past[2] = {0, (int32_t)rest.rects.size()}, neg[2] = {-1, 0};
  struct { const int32_t* ids; int64_t n; const double* v; } calls[] = {{nullptr, 2, good}, {two, 2, nullptr}, {two, -1, good}, {twice, 2, good}, {past, 2, good}, {neg, 2, good}, {two, 2, bad}};
  for (const auto& c : calls) {
    err.clear();
    if (rtx::flat_set_rects("check", &rest, c.ids, c.n, c.v, &err) != RTX_EINVAL || err.empty() || !same_arrays(rest, before, "a refusal")) { fprintf(stderr, "a refusal went through\n"); return 1; }
  }
  if (rtx::flat_set_rects("check", nullptr, two, 2, good, &err) != RTX_EINVAL || rtx::flat_set_rects("check", &rest, two, 0, good, &err) != RTX_OK || !same_arrays(rest, before, "n = 0")) return 1;
  // a BVH that holds a MovingSphere refuses its rectangle, alone and among good ids
  Built B3;
  rtx::FlatScene timed;
  if (!flatten(none, &B3, &timed, true)) return 1;
  const rtx::FlatScene timed_before = timed;
  int32_t tid = -1;
  if (rtx::flat_rect_ids("ids", timed, B3.g, B3.timed_rect, &tid, 1, &err) != 1) return 1;
  if (!update_for(B3, timed, all, true, &ids, &vals)) return 1;
  if (!set(&timed, {tid}, {0.9, 1.7, 6.0, 6.8, 1.5}, RTX_EUNSUPPORTED)) return 1;
  std::vector<int32_t> ids2 = ids;
  std::vector<double> vals2 = vals;
  ids2.push_back(tid);
  vals2.insert(vals2.end(), {0.9, 1.7, 6.0, 6.8, 1.5});
  if (!set(&timed, ids2, vals2, RTX_EUNSUPPORTED) || !same_arrays(timed, timed_before, "the timed BVH")) return 1;
  if (!set(&timed, ids, vals) || same(timed.rects, timed_before.rects)) return 1;
  printf("set_rects host check clean\n");
  return 0;
}
