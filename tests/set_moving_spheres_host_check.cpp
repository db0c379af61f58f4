// Host checker of rtx_flat_set_moving_spheres (tests/test_set_moving_spheres_host.py builds it with the product's host sources,
// plain and under -fsanitize=address,undefined, and runs it).  A CPU program with its own main; nothing of it is loaded into Python.
// Worlds: `field`: one BVH of movers and static spheres with an ordered interval, beside a second timed BVH no update names;
// `leaf4`: the same under max_leaf 4, so that a leaf holds static spheres and movers; `unordered`: a BVH whose interval is
// reversed beside an ordered one (it gets the static copy); `plain`: movers as slots of the world list.  Each is built at rest,
// updated with full and partial updates and judged two ways: against the world flattened from scratch with those values (byte
// for byte where the builder chose the same topology), and by restating the flattener's TOP-DOWN rule on the updated topology --
// the union over the interval for `nodes`, the two end unions, the margin and the narrowing for every `motion32` record -- bit
// for bit.  Moved back, every array must be what it was.  Then the refusals, each of which must leave the scene untouched
// (a BVH with a GravitySphere among them), and a BVH whose root is a leaf code (made by hand: no builder emits one).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "../ray-tracing-series-rust_amd/csrc/host/set_triangles.hpp"

namespace rtx {
// the GPU builder lives in csrc/hip/lbvh.hip: not part of a CPU-only program
int32_t build_bvh_gpu(const std::vector<double>&, int, std::vector<rt::FlatNode>*, std::vector<uint32_t>*, int32_t*, double*, std::string* err) {
  if (err) *err = "no GPU builder in the sanitizer program";
  return -1;
}
}  // namespace rtx

namespace {
struct Val { double v[7]; };
typedef std::function<bool(int)> Moved;  // does the k-th updatable mover (in creation order) take its moved values?

// small nudges, each end on its own, and a radius within a few per cent: the builder mostly keeps its topology
Val moved_of(const Val& s, int k) {
  Val o = s;
  for (int a = 0; a < 6; ++a) o.v[a] += (a % 2 ? -1.0 : 1.0) * (0.011 + 0.0017 * k + 0.0031 * a);
  o.v[6] *= k % 2 ? 0.95 : 1.06;
  return o;
}

struct Built {
  rtx::SceneGraph g{5};
  int32_t world = -1;
  std::vector<int32_t> handle;  // per updatable mover, in creation order
  std::vector<Val> rest, moved;
};

struct Maker {
  Built* B;
  Moved on;
  int32_t mover(double x, double y, double z, double dx, double dy, double dz, double r, double t0, double t1, int32_t mat) {
    const Val s = {{x, y, z, x + dx, y + dy, z + dz, r}};
    const int k = (int)B->handle.size();
    const Val m = moved_of(s, k);
    const Val& use = on(k) ? m : s;
    const int32_t h = B->g.moving_sphere(use.v, use.v + 3, t0, t1, use.v[6], mat);
    B->handle.push_back(h);
    B->rest.push_back(s);
    B->moved.push_back(m);
    return h;
  }
  int32_t list(const std::vector<int32_t>& o) { const int32_t l = B->g.list_new(); for (int32_t x : o) B->g.list_add(l, x); return l; }
  std::vector<int32_t> movers(int n, double x0, double y0, double z0, double t0, double t1, int32_t mat) {
    std::vector<int32_t> out;
    for (int k = 0; k < n; ++k)
      out.push_back(mover(x0 + 0.83 * (k % 4) + 0.017 * k, y0 + 0.041 * k, z0 + 0.79 * (k / 4) + 0.013 * k, 0.11 * (k % 3), 0.31 + 0.02 * k, -0.07 * (k % 2),
                          0.21 + 0.019 * (k % 5), t0, t1, mat));
    return out;
  }
};

void make_world(Built* B, const std::string& name, const Moved& on) {
  rtx::SceneGraph& g = B->g;
  Maker m{B, on};
  const double c1[3] = {0.5, 0.5, 0.5}, c2[3] = {0.8, 0.8, 0.9};
  const int32_t grey = g.lambertian(g.solid_color(c1)), metal = g.metal(c2, 0.2);
  auto fixed = [&](double x, double y, double z, double r, int32_t mat) { const double c[3] = {x, y, z}; return g.sphere(c, r, mat); };
  const int32_t ground = fixed(2.0, -500.0, 2.0, 500.0, grey);
  const double a[3] = {6.0, 3.0, -2.0}, b[3] = {6.0, 3.6, -2.2};
  const int32_t other = g.bvh_from_list(m.list({g.moving_sphere(a, b, 0.0, 1.0, 0.3, grey), fixed(7.0, 3.0, -2.0, 0.3, grey), fixed(7.5, 2.0, -1.0, 0.2, metal)}), 0.0, 1.0);
  if (name == "field" || name == "leaf4") {
    std::vector<int32_t> o = m.movers(11, 0.5, 0.8, 0.6, 0.0, 1.0, grey);
    o.push_back(fixed(1.1, 2.4, 1.3, 0.4, metal));
    o.push_back(fixed(2.9, 1.9, 0.4, 0.3, grey));
    o.push_back(m.mover(3.3, 2.2, 2.1, 0.2, 0.1, 0.3, 0.3, 0.25, 0.5, metal));  // its own interval nested in the BVH's
    o.push_back(m.mover(0.3, 2.1, 2.7, 0.1, 0.4, 0.0, 0.25, 1.0, 0.0, metal));  // ... and reversed
    B->world = m.list({ground, g.bvh_from_list(m.list(o), 0.0, 1.0), other});
  } else if (name == "unordered") {
    B->world = m.list({ground, g.bvh_from_list(m.list(m.movers(6, 0.5, 0.8, 0.6, 0.0, 1.0, grey)), 1.0, 0.0), other});
  } else if (name == "plain") {
    std::vector<int32_t> o = m.movers(3, 0.5, 0.8, 0.6, 0.0, 1.0, grey);
    o.push_back(ground);
    B->world = m.list(o);
  } else if (name == "tiny") {  // two movers in one BVH: one node (check_leaf_root turns it into a leaf-code root)
    B->world = m.list({ground, g.bvh_from_list(m.list(m.movers(2, 0.5, 0.8, 0.6, 0.0, 1.0, grey)), 0.0, 1.0)});
  } else {  // gravity: the refusal
    std::vector<int32_t> o = m.movers(3, 0.5, 0.8, 0.6, 0.0, 1.0, grey);
    const double s[3] = {2.0, 3.0, 1.0};
    o.push_back(g.gravity_sphere(s, 0.0, 0.3, grey));
    B->world = m.list({ground, g.bvh_from_list(m.list(o), 0.0, 1.0), g.bvh_from_list(m.list(m.movers(3, 4.5, 0.8, 0.6, 0.0, 1.0, metal)), 0.0, 1.0)});
  }
}

bool flatten(const std::string& name, const Moved& on, Built* B, rtx::FlatScene* fs) {
  make_world(B, name, on);
  if (B->world < 0) { fprintf(stderr, "%s: the graph was refused: %s\n", name.c_str(), B->g.error.c_str()); return false; }
  std::string err;
  rtx::BuildOptions bo;
  if (name == "leaf4") bo.max_leaf = 4;
  if (!rtx::flatten_scene(B->g, B->world, bo, fs, &err)) { fprintf(stderr, "flatten: %s\n", err.c_str()); return false; }
  return true;
}

void update_for(const Built& B, const rtx::FlatScene& fs, const Moved& pick, bool to_moved, std::vector<int32_t>* ids, std::vector<double>* vals) {
  ids->clear(); vals->clear();
  for (size_t k = 0; k < B.handle.size(); ++k) {
    if (!pick((int)k)) continue;
    ids->push_back(fs.handle_moving_sphere_id[(size_t)B.handle[k]]);
    const Val& s = to_moved ? B.moved[k] : B.rest[k];
    vals->insert(vals->end(), s.v, s.v + 7);
  }
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }
bool same_arrays(const rtx::FlatScene& a, const rtx::FlatScene& b, const char* what) {
  const bool ok = same(a.triangles, b.triangles) && same(a.entries, b.entries) && same(a.top_level, b.top_level) && same(a.nodes, b.nodes) &&
                  same(a.nodes32, b.nodes32) && same(a.motion32, b.motion32) && same(a.member_local_box, b.member_local_box) && same(a.refs, b.refs) &&
                  same(a.rects, b.rects) && same(a.spheres, b.spheres) && same(a.moving_spheres, b.moving_spheres) && same(a.top_box32, b.top_box32) &&
                  same(a.handle_moving_sphere_id, b.handle_moving_sphere_id);
  if (!ok) fprintf(stderr, "%s: the arrays differ\n", what);
  return ok;
}

// ---- the flattener's top-down rule, written out again here so that the bottom-up refit is not judged by its own arithmetic
struct Box6 { double b[6]; };
Box6 prim_box_at(const rtx::FlatScene& fs, rt::PrimRef ref, double ta, double tb) {
  Box6 o;
  const uint32_t i = rt::primref_index(ref);
  if (rt::primref_type(ref) == rt::PRIM_SPHERE) {
    const rt::FlatSphere& s = fs.spheres[i];
    const double c[3] = {s.cx, s.cy, s.cz}, r = std::fabs(s.radius);
    for (int a = 0; a < 3; ++a) { o.b[a] = c[a] - r; o.b[3 + a] = c[a] + r; }
    return o;
  }
  const rt::FlatMovingSphere& s = fs.moving_spheres[i];
  const double r = std::fabs(s.radius), ka = (ta - s.time0) / (s.time1 - s.time0), kb = (tb - s.time0) / (s.time1 - s.time0);
  for (int a = 0; a < 3; ++a) {
    const double ca = s.c0[a] + ka * (s.c1[a] - s.c0[a]), cb = s.c0[a] + kb * (s.c1[a] - s.c0[a]);
    o.b[a] = std::fmin(ca - r, cb - r); o.b[3 + a] = std::fmax(ca + r, cb + r);
  }
  return o;
}
Box6 box_below(const rtx::FlatScene& fs, const rt::FlatEntry& e, int32_t code, double ta, double tb) {
  Box6 r;
  for (int a = 0; a < 3; ++a) { r.b[a] = HUGE_VAL; r.b[3 + a] = -HUGE_VAL; }
  auto grow = [&](const Box6& k) { for (int a = 0; a < 3; ++a) { r.b[a] = std::fmin(r.b[a], k.b[a]); r.b[3 + a] = std::fmax(r.b[3 + a], k.b[3 + a]); } };
  if (code >= 0) { for (int c = 0; c < 2; ++c) grow(box_below(fs, e, fs.nodes[(size_t)code].child[c], ta, tb)); return r; }
  for (uint32_t i = 0; i < rt::leaf_count(code); ++i) grow(prim_box_at(fs, fs.refs[(size_t)e.b + rt::leaf_first(code) + i], ta, tb));
  return r;
}
float down(double x) { float f = (float)x; return (double)f > x ? std::nextafterf(f, -INFINITY) : f; }
float up(double x) { float f = (float)x; return (double)f < x ? std::nextafterf(f, INFINITY) : f; }

int audit_top_down(const rtx::FlatScene& fs, const char* what) {
  int bad = 0;
  for (const rt::FlatEntry& e : fs.entries) {
    if (e.kind != rt::ENTRY_BVH || e.a < 0) continue;
    bool mover = false, other = false;
    for (int32_t i = 0; i < e.c; ++i) {
      const uint32_t ty = rt::primref_type(fs.refs[(size_t)e.b + i]);
      mover |= ty == rt::PRIM_MOVING_SPHERE;
      other |= ty != rt::PRIM_MOVING_SPHERE && ty != rt::PRIM_SPHERE;
    }
    if (other) continue;
    const bool time_boxes = mover && e.f[0] < e.f[1] && !fs.motion32.empty();
    std::vector<int32_t> todo{e.a};
    while (!todo.empty()) {
      const int32_t n = todo.back();
      todo.pop_back();
      const rt::FlatNode& nd = fs.nodes[(size_t)n];
      for (int c = 0; c < 2; ++c) {
        if (nd.child[c] >= 0) todo.push_back(nd.child[c]);
        const Box6 u = box_below(fs, e, nd.child[c], e.f[0], e.f[1]);
        if (memcmp(u.b, nd.bmin[c], 24) != 0 || memcmp(u.b + 3, nd.bmax[c], 24) != 0) { fprintf(stderr, "%s: node %d child %d is not the union over the interval\n", what, n, c); ++bad; }
        if (fs.motion32.empty()) continue;
        float want[4][3];  // lo0, hi0, dlo, dhi
        if (time_boxes) {
          const Box6 b0 = box_below(fs, e, nd.child[c], e.f[0], e.f[0]), b1 = box_below(fs, e, nd.child[c], e.f[1], e.f[1]);
          for (int a = 0; a < 3; ++a) {
            const double mag = std::fmax(std::fmax(std::fabs(b0.b[a]), std::fabs(b0.b[3 + a])), std::fmax(std::fabs(b1.b[a]), std::fabs(b1.b[3 + a])));
            const double margin = mag * 0x1.0p-21 + 1e-30;
            const float lo_a = down(b0.b[a] - margin), lo_b = down(b1.b[a] - margin), hi_a = up(b0.b[3 + a] + margin), hi_b = up(b1.b[3 + a] + margin);
            want[0][a] = lo_a; want[1][a] = hi_a; want[2][a] = lo_b - lo_a; want[3][a] = hi_b - hi_a;
          }
        } else {
          for (int a = 0; a < 3; ++a) { want[0][a] = down(nd.bmin[c][a]); want[1][a] = up(nd.bmax[c][a]); want[2][a] = 0.0f; want[3][a] = 0.0f; }
        }
        const rt::FlatMotion32& m = fs.motion32[(size_t)n];
        if (memcmp(want[0], m.lo0[c], 12) != 0 || memcmp(want[1], m.hi0[c], 12) != 0 || memcmp(want[2], m.dlo[c], 12) != 0 || memcmp(want[3], m.dhi[c], 12) != 0) {
          fprintf(stderr, "%s: motion32[%d] child %d is not what the top-down rule gives\n", what, n, c);
          ++bad;
        }
      }
    }
  }
  return bad;
}

int against_fresh(const rtx::FlatScene& got, const rtx::FlatScene& fresh, const rtx::FlatScene& first, const char* what, int* same_topo) {
  int bad = audit_top_down(got, what);
  if (!same(got.moving_spheres, fresh.moving_spheres)) { fprintf(stderr, "%s: the movers differ from the fresh ones\n", what); ++bad; }
  if (!same(got.entries, first.entries) || !same(got.refs, first.refs) || !same(got.top_level, first.top_level) || !same(got.spheres, first.spheres) ||
      !same(got.top_box32, first.top_box32)) { fprintf(stderr, "%s: entries / refs / top_level / spheres / top_box32 changed\n", what); ++bad; }
  for (size_t n = 0; n < got.nodes.size(); ++n) {
    if (memcmp(got.nodes[n].child, first.nodes[n].child, 16) != 0) { fprintf(stderr, "%s: node %zu's topology changed\n", what, n); ++bad; }
    for (int c = 0; c < 2; ++c)
      for (int a = 0; a < 3; ++a)
        if (got.nodes32[n].lo[c][a] != rt::f32_narrow_down(got.nodes[n].bmin[c][a]) || got.nodes32[n].hi[c][a] != rt::f32_narrow_up(got.nodes[n].bmax[c][a])) { fprintf(stderr, "%s: nodes32[%zu] is not the narrowing of nodes\n", what, n); ++bad; }
  }
  bool same_topology = got.nodes.size() == fresh.nodes.size() && same(got.refs, fresh.refs);
  for (size_t n = 0; same_topology && n < got.nodes.size(); ++n) same_topology = memcmp(got.nodes[n].child, fresh.nodes[n].child, 16) == 0;
  if (same_topology) {
    ++*same_topo;
    if (!same(got.nodes, fresh.nodes) || !same(got.nodes32, fresh.nodes32) || !same(got.motion32, fresh.motion32)) { fprintf(stderr, "%s: same topology as the fresh scene, other boxes\n", what); ++bad; }
  } else {
    printf("%s: the fresh flatten chose another topology (boxes compared through the top-down rule only)\n", what);
  }
  return bad;
}

int check_world(const std::string& name) {
  int bad = 0, same_topo = 0;
  const Moved none = [](int) { return false; }, all = [](int) { return true; };
  Built B0;
  rtx::FlatScene fs;
  if (!flatten(name, none, &B0, &fs)) return 1;
  const rtx::FlatScene first = fs;
  bad += audit_top_down(first, (name + " at rest (the checker's own rule against the flattener)").c_str());
  const int n_mov = (int)B0.handle.size();
  const std::vector<Moved> picks = {all, [](int k) { return k == 0; }, [](int k) { return k % 5 == 0; }, [n_mov](int k) { return k >= n_mov / 2; }};
  std::vector<int32_t> ids;
  std::vector<double> vals;
  std::string err;
  for (size_t p = 0; p < picks.size(); ++p) {
    Built Bf;
    rtx::FlatScene fresh;
    if (!flatten(name, picks[p], &Bf, &fresh)) return 1;
    update_for(B0, fs, picks[p], true, &ids, &vals);
    if (rtx::flat_set_moving_spheres("check", &fs, ids.data(), (int64_t)ids.size(), vals.data(), &err) != RTX_OK) { fprintf(stderr, "%s: update %zu refused: %s\n", name.c_str(), p, err.c_str()); return 1; }
    if (same(fs.moving_spheres, first.moving_spheres)) { fprintf(stderr, "%s: update %zu moved no mover\n", name.c_str(), p); ++bad; }
    if (name != "plain" && same(fs.nodes, first.nodes)) { fprintf(stderr, "%s: update %zu refitted nothing\n", name.c_str(), p); ++bad; }
    bad += against_fresh(fs, fresh, first, (name + " update " + std::to_string(p)).c_str(), &same_topo);
    update_for(B0, fs, picks[p], false, &ids, &vals);
    if (rtx::flat_set_moving_spheres("check", &fs, ids.data(), (int64_t)ids.size(), vals.data(), &err) != RTX_OK) { fprintf(stderr, "%s: way back %zu refused: %s\n", name.c_str(), p, err.c_str()); return 1; }
    if (!same_arrays(fs, first, (name + " back at rest").c_str())) ++bad;
  }
  if (same_topo == 0) { fprintf(stderr, "%s: no update kept the fresh build's topology: nothing was compared byte for byte\n", name.c_str()); ++bad; }
  printf("%s: %d updatable movers, %zu flat, %zu nodes, %zu time-aware records: %d faults\n", name.c_str(), n_mov, fs.moving_spheres.size(), fs.nodes.size(),
         fs.motion32.size(), bad);
  return bad;
}

int check_refusals() {
  int bad = 0;
  Built B;
  rtx::FlatScene fs;
  if (!flatten("gravity", [](int) { return false; }, &B, &fs)) return 1;
  const rtx::FlatScene first = fs;
  const double nan = std::nan(""), inf = HUGE_VAL;
  std::vector<double> good(14, 1.5), with_nan = good, with_inf = good;
  with_nan[9] = nan; with_inf[6] = inf;
  const int32_t n_ids = (int32_t)fs.moving_spheres.size();
  struct Case { const char* name; std::vector<int32_t> ids; int64_t n; const double* v; bool null_ids; const char* word; };
  const std::vector<Case> cases = {
      {"null ids", {3, 4}, 2, good.data(), true, "ids is NULL"},          {"null movers", {3, 4}, 2, nullptr, false, "movers is NULL"},
      {"negative n", {3, 4}, -1, good.data(), false, "n < 0"},            {"id negative", {3, -1}, 2, good.data(), false, "ids[1] is out of range"},
      {"id past the end", {n_ids, 4}, 2, good.data(), false, "ids[0] is out of range"}, {"id named twice", {4, 4}, 2, good.data(), false, "twice"},
      {"NaN centre", {3, 4}, 2, with_nan.data(), false, "movers[1][2] is not finite"}, {"infinite radius", {3, 4}, 2, with_inf.data(), false, "movers[0][6] is not finite"},
  };
  for (const Case& c : cases) {
    std::string err;
    const rtx_status st = rtx::flat_set_moving_spheres("check", &fs, c.null_ids ? nullptr : c.ids.data(), c.n, c.v, &err);
    if (st != RTX_EINVAL || err.find(c.word) == std::string::npos) { fprintf(stderr, "refusal '%s': status %d, message '%s'\n", c.name, (int)st, err.c_str()); ++bad; }
    if (!same_arrays(fs, first, c.name)) ++bad;
  }
  std::string err;
  if (rtx::flat_set_moving_spheres("check", nullptr, cases[0].ids.data(), 2, good.data(), &err) != RTX_EINVAL || err.find("scene is NULL") == std::string::npos) { fprintf(stderr, "NULL scene accepted\n"); ++bad; }
  if (rtx::flat_set_moving_spheres("check", &fs, cases[0].ids.data(), 0, good.data(), &err) != RTX_OK || !same_arrays(fs, first, "n = 0")) { fprintf(stderr, "n = 0 did something\n"); ++bad; }
  // movers 0..2 share their BVH with a GravitySphere: refused, also among good ids; movers 3..5 (a BVH of their own) still update
  const int32_t in_gravity = fs.handle_moving_sphere_id[(size_t)B.handle[0]], clean = fs.handle_moving_sphere_id[(size_t)B.handle[3]];
  const int32_t mixed_ids[2] = {clean, in_gravity};
  if (rtx::flat_set_moving_spheres("check", &fs, &in_gravity, 1, good.data(), &err) != RTX_EUNSUPPORTED || err.find("GravitySphere") == std::string::npos ||
      err.find("not linear in time") == std::string::npos) { fprintf(stderr, "gravity BVH accepted: %s\n", err.c_str()); ++bad; }
  if (rtx::flat_set_moving_spheres("check", &fs, mixed_ids, 2, good.data(), &err) != RTX_EUNSUPPORTED) { fprintf(stderr, "gravity BVH accepted among good ids\n"); ++bad; }
  if (!same_arrays(fs, first, "gravity")) ++bad;
  if (rtx::flat_set_moving_spheres("check", &fs, &clean, 1, B.moved[3].v, &err) != RTX_OK || same(fs.nodes, first.nodes)) { fprintf(stderr, "the BVH beside the gravity one did not update: %s\n", err.c_str()); ++bad; }
  // a BVH that holds a mover is still refused by the updates of STATIC primitives
  const int32_t sphere0 = 0;
  Built Bf;
  rtx::FlatScene field;
  if (!flatten("field", [](int) { return false; }, &Bf, &field)) return 1;
  const int32_t static_in_timed = (int32_t)field.spheres.size() - 3;  // (ground, then the field's two static spheres, then `other`'s two)
  (void)sphere0;
  if (rtx::flat_set_spheres("check", &field, &static_in_timed, 1, good.data(), &err) != RTX_EUNSUPPORTED || err.find("MovingSphere") == std::string::npos) { fprintf(stderr, "set_spheres took a timed BVH: %s\n", err.c_str()); ++bad; }
  printf("refusals: %d faults\n", bad);
  return bad;
}

// A BVH whose root is a LEAF CODE has no node.  The flattener's builders always emit a node, so the shape is made by hand: the
// one node of a two-mover BVH is dropped and the entry names the leaf of both.  An update then changes the records and nothing else.
int check_leaf_root() {
  int bad = 0;
  Built B, Bf;
  rtx::FlatScene fs, fresh;
  if (!flatten("tiny", [](int) { return false; }, &B, &fs) || !flatten("tiny", [](int) { return true; }, &Bf, &fresh)) return 1;
  if (fs.nodes.size() != 1) { fprintf(stderr, "leaf root: the two-mover BVH has %zu nodes, not 1\n", fs.nodes.size()); return 1; }
  for (rt::FlatEntry& e : fs.entries)
    if (e.kind == rt::ENTRY_BVH) e.a = rt::make_leaf(0, 2);
  fs.nodes.clear(); fs.nodes32.clear(); fs.motion32.clear();
  const rtx::FlatScene first = fs;
  const rtx::MeshShadow sh = rtx::build_mesh_shadow(fs, rtx::build_update_shadow(fs));
  if (!sh.broken.empty() || sh.bvhs.size() != 1 || sh.bvhs[0].n_nodes != 0 || sh.bvhs[0].time_boxes != 0 || !sh.bvhs[0].has_mover) { fprintf(stderr, "leaf root: shadow '%s'\n", sh.broken.c_str()); ++bad; }
  std::vector<int32_t> ids;
  std::vector<double> vals;
  std::string err;
  update_for(B, fs, [](int) { return true; }, true, &ids, &vals);
  if (rtx::flat_set_moving_spheres("check", &fs, ids.data(), (int64_t)ids.size(), vals.data(), &err) != RTX_OK) { fprintf(stderr, "leaf root: refused: %s\n", err.c_str()); return 1; }
  if (!same(fs.moving_spheres, fresh.moving_spheres) || same(fs.moving_spheres, first.moving_spheres)) { fprintf(stderr, "leaf root: the movers are not the fresh ones\n"); ++bad; }
  if (!same(fs.entries, first.entries) || !same(fs.refs, first.refs) || !fs.nodes.empty()) { fprintf(stderr, "leaf root: more than the movers changed\n"); ++bad; }
  printf("leaf-code root: %d faults\n", bad);
  return bad;
}
}  // namespace

int main() {
  int bad = 0;
  for (const char* name : {"field", "leaf4", "unordered", "plain"}) bad += check_world(name);
  bad += check_refusals();
  bad += check_leaf_root();
  if (bad) { printf("set_moving_spheres host check: %d faults\n", bad); return 1; }
  printf("set_moving_spheres host check clean\n");
  return 0;
}
