// Host checker of rtx_flat_set_spheres (tests/test_set_spheres_host.py builds it with the product's host sources under
// -fsanitize=address,undefined and runs it).  A CPU program with its own main; nothing of it is loaded into Python.
// Worlds: `field`: one BVH of static spheres (one of negative radius) and a ground, beside a BVH of moving spheres so that the
// time-aware boxes exist; `lamp`: a top-level sphere light with a checker emission next to a rectangle light and plain spheres,
// and a medium around a sphere; `instanced`: an instance tree whose members are a sphere, a group of spheres and a BVH of
// spheres.  Each is built at rest, updated with full and partial updates and compared with the world flattened from scratch
// with those values (the light table included); moved back, every array must be what it was.  Then the refusals, each of which
// must leave the scene untouched, and a BVH whose root is a leaf code (made by hand: no builder emits one).
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
struct Val { double v[4]; };
typedef std::function<bool(int)> Moved;  // does the k-th movable sphere (in creation order) take its moved values?

// k % 3 == 0: the sphere leaves its old box (2.6 |r| along x); 1: it shrinks; 2: it grows.  Irrational-looking factors keep
// every plane away from a tie.
Val moved_of(const Val& s, int k) {
  Val o = s;
  const double r = std::fabs(s.v[3]);
  if (k % 3 == 0) { o.v[0] += 2.6 * r + 0.0137 * k; o.v[1] += 0.11 * r; }
  else if (k % 3 == 1) { o.v[3] *= 0.57; o.v[2] += 0.13 * r; }
  else { o.v[3] *= 1.37; o.v[0] -= 0.09 * r; }
  return o;
}

struct Built {
  rtx::SceneGraph g{5};
  int32_t world = -1;
  std::vector<int32_t> handle;  // per movable sphere, in creation order
  std::vector<Val> rest, moved;
};

struct Maker {
  Built* B;
  Moved on;
  int32_t sphere(double x, double y, double z, double r, int32_t mat) {
    const Val s = {{x, y, z, r}};
    const int k = (int)B->handle.size();
    const Val m = moved_of(s, k);
    const Val& use = on(k) ? m : s;
    const int32_t h = B->g.sphere(use.v, use.v[3], mat);
    B->handle.push_back(h);
    B->rest.push_back(s);
    B->moved.push_back(m);
    return h;
  }
  int32_t list(const std::vector<int32_t>& o) { const int32_t l = B->g.list_new(); for (int32_t x : o) B->g.list_add(l, x); return l; }
  std::vector<int32_t> spheres(int n, double x0, double y0, double z0, int32_t mat) {
    std::vector<int32_t> out;
    for (int k = 0; k < n; ++k) out.push_back(sphere(x0 + 0.83 * (k % 4) + 0.017 * k, y0 + 0.041 * k, z0 + 0.79 * (k / 4) + 0.013 * k, 0.21 + 0.019 * (k % 5), mat));
    return out;
  }
};

void make_world(Built* B, const std::string& name, const Moved& on) {
  rtx::SceneGraph& g = B->g;
  Maker m{B, on};
  const double c1[3] = {0.5, 0.5, 0.5}, c2[3] = {0.8, 0.8, 0.9}, bright[3] = {6.0, 5.0, 4.0}, black[3] = {0.0, 0.0, 0.0}, solid[3] = {4.0, 4.0, 4.0};
  const int32_t grey = g.lambertian(g.solid_color(c1)), metal = g.metal(c2, 0.2), glass = g.dielectric(1.5);
  auto fixed = [&](double x, double y, double z, double r, int32_t mat) { const double c[3] = {x, y, z}; return g.sphere(c, r, mat); };
  const int32_t ground = fixed(2.0, -500.0, 2.0, 500.0, grey);
  if (name == "field") {
    std::vector<int32_t> o = m.spheres(13, 0.5, 0.8, 0.6, grey);
    o.push_back(m.sphere(1.0, 2.6, 1.2, 0.45, glass));
    o.push_back(m.sphere(1.0, 2.6, 1.2, -0.4, glass));
    o.push_back(ground);
    const double a[3] = {3.0, 3.0, -2.0}, b[3] = {3.0, 3.6, -2.0};
    const int32_t movers = g.bvh_from_list(m.list({g.moving_sphere(a, b, 0.0, 1.0, 0.3, grey), fixed(5.0, 3.0, -2.0, 0.3, grey)}), 0.0, 1.0);
    B->world = m.list({g.bvh_from_list(m.list(o), 0.0, 1.0), movers});
  } else if (name == "lamp") {
    const int32_t emit = g.checker(g.solid_color(bright), g.solid_color(black));
    const int32_t light = m.sphere(2.05, 2.6, 2.05, 0.4, g.diffuse_light(emit));  // k = 0: it moves 1.04 + along x, into other cells
    const int32_t rect = g.rect(rtx::H_XZ_RECT, 2.9, 4.1, 1.95, 3.15, 3.1, g.diffuse_light(g.solid_color(solid)));
    const int32_t inside = m.sphere(4.6, 1.2, 4.4, 0.9, glass);
    B->world = m.list({ground, light, rect, m.sphere(0.9, 0.6, 0.8, 0.5, metal), m.sphere(3.3, 0.7, 0.9, 0.6, grey), g.constant_medium(c2, 0.7, inside)});
  } else if (name == "instanced") {
    const double t0[3] = {0.4, 0.2, 0.3}, t1[3] = {3.1, 0.3, 2.2}, t2[3] = {1.2, 0.4, 4.0};
    const int32_t a = g.translate(t0, g.rotate_y(20.0, g.bvh_from_list(m.list(m.spheres(9, 0.2, 0.8, 0.3, grey)), 0.0, 1.0)));
    const int32_t b = g.translate(t1, g.rotate_y(-35.0, m.list(m.spheres(3, 0.2, 0.5, 0.3, metal))));
    const int32_t c = g.translate(t2, m.sphere(0.4, 0.7, 0.5, 0.35, glass));
    B->world = m.list({ground, g.instance_bvh_from_list(m.list({a, b, c}))});
  } else if (name == "tiny") {  // two spheres in one BVH: one node (check_leaf_root turns it into a leaf-code root)
    B->world = m.list({ground, g.bvh_from_list(m.list(m.spheres(2, 0.5, 0.8, 0.6, grey)), 0.0, 1.0)});
  } else {  // movers: the refusal
    std::vector<int32_t> o = m.spheres(5, 0.5, 0.8, 0.6, grey);
    const double a[3] = {1.0, 2.5, 1.0}, b[3] = {1.0, 3.0, 1.0};
    o.push_back(g.moving_sphere(a, b, 0.0, 1.0, 0.3, grey));
    B->world = m.list({ground, g.bvh_from_list(m.list(o), 0.0, 1.0)});
  }
}

bool flatten(const std::string& name, const Moved& on, Built* B, rtx::FlatScene* fs) {
  make_world(B, name, on);
  if (B->world < 0) { fprintf(stderr, "%s: the graph was refused: %s\n", name.c_str(), B->g.error.c_str()); return false; }
  std::string err;
  if (!rtx::flatten_scene(B->g, B->world, rtx::BuildOptions(), fs, &err)) { fprintf(stderr, "flatten: %s\n", err.c_str()); return false; }
  return true;
}

// ids and values that give the movable spheres chosen by `pick` the values `to_moved` says (moved or rest)
void update_for(const Built& B, const rtx::FlatScene& fs, const Moved& pick, bool to_moved, std::vector<int32_t>* ids, std::vector<double>* vals) {
  ids->clear(); vals->clear();
  for (size_t k = 0; k < B.handle.size(); ++k) {
    if (!pick((int)k)) continue;
    ids->push_back(fs.handle_sphere_id[(size_t)B.handle[k]]);
    const Val& s = to_moved ? B.moved[k] : B.rest[k];
    vals->insert(vals->end(), s.v, s.v + 4);
  }
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }
bool same_arrays(const rtx::FlatScene& a, const rtx::FlatScene& b, const char* what) {
  const bool ok = same(a.triangles, b.triangles) && same(a.entries, b.entries) && same(a.top_level, b.top_level) && same(a.nodes, b.nodes) &&
                  same(a.nodes32, b.nodes32) && same(a.motion32, b.motion32) && same(a.member_local_box, b.member_local_box) && same(a.refs, b.refs) &&
                  same(a.rects, b.rects) && same(a.spheres, b.spheres) && same(a.top_box32, b.top_box32) && same(a.handle_sphere_id, b.handle_sphere_id);
  if (!ok) fprintf(stderr, "%s: the arrays differ\n", what);
  return ok;
}

// The checker's own box of everything below child code `code` of BVH entry e (static spheres only), written out again here so
// that the refit is not judged by its own arithmetic.
struct Box6 { double lo[3], hi[3]; };
Box6 box_below(const rtx::FlatScene& fs, const rt::FlatEntry& e, int32_t code) {
  Box6 b;
  for (int a = 0; a < 3; ++a) { b.lo[a] = HUGE_VAL; b.hi[a] = -HUGE_VAL; }
  if (code >= 0) {
    for (int c = 0; c < 2; ++c) {
      const Box6 k = box_below(fs, e, fs.nodes[(size_t)code].child[c]);
      for (int a = 0; a < 3; ++a) { b.lo[a] = std::fmin(b.lo[a], k.lo[a]); b.hi[a] = std::fmax(b.hi[a], k.hi[a]); }
    }
    return b;
  }
  for (uint32_t i = 0; i < rt::leaf_count(code); ++i) {
    const rt::FlatSphere& s = fs.spheres[rt::primref_index(fs.refs[(size_t)e.b + rt::leaf_first(code) + i])];
    const double c[3] = {s.cx, s.cy, s.cz};
    for (int a = 0; a < 3; ++a) { b.lo[a] = std::fmin(b.lo[a], c[a] - std::fabs(s.radius)); b.hi[a] = std::fmax(b.hi[a], c[a] + std::fabs(s.radius)); }
  }
  return b;
}
int audit_boxes(const rtx::FlatScene& fs, const char* what) {
  int bad = 0;
  for (const rt::FlatEntry& e : fs.entries) {
    if (e.kind != rt::ENTRY_BVH || e.a < 0) continue;
    bool timed = false;
    for (int32_t i = 0; i < e.c; ++i) timed |= rt::primref_type(fs.refs[(size_t)e.b + i]) != rt::PRIM_SPHERE;
    if (timed) continue;
    std::vector<int32_t> todo{e.a};
    while (!todo.empty()) {
      const int32_t n = todo.back();
      todo.pop_back();
      for (int c = 0; c < 2; ++c) {
        const Box6 b = box_below(fs, e, fs.nodes[(size_t)n].child[c]);
        if (memcmp(b.lo, fs.nodes[(size_t)n].bmin[c], 24) != 0 || memcmp(b.hi, fs.nodes[(size_t)n].bmax[c], 24) != 0) { fprintf(stderr, "%s: node %d child %d is not the union of what lies below it\n", what, n, c); ++bad; }
        if (fs.nodes[(size_t)n].child[c] >= 0) todo.push_back(fs.nodes[(size_t)n].child[c]);
      }
    }
  }
  return bad;
}

// The updated scene against the one flattened from scratch with those values.  The worlds here are small enough that the
// builder usually picks the same topology for both, and the comparison is then every array byte for byte; where it does not
// (reported), the spheres, the members' local boxes, top_box32 and the light table still have to agree.
int against_fresh(const rtx::FlatScene& got, const rtx::FlatScene& fresh, const rtx::FlatScene& first, const char* what) {
  int bad = audit_boxes(got, what);
  if (!same(got.spheres, fresh.spheres)) { fprintf(stderr, "%s: the spheres differ from the fresh ones\n", what); ++bad; }
  if (!same(got.entries, first.entries) || !same(got.refs, first.refs) || !same(got.top_level, first.top_level)) { fprintf(stderr, "%s: entries / refs / top_level changed\n", what); ++bad; }
  for (size_t n = 0; n < got.nodes.size(); ++n) {
    if (memcmp(got.nodes[n].child, first.nodes[n].child, 16) != 0) { fprintf(stderr, "%s: node %zu's topology changed\n", what, n); ++bad; }
    for (int c = 0; c < 2; ++c)
      for (int a = 0; a < 3; ++a)
        if (got.nodes32[n].lo[c][a] != rt::f32_narrow_down(got.nodes[n].bmin[c][a]) || got.nodes32[n].hi[c][a] != rt::f32_narrow_up(got.nodes[n].bmax[c][a])) { fprintf(stderr, "%s: nodes32[%zu] is not the narrowing of nodes\n", what, n); ++bad; }
  }
  if (!same(got.top_box32, fresh.top_box32)) { fprintf(stderr, "%s: top_box32 differs\n", what); ++bad; }
  if (!same(got.member_local_box, fresh.member_local_box)) { fprintf(stderr, "%s: member_local_box differs\n", what); ++bad; }
  const rtx::LightTable lg = rtx::build_light_table(got), lf = rtx::build_light_table(fresh);
  if (!same(lg.lights, lf.lights) || !same(lg.slot_light, lf.slot_light)) { fprintf(stderr, "%s: the light table differs\n", what); ++bad; }
  bool same_topology = got.nodes.size() == fresh.nodes.size() && same(got.refs, fresh.refs);
  for (size_t n = 0; same_topology && n < got.nodes.size(); ++n) same_topology = memcmp(got.nodes[n].child, fresh.nodes[n].child, 16) == 0;  // children and split axis
  if (same_topology) {
    if (!same(got.nodes, fresh.nodes) || !same(got.nodes32, fresh.nodes32) || !same(got.motion32, fresh.motion32)) { fprintf(stderr, "%s: same topology as the fresh scene, other boxes\n", what); ++bad; }
  } else {
    printf("%s: the fresh flatten chose another topology (boxes compared through the audit and the members only)\n", what);
  }
  return bad;
}

int check_world(const std::string& name) {
  int bad = 0;
  const Moved none = [](int) { return false; }, all = [](int) { return true; };
  Built B0;
  rtx::FlatScene fs;
  if (!flatten(name, none, &B0, &fs)) return 1;
  const rtx::FlatScene first = fs;
  const int n_mov = (int)B0.handle.size();
  const std::vector<Moved> picks = {all, [](int k) { return k == 0; }, [](int k) { return k % 7 == 0; }, [n_mov](int k) { return k >= n_mov / 2; }};
  std::vector<int32_t> ids;
  std::vector<double> vals;
  std::string err;
  for (size_t p = 0; p < picks.size(); ++p) {
    Built Bf;
    rtx::FlatScene fresh;
    if (!flatten(name, picks[p], &Bf, &fresh)) return 1;
    update_for(B0, fs, picks[p], true, &ids, &vals);
    if (rtx::flat_set_spheres("check", &fs, ids.data(), (int64_t)ids.size(), vals.data(), &err) != RTX_OK) { fprintf(stderr, "%s: update %zu refused: %s\n", name.c_str(), p, err.c_str()); return 1; }
    if (same(fs.spheres, first.spheres)) { fprintf(stderr, "%s: update %zu moved no sphere\n", name.c_str(), p); ++bad; }
    bad += against_fresh(fs, fresh, first, (name + " update " + std::to_string(p)).c_str());
    update_for(B0, fs, picks[p], false, &ids, &vals);
    if (rtx::flat_set_spheres("check", &fs, ids.data(), (int64_t)ids.size(), vals.data(), &err) != RTX_OK) { fprintf(stderr, "%s: way back %zu refused: %s\n", name.c_str(), p, err.c_str()); return 1; }
    if (!same_arrays(fs, first, (name + " back at rest").c_str())) ++bad;
  }
  // two updates in a row: first half, second half == all
  Built Bf;
  rtx::FlatScene fresh;
  if (!flatten(name, all, &Bf, &fresh)) return 1;
  for (int half = 0; half < 2; ++half) {
    update_for(B0, fs, [n_mov, half](int k) { return (k < n_mov / 2) == (half == 0); }, true, &ids, &vals);
    if (rtx::flat_set_spheres("check", &fs, ids.data(), (int64_t)ids.size(), vals.data(), &err) != RTX_OK) { fprintf(stderr, "%s: half %d refused: %s\n", name.c_str(), half, err.c_str()); return 1; }
  }
  bad += against_fresh(fs, fresh, first, (name + " two updates in a row").c_str());
  if (name == "lamp") {  // the sphere light moved across checker cells: the table cannot be what it was
    const rtx::LightTable l0 = rtx::build_light_table(first), l1 = rtx::build_light_table(fs);
    if (l0.lights.size() != 2 || same(l0.lights, l1.lights)) { fprintf(stderr, "lamp: the light table did not follow the light\n"); ++bad; }
  }
  printf("%s: %d movable spheres, %zu flat, %zu nodes: %d faults\n", name.c_str(), n_mov, fs.spheres.size(), fs.nodes.size(), bad);
  return bad;
}

int check_refusals() {
  int bad = 0;
  Built B;
  rtx::FlatScene fs;
  if (!flatten("field", [](int) { return false; }, &B, &fs)) return 1;
  const rtx::FlatScene first = fs;
  const double nan = std::nan(""), inf = HUGE_VAL;
  std::vector<double> good(8, 1.5), with_nan = good, with_inf = good;
  with_nan[6] = nan; with_inf[3] = inf;
  const int32_t n_ids = (int32_t)fs.spheres.size();
  struct Case { const char* name; std::vector<int32_t> ids; int64_t n; const double* v; bool null_ids; const char* word; };
  const std::vector<Case> cases = {
      {"null ids", {0, 1}, 2, good.data(), true, "ids is NULL"},          {"null spheres", {0, 1}, 2, nullptr, false, "spheres is NULL"},
      {"negative n", {0, 1}, -1, good.data(), false, "n < 0"},            {"id negative", {0, -1}, 2, good.data(), false, "ids[1] is out of range"},
      {"id past the end", {n_ids, 1}, 2, good.data(), false, "ids[0] is out of range"}, {"id named twice", {1, 1}, 2, good.data(), false, "twice"},
      {"NaN centre", {0, 1}, 2, with_nan.data(), false, "spheres[1][2] is not finite"}, {"infinite radius", {0, 1}, 2, with_inf.data(), false, "spheres[0][3] is not finite"},
  };
  for (const Case& c : cases) {
    std::string err;
    const rtx_status st = rtx::flat_set_spheres("check", &fs, c.null_ids ? nullptr : c.ids.data(), c.n, c.v, &err);
    if (st != RTX_EINVAL || err.find(c.word) == std::string::npos) { fprintf(stderr, "refusal '%s': status %d, message '%s'\n", c.name, (int)st, err.c_str()); ++bad; }
    if (!same_arrays(fs, first, c.name)) ++bad;
  }
  std::string err;
  if (rtx::flat_set_spheres("check", nullptr, cases[0].ids.data(), 2, good.data(), &err) != RTX_EINVAL || err.find("scene is NULL") == std::string::npos) { fprintf(stderr, "NULL scene accepted\n"); ++bad; }
  if (rtx::flat_set_spheres("check", &fs, cases[0].ids.data(), 0, good.data(), &err) != RTX_OK || !same_arrays(fs, first, "n = 0")) { fprintf(stderr, "n = 0 did something\n"); ++bad; }
  // the static sphere inside the BVH that holds a MovingSphere (the last sphere emitted): refused; so is a call that names it among good ids
  const int32_t timed_id = n_ids - 1;
  const int32_t mixed_ids[2] = {0, timed_id};
  if (rtx::flat_set_spheres("check", &fs, &timed_id, 1, good.data(), &err) != RTX_EUNSUPPORTED || err.find("MovingSphere") == std::string::npos) { fprintf(stderr, "timed BVH accepted: %s\n", err.c_str()); ++bad; }
  if (rtx::flat_set_spheres("check", &fs, mixed_ids, 2, good.data(), &err) != RTX_EUNSUPPORTED) { fprintf(stderr, "timed BVH accepted among good ids\n"); ++bad; }
  if (!same_arrays(fs, first, "timed")) ++bad;
  printf("refusals: %d faults\n", bad);
  return bad;
}

// A BVH whose root is a LEAF CODE has no node (the walkers start at the code; host/wide_tree.hpp).  The flattener's builders
// always emit a node, so the shape is made by hand: the one node of a two-sphere BVH is dropped and the entry names the leaf of
// both.  An update then changes the spheres and nothing else, and is not reported broken.
int check_leaf_root() {
  int bad = 0;
  Built B, Bf;
  rtx::FlatScene fs, fresh;
  if (!flatten("tiny", [](int) { return false; }, &B, &fs) || !flatten("tiny", [](int) { return true; }, &Bf, &fresh)) return 1;
  if (fs.nodes.size() != 1) { fprintf(stderr, "leaf root: the two-sphere BVH has %zu nodes, not 1\n", fs.nodes.size()); return 1; }
  for (rt::FlatEntry& e : fs.entries)
    if (e.kind == rt::ENTRY_BVH) e.a = rt::make_leaf(0, 2);
  fs.nodes.clear(); fs.nodes32.clear();
  const rtx::FlatScene first = fs;
  const rtx::MeshShadow sh = rtx::build_mesh_shadow(fs, rtx::build_update_shadow(fs));
  if (!sh.broken.empty() || sh.bvhs.size() != 1 || sh.bvhs[0].n_nodes != 0 || sh.bvhs[0].n_leaves != 0) { fprintf(stderr, "leaf root: shadow '%s'\n", sh.broken.c_str()); ++bad; }
  std::vector<int32_t> ids;
  std::vector<double> vals;
  std::string err;
  update_for(B, fs, [](int) { return true; }, true, &ids, &vals);
  if (rtx::flat_set_spheres("check", &fs, ids.data(), (int64_t)ids.size(), vals.data(), &err) != RTX_OK) { fprintf(stderr, "leaf root: refused: %s\n", err.c_str()); return 1; }
  if (!same(fs.spheres, fresh.spheres)) { fprintf(stderr, "leaf root: the spheres differ from the fresh ones\n"); ++bad; }
  if (same(fs.spheres, first.spheres)) { fprintf(stderr, "leaf root: nothing moved\n"); ++bad; }
  if (!same(fs.entries, first.entries) || !same(fs.refs, first.refs) || !fs.nodes.empty() || !same(fs.top_box32, first.top_box32)) { fprintf(stderr, "leaf root: more than the spheres changed\n"); ++bad; }
  printf("leaf-code root: %d faults\n", bad);
  return bad;
}
}  // namespace

int main() {
  int bad = 0;
  for (const char* name : {"field", "lamp", "instanced"}) bad += check_world(name);
  bad += check_refusals();
  bad += check_leaf_root();
  if (bad) { printf("set_spheres host check: %d faults\n", bad); return 1; }
  printf("set_spheres host check clean\n");
  return 0;
}
