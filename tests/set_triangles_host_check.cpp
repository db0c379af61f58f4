// Host checker of rtx_flat_set_triangles (tests/test_set_triangles_host.py builds it with the product's host sources under
// -fsanitize=address,undefined and runs it).  Three small worlds -- `mixed`: one BVH of triangles, static spheres (one of negative
// radius) and rectangles beside a BVH of moving spheres, so that the time-aware boxes exist; `shared`: a triangle in a BVH and as
// a plain top-level slot, another listed twice; `instanced`: an instance tree of two Translate(RotateY(BvhNode)) and a
// Translate(list of 3 triangles) -- are built at rest, deformed with full and partial updates and compared with the world
// flattened from scratch with those vertices; moved back, every array must be what it was.  Then the refusals, each of which
// must leave the scene untouched, a BVH whose root is a leaf code (made by hand: no builder emits one), and the shadow's
// `broken` paths on hand-damaged arrays.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
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
struct Tri { double v[9]; };
typedef std::function<bool(int)> Moved;  // does the k-th deformable triangle (in creation order) take its displaced vertices?

Tri displaced(const Tri& t, double cell) {
  Tri o = t;
  for (int c = 0; c < 3; ++c) {
    const double x = t.v[3 * c], y = t.v[3 * c + 1], z = t.v[3 * c + 2];
    o.v[3 * c + 1] = y + cell * std::sin(2.1 * x + 0.3) * std::cos(1.7 * z + 0.5);
    o.v[3 * c] = x + 0.11 * (y - 0.5) + 0.05 * cell * std::sin(3.3 * z);
    o.v[3 * c + 2] = z + 0.07 * cell * std::cos(2.9 * x);
  }
  return o;
}

struct Built {
  rtx::SceneGraph g{5};
  int32_t world = -1;
  std::vector<int32_t> handle;  // per deformable triangle, in creation order
  std::vector<Tri> rest, moved;
};

struct Maker {
  Built* B;
  Moved on;
  int32_t tri(double x, double y, double z, double s, double cell, int32_t mat) {
    Tri t = {{x, y, z, x + s, y + 0.2 * s, z + 0.1 * s, x + 0.3 * s, y + 0.1 * s, z + s}};
    const Tri m = displaced(t, cell);
    const Tri& use = on((int)B->handle.size()) ? m : t;
    const int32_t h = B->g.triangle(&use.v[0], &use.v[3], &use.v[6], mat);
    B->handle.push_back(h);
    B->rest.push_back(t);
    B->moved.push_back(m);
    return h;
  }
  int32_t list(const std::vector<int32_t>& o) { const int32_t l = B->g.list_new(); for (int32_t x : o) B->g.list_add(l, x); return l; }
  std::vector<int32_t> sheet(int n, double x0, double y0, double z0, int32_t mat) {
    std::vector<int32_t> out;
    for (int k = 0; k < n; ++k) out.push_back(tri(x0 + 0.6 * (k % 4), y0 + 0.03 * k, z0 + 0.6 * (k / 4), 0.55, 0.5, mat));
    return out;
  }
};

void make_world(Built* B, const std::string& name, const Moved& on) {
  rtx::SceneGraph& g = B->g;
  Maker m{B, on};
  const double c1[3] = {0.5, 0.5, 0.5}, c2[3] = {0.8, 0.8, 0.9};
  const int32_t grey = g.lambertian(g.solid_color(c1)), metal = g.metal(c2, 0.2), glass = g.dielectric(1.5);
  auto sphere = [&](double x, double y, double z, double r, int32_t mat) { const double c[3] = {x, y, z}; return g.sphere(c, r, mat); };
  const int32_t ground = sphere(2.0, -500.0, 2.0, 500.0, grey);
  if (name == "mixed") {
    std::vector<int32_t> o = m.sheet(13, 0.5, 0.8, 0.6, grey);
    o.push_back(sphere(1.0, 1.6, 1.2, 0.45, glass));
    o.push_back(sphere(1.0, 1.6, 1.2, -0.4, glass));
    o.push_back(sphere(3.2, 1.5, 2.8, 0.5, metal));
    o.push_back(g.rect(rtx::H_XZ_RECT, 0.4, 1.6, 2.6, 3.8, 1.9, grey));
    o.push_back(g.rect(rtx::H_XY_RECT, 2.6, 3.9, 0.5, 1.8, 0.45, metal));
    o.push_back(g.rect(rtx::H_YZ_RECT, 0.7, 1.9, 1.1, 2.3, 4.1, grey));
    const double a[3] = {3.0, 3.0, -2.0}, b[3] = {3.0, 3.6, -2.0};
    const int32_t movers = g.bvh_from_list(m.list({g.moving_sphere(a, b, 0.0, 1.0, 0.3, grey), sphere(5.0, 3.0, -2.0, 0.3, grey)}), 0.0, 1.0);
    B->world = m.list({ground, g.bvh_from_list(m.list(o), 0.0, 1.0), movers});
  } else if (name == "shared") {
    std::vector<int32_t> o = m.sheet(6, 0.5, 0.8, 0.6, grey);
    const int32_t both = m.tri(1.0, 2.0, 1.0, 1.2, 0.5, metal), alone = m.tri(3.0, 1.8, 2.0, 1.1, 0.5, metal), twice = m.tri(0.6, 2.4, 3.0, 0.9, 0.5, grey);
    o.push_back(both); o.push_back(twice); o.push_back(twice);
    B->world = m.list({ground, both, g.bvh_from_list(m.list(o), 0.0, 1.0), alone});
  } else if (name == "instanced") {
    const double t0[3] = {0.4, 0.2, 0.3}, t1[3] = {3.1, 0.3, 2.2}, t2[3] = {1.2, 0.4, 4.0};
    const int32_t a = g.translate(t0, g.rotate_y(20.0, g.bvh_from_list(m.list(m.sheet(9, 0.2, 0.8, 0.3, grey)), 0.0, 1.0)));
    const int32_t b = g.translate(t1, g.rotate_y(-35.0, g.bvh_from_list(m.list(m.sheet(12, 0.2, 0.8, 0.3, metal)), 0.0, 1.0)));
    const int32_t c = g.translate(t2, m.list(m.sheet(3, 0.2, 0.5, 0.3, grey)));
    B->world = m.list({ground, g.instance_bvh_from_list(m.list({a, b, c}))});
  } else if (name == "tiny") {  // two triangles in one BVH: one node (check_leaf_root turns it into a leaf-code root)
    B->world = m.list({ground, g.bvh_from_list(m.list(m.sheet(2, 0.5, 0.8, 0.6, grey)), 0.0, 1.0)});
  } else {  // movers: the refusal
    std::vector<int32_t> o = m.sheet(5, 0.5, 0.8, 0.6, grey);
    const double a[3] = {1.0, 2.5, 1.0}, b[3] = {1.0, 3.0, 1.0};
    o.push_back(g.moving_sphere(a, b, 0.0, 1.0, 0.3, grey));
    B->world = m.list({ground, g.bvh_from_list(m.list(o), 0.0, 1.0)});
  }
}

bool flatten(const std::string& name, const Moved& on, Built* B, rtx::FlatScene* fs) {
  make_world(B, name, on);
  std::string err;
  if (!rtx::flatten_scene(B->g, B->world, rtx::BuildOptions(), fs, &err)) { fprintf(stderr, "flatten: %s\n", err.c_str()); return false; }
  return true;
}

// ids and vertices that give the deformable triangles chosen by `pick` the vertices `to` says (displaced or rest)
void update_for(const Built& B, const rtx::FlatScene& fs, const Moved& pick, bool to_moved, std::vector<int32_t>* ids, std::vector<double>* verts) {
  ids->clear(); verts->clear();
  for (size_t k = 0; k < B.handle.size(); ++k) {
    if (!pick((int)k)) continue;
    ids->push_back(fs.handle_triangle_id[(size_t)B.handle[k]]);
    const Tri& t = to_moved ? B.moved[k] : B.rest[k];
    verts->insert(verts->end(), t.v, t.v + 9);
  }
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }
bool same_arrays(const rtx::FlatScene& a, const rtx::FlatScene& b, const char* what) {
  const bool ok = same(a.triangles, b.triangles) && same(a.triangle_id, b.triangle_id) && same(a.entries, b.entries) && same(a.top_level, b.top_level) &&
                  same(a.nodes, b.nodes) && same(a.nodes32, b.nodes32) && same(a.motion32, b.motion32) && same(a.member_local_box, b.member_local_box) &&
                  same(a.refs, b.refs) && same(a.rects, b.rects) && same(a.spheres, b.spheres) && same(a.top_box32, b.top_box32);
  if (!ok) fprintf(stderr, "%s: the arrays differ\n", what);
  return ok;
}

// The checker's own box of everything below child code `code` of BVH entry e: the union of the reference boxes (hit.rs) of its
// primitives, written out again here so that the refit is not judged by its own arithmetic.
struct Box6 { double lo[3], hi[3]; };
Box6 box_below(const rtx::FlatScene& fs, const rt::FlatEntry& e, int32_t code) {
  Box6 b;
  for (int a = 0; a < 3; ++a) { b.lo[a] = HUGE_VAL; b.hi[a] = -HUGE_VAL; }
  auto grow = [&](const double* lo, const double* hi) { for (int a = 0; a < 3; ++a) { b.lo[a] = std::fmin(b.lo[a], lo[a]); b.hi[a] = std::fmax(b.hi[a], hi[a]); } };
  if (code >= 0) {
    for (int c = 0; c < 2; ++c) { const Box6 k = box_below(fs, e, fs.nodes[(size_t)code].child[c]); grow(k.lo, k.hi); }
    return b;
  }
  for (uint32_t i = 0; i < rt::leaf_count(code); ++i) {
    const rt::PrimRef r = fs.refs[(size_t)e.b + rt::leaf_first(code) + i];
    const uint32_t k = rt::primref_index(r);
    double lo[3], hi[3];
    if (rt::primref_type(r) == rt::PRIM_SPHERE) {
      const rt::FlatSphere& s = fs.spheres[k];
      const double c[3] = {s.cx, s.cy, s.cz};
      for (int a = 0; a < 3; ++a) { lo[a] = c[a] - std::fabs(s.radius); hi[a] = c[a] + std::fabs(s.radius); }
    } else if (rt::primref_type(r) == rt::PRIM_RECT) {
      const rt::FlatRect& q = fs.rects[k];
      const int thin = q.axis == rt::RECT_XY ? 2 : (q.axis == rt::RECT_XZ ? 1 : 0), u = thin == 0 ? 1 : 0, v = thin == 2 ? 1 : 2;
      lo[thin] = q.k - 0.0001; hi[thin] = q.k + 0.0001; lo[u] = q.a0; hi[u] = q.a1; lo[v] = q.b0; hi[v] = q.b1;
    } else {
      const rt::FlatTriangle& t = fs.triangles[k];
      for (int a = 0; a < 3; ++a) { lo[a] = std::fmin(std::fmin(t.v0[a], t.v1[a]), t.v2[a]); hi[a] = std::fmax(std::fmax(t.v0[a], t.v1[a]), t.v2[a]); }
    }
    grow(lo, hi);
  }
  return b;
}
int audit_boxes(const rtx::FlatScene& fs, const char* what) {
  int bad = 0;
  for (const rt::FlatEntry& e : fs.entries) {
    if (e.kind != rt::ENTRY_BVH || e.a < 0) continue;
    bool timed = false;
    for (int32_t i = 0; i < e.c; ++i) timed |= rt::primref_type(fs.refs[(size_t)e.b + i]) == rt::PRIM_MOVING_SPHERE;
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

// The updated scene against the one flattened from scratch with those vertices.  The worlds here are small enough that the
// builder picks the same topology for both, so the comparison is every array byte for byte; where it does not (reported), the
// triangles by id, the boxes of the instance trees' leaves by slot and top_box32 still have to agree.
int against_fresh(const rtx::FlatScene& got, const rtx::FlatScene& fresh, const rtx::FlatScene& first, const char* what) {
  int bad = audit_boxes(got, what);
  std::map<int32_t, rt::FlatTriangle> by_id;
  for (size_t t = 0; t < fresh.triangles.size(); ++t) by_id[fresh.triangle_id[t]] = fresh.triangles[t];
  if (got.triangles.size() != fresh.triangles.size() || !same(got.triangle_id, first.triangle_id)) { fprintf(stderr, "%s: triangle ids changed\n", what); ++bad; }
  for (size_t t = 0; t < got.triangles.size() && t < got.triangle_id.size(); ++t)
    if (memcmp(&got.triangles[t], &by_id[got.triangle_id[t]], sizeof(rt::FlatTriangle)) != 0) { fprintf(stderr, "%s: triangle %zu differs from the fresh one of its id\n", what, t); ++bad; }
  if (!same(got.entries, first.entries) || !same(got.refs, first.refs) || !same(got.top_level, first.top_level)) { fprintf(stderr, "%s: entries / refs / top_level changed\n", what); ++bad; }
  for (size_t n = 0; n < got.nodes.size(); ++n) {
    if (memcmp(got.nodes[n].child, first.nodes[n].child, 16) != 0) { fprintf(stderr, "%s: node %zu's topology changed\n", what, n); ++bad; }
    for (int c = 0; c < 2; ++c)
      for (int a = 0; a < 3; ++a) {
        if (got.nodes32[n].lo[c][a] != rtx::narrow_down(got.nodes[n].bmin[c][a]) || got.nodes32[n].hi[c][a] != rtx::narrow_up(got.nodes[n].bmax[c][a])) { fprintf(stderr, "%s: nodes32[%zu] is not the narrowing of nodes\n", what, n); ++bad; }
      }
  }
  if (!same(got.top_box32, fresh.top_box32)) { fprintf(stderr, "%s: top_box32 differs\n", what); ++bad; }
  if (!same(got.member_local_box, fresh.member_local_box)) { fprintf(stderr, "%s: member_local_box differs\n", what); ++bad; }
  // (equal child codes are equal trees only when the leaves hold the same primitives: refs and the triangles' order too)
  bool same_topology = got.nodes.size() == fresh.nodes.size() && same(got.refs, fresh.refs) && same(got.triangle_id, fresh.triangle_id);
  for (size_t n = 0; same_topology && n < got.nodes.size(); ++n) same_topology = memcmp(got.nodes[n].child, fresh.nodes[n].child, 16) == 0;  // children and split axis
  if (same_topology) {
    if (!same(got.nodes, fresh.nodes) || !same(got.nodes32, fresh.nodes32) || !same(got.motion32, fresh.motion32)) { fprintf(stderr, "%s: same topology as the fresh scene, other boxes\n", what); ++bad; }
  } else {
    printf("%s: the fresh flatten chose another topology (boxes compared through the triangles and the members only)\n", what);
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
  const int n_def = (int)B0.handle.size();
  const std::vector<Moved> picks = {all, [](int k) { return k == 3; }, [](int k) { return k % 7 == 0; }, [n_def](int k) { return k >= n_def / 2; }};
  std::vector<int32_t> ids;
  std::vector<double> verts;
  std::string err;
  for (size_t p = 0; p < picks.size(); ++p) {
    Built Bf;
    rtx::FlatScene fresh;
    if (!flatten(name, picks[p], &Bf, &fresh)) return 1;
    update_for(B0, fs, picks[p], true, &ids, &verts);
    if (rtx::flat_set_triangles("check", &fs, ids.data(), (int64_t)ids.size(), verts.data(), &err) != RTX_OK) { fprintf(stderr, "%s: update %zu refused: %s\n", name.c_str(), p, err.c_str()); return 1; }
    if (same(fs.nodes, first.nodes)) { fprintf(stderr, "%s: update %zu moved no box\n", name.c_str(), p); ++bad; }
    bad += against_fresh(fs, fresh, first, (name + " update " + std::to_string(p)).c_str());
    update_for(B0, fs, picks[p], false, &ids, &verts);
    if (rtx::flat_set_triangles("check", &fs, ids.data(), (int64_t)ids.size(), verts.data(), &err) != RTX_OK) { fprintf(stderr, "%s: way back %zu refused: %s\n", name.c_str(), p, err.c_str()); return 1; }
    if (!same_arrays(fs, first, (name + " back at rest").c_str())) ++bad;
  }
  // two updates in a row: first half, second half == all
  Built Bf;
  rtx::FlatScene fresh;
  if (!flatten(name, all, &Bf, &fresh)) return 1;
  for (int half = 0; half < 2; ++half) {
    update_for(B0, fs, [n_def, half](int k) { return (k < n_def / 2) == (half == 0); }, true, &ids, &verts);
    if (rtx::flat_set_triangles("check", &fs, ids.data(), (int64_t)ids.size(), verts.data(), &err) != RTX_OK) { fprintf(stderr, "%s: half %d refused: %s\n", name.c_str(), half, err.c_str()); return 1; }
  }
  bad += against_fresh(fs, fresh, first, (name + " two updates in a row").c_str());
  printf("%s: %d deformable triangles, %zu flat, %zu nodes: %d faults\n", name.c_str(), n_def, fs.triangles.size(), fs.nodes.size(), bad);
  return bad;
}

int check_refusals() {
  int bad = 0;
  Built B;
  rtx::FlatScene fs;
  if (!flatten("mixed", [](int) { return false; }, &B, &fs)) return 1;
  const rtx::FlatScene first = fs;
  const double nan = std::nan(""), inf = HUGE_VAL;
  std::vector<double> good(18, 1.5), with_nan = good, with_inf = good;
  with_nan[13] = nan; with_inf[8] = inf;
  const int32_t n_ids = 13;
  struct Case { const char* name; std::vector<int32_t> ids; int64_t n; const double* v; bool null_ids; const char* word; };
  const std::vector<Case> cases = {
      {"null ids", {0, 1}, 2, good.data(), true, "ids is NULL"},          {"null vertices", {0, 1}, 2, nullptr, false, "vertices is NULL"},
      {"negative n", {0, 1}, -1, good.data(), false, "n < 0"},            {"id negative", {0, -1}, 2, good.data(), false, "ids[1] is out of range"},
      {"id past the end", {n_ids, 1}, 2, good.data(), false, "ids[0] is out of range"}, {"id named twice", {1, 1}, 2, good.data(), false, "twice"},
      {"NaN vertex", {0, 1}, 2, with_nan.data(), false, "vertices[1][4] is not finite"}, {"infinite vertex", {0, 1}, 2, with_inf.data(), false, "vertices[0][8] is not finite"},
  };
  for (const Case& c : cases) {
    std::string err;
    const rtx_status st = rtx::flat_set_triangles("check", &fs, c.null_ids ? nullptr : c.ids.data(), c.n, c.v, &err);
    if (st != RTX_EINVAL || err.find(c.word) == std::string::npos) { fprintf(stderr, "refusal '%s': status %d, message '%s'\n", c.name, (int)st, err.c_str()); ++bad; }
    if (!same_arrays(fs, first, c.name)) ++bad;
  }
  std::string err;
  if (rtx::flat_set_triangles("check", nullptr, cases[0].ids.data(), 2, good.data(), &err) != RTX_EINVAL || err.find("scene is NULL") == std::string::npos) { fprintf(stderr, "NULL scene accepted\n"); ++bad; }
  if (rtx::flat_set_triangles("check", &fs, cases[0].ids.data(), 0, good.data(), &err) != RTX_OK || !same_arrays(fs, first, "n = 0")) { fprintf(stderr, "n = 0 did something\n"); ++bad; }
  // a BVH that holds a MovingSphere
  Built Bm;
  rtx::FlatScene fm;
  if (!flatten("movers", [](int) { return false; }, &Bm, &fm)) return 1;
  const rtx::FlatScene fm_first = fm;
  std::vector<int32_t> ids;
  std::vector<double> verts;
  update_for(Bm, fm, [](int) { return true; }, true, &ids, &verts);
  if (rtx::flat_set_triangles("check", &fm, ids.data(), (int64_t)ids.size(), verts.data(), &err) != RTX_EUNSUPPORTED || err.find("MovingSphere") == std::string::npos) { fprintf(stderr, "movers accepted: %s\n", err.c_str()); ++bad; }
  if (!same_arrays(fm, fm_first, "movers")) ++bad;
  printf("refusals: %d faults\n", bad);
  return bad;
}

// A BVH whose root is a LEAF CODE has no node (the walkers start at the code; host/wide_tree.hpp).  The flattener's builders
// always emit a node, so the shape is made by hand: the one node of a two-triangle BVH is dropped and the entry names the
// leaf of both.  An update then changes the triangles and nothing else, and is not reported broken.
int check_leaf_root() {
  int bad = 0;
  Built B, Bf;
  rtx::FlatScene fs, fresh;
  if (!flatten("tiny", [](int) { return false; }, &B, &fs) || !flatten("tiny", [](int) { return true; }, &Bf, &fresh)) return 1;
  if (fs.nodes.size() != 1) { fprintf(stderr, "leaf root: the two-triangle BVH has %zu nodes, not 1\n", fs.nodes.size()); return 1; }
  for (rt::FlatEntry& e : fs.entries)
    if (e.kind == rt::ENTRY_BVH) e.a = rt::make_leaf(0, 2);
  fs.nodes.clear(); fs.nodes32.clear();
  const rtx::FlatScene first = fs;
  const rtx::MeshShadow sh = rtx::build_mesh_shadow(fs, rtx::build_update_shadow(fs));
  if (!sh.broken.empty() || sh.bvhs.size() != 1 || sh.bvhs[0].n_nodes != 0 || sh.bvhs[0].n_leaves != 0) { fprintf(stderr, "leaf root: shadow '%s'\n", sh.broken.c_str()); ++bad; }
  std::vector<int32_t> ids;
  std::vector<double> verts;
  std::string err;
  update_for(B, fs, [](int) { return true; }, true, &ids, &verts);
  if (rtx::flat_set_triangles("check", &fs, ids.data(), (int64_t)ids.size(), verts.data(), &err) != RTX_OK) { fprintf(stderr, "leaf root: refused: %s\n", err.c_str()); return 1; }
  std::map<int32_t, rt::FlatTriangle> by_id;
  for (size_t t = 0; t < fresh.triangles.size(); ++t) by_id[fresh.triangle_id[t]] = fresh.triangles[t];
  for (size_t t = 0; t < fs.triangles.size(); ++t)
    if (memcmp(&fs.triangles[t], &by_id[fs.triangle_id[t]], sizeof(rt::FlatTriangle)) != 0) { fprintf(stderr, "leaf root: triangle %zu differs from the fresh one\n", t); ++bad; }
  if (same(fs.triangles, first.triangles)) { fprintf(stderr, "leaf root: nothing moved\n"); ++bad; }
  if (!same(fs.entries, first.entries) || !same(fs.refs, first.refs) || !fs.nodes.empty() || !same(fs.top_box32, first.top_box32)) { fprintf(stderr, "leaf root: more than the triangles changed\n"); ++bad; }
  printf("leaf-code root: %d faults\n", bad);
  return bad;
}

// Every hand-damaged copy must be reported broken (and an update refused with that message), never walked.
int check_broken() {
  int bad = 0;
  Built B;
  rtx::FlatScene good;
  if (!flatten("instanced", [](int) { return false; }, &B, &good)) return 1;
  int32_t bvh_entry = -1, bvh_node_with_child = -1;
  for (size_t k = 0; k < good.entries.size(); ++k)
    if (good.entries[k].kind == rt::ENTRY_BVH && bvh_entry < 0) bvh_entry = (int32_t)k;
  for (size_t n = 0; n < good.nodes.size(); ++n)
    for (int c = 0; c < 2; ++c)
      if (!rt::node_child_is_leaf(good.nodes[n].child[c]) && bvh_node_with_child < 0) bvh_node_with_child = (int32_t)n;
  if (bvh_entry < 0 || bvh_node_with_child < 0) { fprintf(stderr, "broken: the world has no BVH with an inner child\n"); return 1; }
  struct Damage { const char* name; std::function<void(rtx::FlatScene*)> hurt; const char* word; };
  const std::vector<Damage> damages = {
      {"id table too short", [](rtx::FlatScene* f) { f->triangle_id.pop_back(); }, "one id per flat triangle"},
      {"id out of range", [](rtx::FlatScene* f) { f->triangle_id[0] = 1 << 20; }, "outside [0"},
      {"negative id", [](rtx::FlatScene* f) { f->triangle_id[1] = -2; }, "outside [0"},
      {"id skipped", [](rtx::FlatScene* f) { for (int32_t& i : f->triangle_id) if (i == 2) i = 3; }, "skips an id"},
      {"reference past the triangles", [](rtx::FlatScene* f) { for (rt::PrimRef& r : f->refs) if (rt::primref_type(r) == rt::PRIM_TRIANGLE) { r = rt::make_primref(rt::PRIM_TRIANGLE, 1u << 20); break; } }, "outside the triangle array"},
      {"run past the references", [=](rtx::FlatScene* f) { f->entries[(size_t)bvh_entry].c = 1 << 20; }, "outside the reference array"},
      {"root past the nodes", [=](rtx::FlatScene* f) { f->entries[(size_t)bvh_entry].a = 1 << 20; }, "root outside the node array"},
      {"child past the nodes", [=](rtx::FlatScene* f) { rt::FlatNode& n = f->nodes[(size_t)bvh_node_with_child]; n.child[rt::node_child_is_leaf(n.child[0]) ? 1 : 0] = 1 << 20; }, "outside the node array"},
      {"a cycle", [=](rtx::FlatScene* f) { rt::FlatNode& n = f->nodes[(size_t)bvh_node_with_child]; n.child[rt::node_child_is_leaf(n.child[0]) ? 1 : 0] = bvh_node_with_child; }, "two parents"},
      {"leaf past its run", [=](rtx::FlatScene* f) { f->entries[(size_t)bvh_entry].c = 1; }, "outside its run"},
      {"local boxes too short", [](rtx::FlatScene* f) { f->member_local_box.pop_back(); }, "member_local_box"},
      {"top boxes too short", [](rtx::FlatScene* f) { f->top_box32.pop_back(); }, "top_box32"},
  };
  const int32_t ids[1] = {0};
  const double verts[9] = {1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 2.0, 1.5};
  for (const Damage& d : damages) {
    rtx::FlatScene f = good;
    d.hurt(&f);
    const rtx::FlatScene before = f;
    const rtx::MeshShadow sh = rtx::build_mesh_shadow(f, rtx::build_update_shadow(f));
    if (sh.broken.find(d.word) == std::string::npos) { fprintf(stderr, "broken '%s': the shadow says '%s'\n", d.name, sh.broken.c_str()); ++bad; }
    std::string err;
    if (rtx::flat_set_triangles("check", &f, ids, 1, verts, &err) != RTX_EINVAL || err.find(d.word) == std::string::npos) { fprintf(stderr, "broken '%s': the update says '%s'\n", d.name, err.c_str()); ++bad; }
    if (!same_arrays(f, before, d.name)) ++bad;
  }
  const rtx::MeshShadow ok = rtx::build_mesh_shadow(good, rtx::build_update_shadow(good));
  if (!ok.broken.empty()) { fprintf(stderr, "the undamaged scene is reported broken: %s\n", ok.broken.c_str()); ++bad; }
  printf("broken shadows: %d faults\n", bad);
  return bad;
}
}  // namespace

int main() {
  int bad = 0;
  for (const char* name : {"mixed", "shared", "instanced"}) bad += check_world(name);
  bad += check_refusals();
  bad += check_leaf_root();
  bad += check_broken();
  if (bad) { printf("set_triangles host check: %d faults\n", bad); return 1; }
  printf("set_triangles host check clean\n");
  return 0;
}
