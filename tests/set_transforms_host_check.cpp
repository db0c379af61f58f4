// Host checker of rtx_flat_set_transforms (tests/test_set_transforms_host.py builds it with the product's host sources under
// -fsanitize=address,undefined and runs it).  A small zoo -- a tree whose members cover every chain length, a negative-radius
// sphere, a BVH under a chain; beside the tree a ConstantMedium over a chain and a BvhNode of moving spheres, so that the
// time-aware boxes exist -- is built at a pose, moved to another with full and with partial updates, and compared with the
// zoo flattened from scratch at that pose: entries byte for byte, every leaf box by slot, every union, both narrowed copies;
// moved back, every array must be what it was.  Then the refusals, each of which must leave the scene untouched, and the
// narrowing the device refit uses (core/member_box.hpp) against the converter's (host/f32_layout.hpp).
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "../ray-tracing-series-rust_amd/csrc/host/set_transforms.hpp"

namespace rtx {
// the GPU builder lives in csrc/hip/lbvh.hip: not part of a CPU-only program
int32_t build_bvh_gpu(const std::vector<double>&, int, std::vector<rt::FlatNode>*, std::vector<uint32_t>*, int32_t*, double*, std::string* err) {
  if (err) *err = "no GPU builder in the sanitizer program";
  return -1;
}
}  // namespace rtx

namespace {
struct V { double v[3]; };
V v3(double x, double y, double z) { return V{{x, y, z}}; }

// the parameters of every wrapper of the zoo, in the order make_world uses them
struct Pose {
  std::vector<V> t;
  std::vector<double> r;
};
Pose pose_at(double s) {  // s = 0: the original pose
  Pose p;
  for (int k = 0; k < 9; ++k) p.t.push_back(v3(-4.0 + 1.1 * k + 0.37 * s * (k % 3 - 1), 0.05 * s * k, -1.0 + 0.4 * (k % 4) - 0.29 * s * (k % 2)));
  for (int k = 0; k < 8; ++k) p.r.push_back(17.0 * k - 40.0 + 61.0 * s * (k % 3 + 1));
  return p;
}

struct Built {
  rtx::SceneGraph g{5};
  int32_t world = -1;
  // slot -> its ops (outermost first) as (kind, index into Pose::t or Pose::r)
  std::map<int32_t, std::vector<std::pair<int32_t, int>>> chain;
};

void make_world(Built* B, const Pose& p) {
  rtx::SceneGraph& g = B->g;
  const V c1 = v3(0.5, 0.5, 0.5), c2 = v3(0.8, 0.8, 0.9), fog = v3(0.2, 0.4, 0.9);
  const int32_t grey = g.lambertian(g.solid_color(c1.v)), metal = g.metal(c2.v, 0.2), glass = g.dielectric(1.5);
  auto list = [&](const std::vector<int32_t>& o) { const int32_t l = g.list_new(); for (int32_t x : o) g.list_add(l, x); return l; };
  auto sphere = [&](double x, double y, double z, double r, int32_t m) { return g.sphere(v3(x, y, z).v, r, m); };
  auto prism = [&](int32_t m) { return g.rect_prism(v3(-0.3, 0.0, -0.5).v, v3(0.3, 0.7, 0.5).v, m); };
  auto T = [&](int k, int32_t o) { return g.translate(p.t[(size_t)k].v, o); };
  auto R = [&](int k, int32_t o) { return g.rotate_y(p.r[(size_t)k], o); };
  std::vector<int32_t> balls;
  for (int k = 0; k < 5; ++k) balls.push_back(sphere(-1.0 + 0.7 * k, 0.3 + 0.02 * k, 0.1 * (k % 2), 0.3, metal));
  const int32_t ball_bvh = g.bvh_from_list(list(balls), 0.0, 1.0);
  const int32_t t = rt::XFORM_TRANSLATE, r = rt::XFORM_ROTATE_Y;
  std::vector<int32_t> members;
  int32_t slot = 1;  // the ground is slot 0
  auto member = [&](int32_t o, std::vector<std::pair<int32_t, int>> ops) { members.push_back(o); if (!ops.empty()) B->chain[slot] = ops; ++slot; };
  member(sphere(-4.0, 0.6, 2.0, 0.6, grey), {});
  member(sphere(1.0, 0.7, 2.2, 0.7, glass), {});
  member(sphere(1.0, 0.7, 2.2, -0.6, glass), {});  // the hollow-glass idiom: an inverted reference box
  member(T(0, R(0, ball_bvh)), {{t, 0}, {r, 0}});  // a BVH member under a chain
  member(R(1, prism(grey)), {{r, 1}});
  member(T(1, prism(metal)), {{t, 1}});
  member(R(2, T(2, prism(grey))), {{r, 2}, {t, 2}});
  member(T(3, R(3, T(4, sphere(0.0, 0.0, 0.0, 0.45, glass)))), {{t, 3}, {r, 3}, {t, 4}});
  member(T(5, R(4, T(6, R(5, prism(metal))))), {{t, 5}, {r, 4}, {t, 6}, {r, 5}});  // the four-op chain
  member(T(7, R(6, g.rect(rtx::H_XY_RECT, -0.5, 0.5, 0.1, 0.9, 0.0, grey))), {{t, 7}, {r, 6}});
  const V a = v3(3.0, 2.0, -2.0), b = v3(3.0, 2.6, -2.0), c = v3(4.0, 2.0, -2.0);
  const int32_t movers = g.bvh_from_list(list({g.moving_sphere(a.v, b.v, 0.0, 1.0, 0.3, grey), g.moving_sphere(c.v, c.v, 0.0, 1.0, 0.3, grey),
                                               sphere(5.0, 2.0, -2.0, 0.3, grey)}), 0.0, 1.0);
  const int32_t smoke = g.constant_medium(fog.v, 0.8, T(8, R(7, prism(grey))));
  const int32_t tree = g.instance_bvh_from_list(list(members));
  B->chain[slot + 1] = {{t, 8}, {r, 7}};  // ground, the members, the movers' BVH, then the medium
  B->world = list({sphere(0.0, -500.0, 0.0, 500.0, grey), tree, movers, smoke});
}

bool flatten(const Pose& p, Built* B, rtx::FlatScene* fs) {
  make_world(B, p);
  std::string err;
  if (!rtx::flatten_scene(B->g, B->world, rtx::BuildOptions(), fs, &err)) { fprintf(stderr, "flatten: %s\n", err.c_str()); return false; }
  return true;
}

// updates that set the chains of `slots` (all chains when empty) to pose p
std::vector<RtxSlotOps> updates_for(const Built& B, const Pose& p, const std::vector<int32_t>& slots) {
  std::vector<RtxSlotOps> out;
  for (const auto& kv : B.chain) {
    bool want = slots.empty();
    for (int32_t s : slots) want |= s == kv.first;
    if (!want) continue;
    RtxSlotOps u;
    memset(&u, 0, sizeof(u));
    u.slot = kv.first;
    u.n_ops = (int32_t)kv.second.size();
    for (size_t k = 0; k < kv.second.size(); ++k) {
      u.ops[k].op = kv.second[k].first;
      if (kv.second[k].first == rt::XFORM_TRANSLATE) memcpy(u.ops[k].v, p.t[(size_t)kv.second[k].second].v, sizeof(u.ops[k].v));
      else u.ops[k].v[0] = p.r[(size_t)kv.second[k].second];
    }
    out.push_back(u);
  }
  return out;
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }
bool same_arrays(const rtx::FlatScene& a, const rtx::FlatScene& b, const char* what) {
  const bool ok = same(a.entries, b.entries) && same(a.top_level, b.top_level) && same(a.nodes, b.nodes) && same(a.nodes32, b.nodes32) &&
                  same(a.motion32, b.motion32) && same(a.member_local_box, b.member_local_box) && same(a.refs, b.refs) && same(a.rects, b.rects);
  if (!ok) fprintf(stderr, "%s: the arrays differ\n", what);
  return ok;
}

// the moved scene against the scene flattened at that pose: entries and top_level byte for byte; in the tree every leaf box by
// slot, every internal child box the union of the two under it, the narrowed copies, and the topology of `first`
int against_fresh(const rtx::FlatScene& got, const rtx::FlatScene& fresh, const rtx::FlatScene& first, const char* what) {
  int bad = 0;
  if (!same(got.entries, fresh.entries) || !same(got.top_level, fresh.top_level)) { fprintf(stderr, "%s: entries differ from the fresh scene's\n", what); ++bad; }
  const rtx::UpdateShadow sg = rtx::build_update_shadow(got), sf = rtx::build_update_shadow(fresh);
  if (!sg.broken.empty() || !sf.broken.empty() || sg.trees.size() != 1 || sf.trees.size() != 1) { fprintf(stderr, "%s: shadow: %s%s\n", what, sg.broken.c_str(), sf.broken.c_str()); return bad + 1; }
  const rtx::TreeShadow& tg = sg.trees[0];
  for (int32_t m = 0; m < tg.n_slots; ++m) {
    const rt::FlatNode& a = got.nodes[(size_t)sg.leaf_parent[2 * (size_t)m]];
    const rt::FlatNode& b = fresh.nodes[(size_t)sf.leaf_parent[2 * (size_t)m]];
    const int ca = sg.leaf_parent[2 * (size_t)m + 1], cb = sf.leaf_parent[2 * (size_t)m + 1];
    if (memcmp(a.bmin[ca], b.bmin[cb], 24) != 0 || memcmp(a.bmax[ca], b.bmax[cb], 24) != 0) { fprintf(stderr, "%s: member %d: leaf box differs from the fresh tree's\n", what, m); ++bad; }
  }
  for (int32_t n = tg.node_base; n < tg.node_base + tg.n_nodes; ++n) {
    const rt::FlatNode& nd = got.nodes[(size_t)n];
    for (int c = 0; c < 2; ++c) {
      if (!rt::node_child_is_leaf(nd.child[c])) {
        const rt::FlatNode& ch = got.nodes[(size_t)nd.child[c]];
        for (int x = 0; x < 3; ++x)
          if (nd.bmin[c][x] != std::fmin(ch.bmin[0][x], ch.bmin[1][x]) || nd.bmax[c][x] != std::fmax(ch.bmax[0][x], ch.bmax[1][x])) { fprintf(stderr, "%s: node %d: not the union\n", what, n); ++bad; }
      }
      for (int x = 0; x < 3; ++x) {
        const rt::FlatNode32& m = got.nodes32[(size_t)n];
        if (m.lo[c][x] != rtx::narrow_down(nd.bmin[c][x]) || m.hi[c][x] != rtx::narrow_up(nd.bmax[c][x])) { fprintf(stderr, "%s: node %d: nodes32\n", what, n); ++bad; }
        const rt::FlatMotion32& mo = got.motion32[(size_t)n];
        if (mo.lo0[c][x] != m.lo[c][x] || mo.hi0[c][x] != m.hi[c][x] || mo.dlo[c][x] != 0.0f || mo.dhi[c][x] != 0.0f) { fprintf(stderr, "%s: node %d: motion32\n", what, n); ++bad; }
      }
    }
    if (memcmp(nd.child, first.nodes[(size_t)n].child, 8) != 0 || memcmp(nd.pad, first.nodes[(size_t)n].pad, 8) != 0) { fprintf(stderr, "%s: node %d: topology changed\n", what, n); ++bad; }
  }
  return bad;
}

int refused(rtx::FlatScene* fs, const rtx::FlatScene& before, const RtxSlotOps* u, int64_t n, const char* word, const char* what) {
  std::string err;
  if (rtx::flat_set_transforms("check", fs, u, n, &err)) { fprintf(stderr, "not refused: %s\n", what); return 1; }
  if (err.find(word) == std::string::npos) { fprintf(stderr, "%s: the message does not name '%s': %s\n", what, word, err.c_str()); return 1; }
  return !fs || same_arrays(*fs, before, what) ? 0 : 1;
}
}  // namespace

int main() {
  int bad = 0;
  const Pose p0 = pose_at(0.0), p1 = pose_at(1.0), p2 = pose_at(-0.6);
  Built B0;
  rtx::FlatScene fs;
  if (!flatten(p0, &B0, &fs)) return 1;
  const rtx::FlatScene first = fs;
  if (fs.motion32.empty() || fs.n_instance_trees != 1 || fs.member_local_box.size() != 6 * 10) { fprintf(stderr, "the zoo is not what this program expects\n"); return 1; }
  std::string err;
  // full sets: p0 -> p1 -> p2, each against a fresh flatten; then home
  for (const Pose* p : {&p1, &p2}) {
    const std::vector<RtxSlotOps> u = updates_for(B0, *p, {});
    if (!rtx::flat_set_transforms("check", &fs, u.data(), (int64_t)u.size(), &err)) { fprintf(stderr, "full update: %s\n", err.c_str()); return 1; }
    Built Bf;
    rtx::FlatScene fresh;
    if (!flatten(*p, &Bf, &fresh)) return 1;
    bad += against_fresh(fs, fresh, first, "full update");
  }
  {
    const std::vector<RtxSlotOps> u = updates_for(B0, p0, {});
    if (!rtx::flat_set_transforms("check", &fs, u.data(), (int64_t)u.size(), &err)) { fprintf(stderr, "home: %s\n", err.c_str()); return 1; }
    bad += same_arrays(fs, first, "the original pose again") ? 0 : 1;
  }
  printf("full updates: %d failure(s)\n", bad);
  // partial sets: one member, three members, the medium outside the tree alone (no refit); the fresh scene has the rest at p0
  const std::vector<std::vector<int32_t>> parts = {{4}, {5, 8, 9}, {12}, {10, 12}};
  for (const std::vector<int32_t>& part : parts) {
    Pose mixed = p0;
    for (const auto& kv : B0.chain)
      for (int32_t s : part)
        if (s == kv.first)
          for (const auto& op : kv.second) { if (op.first == rt::XFORM_TRANSLATE) mixed.t[(size_t)op.second] = p1.t[(size_t)op.second]; else mixed.r[(size_t)op.second] = p1.r[(size_t)op.second]; }
    const std::vector<RtxSlotOps> u = updates_for(B0, mixed, part);
    if (u.size() != part.size()) { fprintf(stderr, "partial update: a slot of the part has no chain\n"); return 1; }
    if (!rtx::flat_set_transforms("check", &fs, u.data(), (int64_t)u.size(), &err)) { fprintf(stderr, "partial update: %s\n", err.c_str()); return 1; }
    Built Bf;
    rtx::FlatScene fresh;
    if (!flatten(mixed, &Bf, &fresh)) return 1;
    bad += against_fresh(fs, fresh, first, "partial update");
    const std::vector<RtxSlotOps> home = updates_for(B0, p0, part);
    if (!rtx::flat_set_transforms("check", &fs, home.data(), (int64_t)home.size(), &err)) return 1;
    bad += same_arrays(fs, first, "partial update undone") ? 0 : 1;
  }
  printf("partial updates: %d failure(s)\n", bad);
  // the ten refusals (a NULL scene and NULL updates are two arguments of one case)
  {
    std::vector<RtxSlotOps> ok = updates_for(B0, p1, {4, 5});
    std::vector<RtxSlotOps> u;
    bad += refused(nullptr, first, ok.data(), 2, "NULL", "a NULL scene");
    bad += refused(&fs, first, nullptr, 2, "NULL", "NULL updates");
    bad += refused(&fs, first, ok.data(), -1, "n < 0", "n < 0");
    u = ok; u[1].slot = 13;
    bad += refused(&fs, first, u.data(), 2, ".slot", "a slot out of range");
    u = ok; u[1].slot = -2;
    bad += refused(&fs, first, u.data(), 2, ".slot", "a negative slot");
    u = ok; u[1].slot = 2;
    bad += refused(&fs, first, u.data(), 2, "chain", "a slot without a chain");
    u = ok; u[0].n_ops = 1;
    bad += refused(&fs, first, u.data(), 2, ".n_ops", "a wrong n_ops");
    u = ok; u[0].n_ops = 5;
    bad += refused(&fs, first, u.data(), 2, ".n_ops", "n_ops past the struct");
    u = ok; u[0].ops[0].op = rt::XFORM_ROTATE_Y;
    bad += refused(&fs, first, u.data(), 2, ".op", "a wrong op kind");
    u = ok; u[0].ops[1].op = 9;
    bad += refused(&fs, first, u.data(), 2, ".op", "an unknown op kind");
    u = ok; u.push_back(ok[0]);
    bad += refused(&fs, first, u.data(), 3, "twice", "a slot named twice");
    u = ok; u[0].ops[0].v[2] = std::nan("");
    bad += refused(&fs, first, u.data(), 2, "not finite", "a NaN offset");
    u = ok; u[0].ops[1].v[0] = -INFINITY;
    bad += refused(&fs, first, u.data(), 2, "not finite", "an infinite angle");
    u = ok; u[0].ops[0].v[0] = 1.7976931348623157e308;
    bad += refused(&fs, first, u.data(), 2, "bounding box", "a member whose new box is not finite");
    if (!rtx::flat_set_transforms("check", &fs, ok.data(), 0, &err) || !same_arrays(fs, first, "n = 0")) ++bad;
  }
  printf("refusals: %d failure(s)\n", bad);
  // the device's narrowing is the converter's
  {
    const double xs[] = {0.0, -0.0, 1.0, -1.0, 0.1, -0.1, 1e-46, -1e-46, 1e-40, 3.4028234663852886e38, 3.5e38, -3.5e38, 1e300, -1e300,
                         16777217.0, -16777217.0, 0.3 + 1e-9, 5e-324, -5e-324, 1.0000000596046448, 1.4012984643e-45, 2.5e-45};
    for (double x : xs) {
      const float d0 = rtx::narrow_down(x), d1 = rt::f32_narrow_down(x), u0 = rtx::narrow_up(x), u1 = rt::f32_narrow_up(x);
      if (memcmp(&d0, &d1, 4) != 0 || memcmp(&u0, &u1, 4) != 0) { fprintf(stderr, "narrowing of %a differs\n", x); ++bad; }
      if (!((double)d1 <= x && x <= (double)u1)) { fprintf(stderr, "narrowing of %a is not outward\n", x); ++bad; }
    }
  }
  if (bad) { fprintf(stderr, "%d check(s) failed\n", bad); return 1; }
  printf("set_transforms host check clean\n");
  return 0;
}
