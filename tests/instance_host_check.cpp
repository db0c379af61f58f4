// Host checker of instance trees (tests/test_instance_tree.py, tests/test_sanitizers.py).  Two uses of one file:
//   * as a shared object (g++ -shared): instance_host_array hands the box audit the arrays oracle_flat_array does not name
//     (top_level, refs, nodes32, top_box32);
//   * with -DINSTANCE_HOST_MAIN, linked with the product's host sources under -fsanitize=address,undefined: it builds a member
//     zoo in every slot layout through the scene-graph API (a SUBSET of tests/instance_scenes.py written again in C++: every
//     member kind and every chain length, fewer members, other neighbours in "one" and "empty"; nothing holds the two together),
//     flattens both spellings and the refusal cases, and sends a few thousand rays through world_hit<F_ALL>, insisting that the
//     instanced and the hoisted spelling agree byte for byte.  member_world_box, emit_instance and instance_walk run here.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../ray-tracing-series-rust_amd/csrc/core/integrator.hpp"
#include "../ray-tracing-series-rust_amd/csrc/host/flat_scene.hpp"

extern "C" const void* instance_host_array(const void* flat, const char* name, int64_t* n, int64_t* elem_bytes) {
  const rtx::FlatScene& fs = *(const rtx::FlatScene*)flat;
#define ARR(VEC) if (!strcmp(name, #VEC)) { *n = (int64_t)fs.VEC.size(); *elem_bytes = (int64_t)sizeof(fs.VEC[0]); return fs.VEC.data(); }
  ARR(top_level) ARR(refs) ARR(nodes32) ARR(top_box32)
#undef ARR
  *n = 0; *elem_bytes = 0;
  return nullptr;
}

#ifdef INSTANCE_HOST_MAIN
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

struct Zoo {
  rtx::SceneGraph g{13};
  int32_t grey, red, glass, metal, checker, noise, image, light;
  Zoo() {
    const V c1 = v3(0.5, 0.5, 0.5), c2 = v3(0.8, 0.2, 0.2), c3 = v3(0.1, 0.3, 0.1), c4 = v3(0.9, 0.9, 0.9), c5 = v3(6, 6, 5);
    grey = g.lambertian(g.solid_color(c1.v));
    red = g.lambertian(g.solid_color(c2.v));
    glass = g.dielectric(1.5);
    metal = g.metal(c4.v, 0.2);
    checker = g.lambertian(g.checker(g.solid_color(c3.v), g.solid_color(c4.v)));
    noise = g.lambertian(g.noise(4.0));
    std::vector<double> tex(3 * 8 * 4);
    for (size_t k = 0; k < tex.size(); ++k) tex[k] = (double)((5 * k + 3) % 11) / 11.0;
    image = g.lambertian(g.image_from_texels(8, 4, tex.data()));
    light = g.diffuse_light(g.solid_color(c5.v));
  }
  int32_t list(const std::vector<int32_t>& objs) {
    const int32_t l = g.list_new();
    for (int32_t o : objs) g.list_add(l, o);
    return l;
  }
  int32_t sphere(double x, double y, double z, double r, int32_t m) { return g.sphere(v3(x, y, z).v, r, m); }
  int32_t prism(double x0, double y0, double z0, double x1, double y1, double z1, int32_t m) { return g.rect_prism(v3(x0, y0, z0).v, v3(x1, y1, z1).v, m); }
  int32_t move(double x, double y, double z, int32_t o) { return g.translate(v3(x, y, z).v, o); }
  int32_t ball_row(double x0, double z, int n, int32_t m) {
    std::vector<int32_t> s;
    for (int k = 0; k < n; ++k) s.push_back(sphere(x0 + 0.7 * k, 0.3 + 0.02 * k, z + 0.1 * (k % 2), 0.3, m));
    return g.bvh_from_list(list(s), 0.0, 1.0);
  }
  int32_t fan(double x0, double z, int32_t m) {
    std::vector<int32_t> t;
    for (int k = 0; k < 6; ++k)
      t.push_back(g.triangle(v3(x0 + 0.5 * k, 0.05, z).v, v3(x0 + 0.5 * k + 0.45, 0.05, z + 0.03 + 0.1 * (k % 3)).v, v3(x0 + 0.5 * k + 0.2, 0.9, z - 0.07 - 0.05 * k).v, m));
    return g.bvh_from_list(list(t), 0.0, 1.0);
  }
  std::vector<int32_t> members() {
    std::vector<int32_t> m;
    m.push_back(ball_row(-4.5, -1.5, 6, red));
    m.push_back(sphere(-4.0, 0.6, 1.0, 0.6, checker));
    m.push_back(g.rect(rtx::H_XY_RECT, -3.0, -2.0, 0.2, 1.2, -0.5, noise));
    m.push_back(g.rect(rtx::H_XZ_RECT, -2.5, -1.5, 0.5, 1.5, 0.4, metal));
    m.push_back(g.rect(rtx::H_YZ_RECT, 0.2, 1.2, 0.0, 1.0, -1.2, image));
    m.push_back(g.triangle(v3(-1.0, 0.1, 1.5).v, v3(0.0, 0.1, 1.5).v, v3(-0.5, 1.1, 1.2).v, red));
    m.push_back(sphere(1.0, 0.7, 1.2, 0.7, glass));
    m.push_back(sphere(1.0, 0.7, 1.2, -0.6, glass));  // the hollow-glass idiom: an inverted reference box
    m.push_back(sphere(2.3, 0.5, 1.2, 0.5, grey));
    m.push_back(prism(3.0, 0.0, 0.5, 3.8, 0.9, 1.3, grey));
    m.push_back(list({sphere(4.6, 0.4, 1.0, 0.4, metal), g.rect(rtx::H_XZ_RECT, 4.2, 5.0, 1.5, 2.1, 0.3, red)}));
    m.push_back(fan(-1.0, -0.6, grey));
    m.push_back(move(2.0, 0.1, -2.2, g.rotate_y(37.0, ball_row(-1.0, 0.0, 5, grey))));
    m.push_back(move(4.4, 0.0, -0.6, g.rotate_y(-52.0, fan(-1.2, 0.0, checker))));
    m.push_back(g.rotate_y(0.0, prism(-5.6, 0.0, -0.4, -5.0, 0.7, 0.6, noise)));
    m.push_back(move(-2.4, 0.0, -2.8, g.rotate_y(90.0, prism(-0.3, 0.0, -0.5, 0.3, 0.7, 0.5, red))));
    m.push_back(move(0.2, 0.0, -2.0, g.rotate_y(180.0, move(0.0, 0.5, 1.0, sphere(0.0, 0.0, 0.0, 0.45, glass)))));
    m.push_back(move(5.4, 0.0, -2.6, g.rotate_y(33.0, move(0.1, 0.0, 0.0, g.rotate_y(-17.0, prism(-0.3, 0.0, -0.5, 0.3, 0.7, 0.5, checker))))));
    m.push_back(sphere(0.0, 4.2, 0.0, 0.7, light));
    m.push_back(prism(-5.0, 0.0, -4.4, -4.0, 0.8, -3.6, red));
    m.push_back(g.bvh_from_list(list({prism(-4.5, 0.0, -4.4, -3.5, 0.8, -3.6, grey), sphere(-4.0, 1.3, -4.0, 0.2, grey)}), 0.0, 1.0));  // coincident top faces
    m.push_back(move(-3.6, 0.0, -2.8, prism(-0.3, 0.0, -0.5, 0.3, 0.7, 0.5, image)));  // one op, a Translate
    m.push_back(g.rotate_y(180.0, move(1.2, 0.0, 2.8, prism(-0.3, 0.0, -0.5, 0.3, 0.7, 0.5, metal))));
    m.push_back(move(-5.2, 0.0, 1.9, g.rotate_y(90.0, g.rect(rtx::H_XY_RECT, -0.5, 0.5, 0.1, 0.9, 0.0, grey))));
    m.push_back(g.bvh_from_list(list({prism(3.5, 0.0, -4.4, 4.5, 0.8, -3.6, grey), sphere(4.0, 1.3, -4.0, 0.2, grey)}), 0.0, 1.0));  // the tie pair, BVH first
    m.push_back(prism(4.0, 0.0, -4.4, 5.0, 0.8, -3.6, red));
    return m;
  }
};

const char* const kLayouts[] = {"middle", "first", "after_bvh", "last", "alone", "two", "pair", "one", "empty"};

// the world of one layout; instanced: the runs marked as trees become instance trees, else their members are listed in place
int32_t make_world(Zoo& z, const std::string& layout, bool instanced) {
  const std::vector<int32_t> zoo = z.members();
  const int32_t ground = z.sphere(0.0, -500.0, 0.0, 500.0, z.grey), s1 = z.sphere(0.0, 0.5, 2.6, 0.5, z.grey);
  const int32_t plain_bvh = z.ball_row(5.5, 2.0, 3, z.grey);
  std::vector<int32_t> slots;
  auto plain = [&](std::initializer_list<int32_t> o) { slots.insert(slots.end(), o.begin(), o.end()); };
  auto tree = [&](const std::vector<int32_t>& ms) {
    if (instanced) slots.push_back(z.g.instance_bvh_from_list(z.list(ms)));
    else slots.insert(slots.end(), ms.begin(), ms.end());
  };
  if (layout == "middle") { plain({ground}); tree(zoo); plain({s1}); }
  else if (layout == "first") { tree(zoo); plain({ground, s1}); }
  else if (layout == "after_bvh") { plain({plain_bvh}); tree(zoo); plain({ground}); }
  else if (layout == "last") { plain({ground, s1}); tree(zoo); }
  else if (layout == "alone") return instanced ? z.g.instance_bvh_from_list(z.list(zoo)) : z.list(zoo);
  else if (layout == "two") {
    tree(std::vector<int32_t>(zoo.begin(), zoo.begin() + 11)); plain({ground, s1});
    tree(std::vector<int32_t>(zoo.begin() + 11, zoo.end())); plain({plain_bvh});
  } else if (layout == "pair") {
    const int32_t ball = z.sphere(2.4, 0.6, 2.4, 0.6, z.glass);
    std::vector<int32_t> ms = zoo;
    ms.push_back(ball);
    const V fog = v3(0.2, 0.4, 0.9);
    plain({ground}); tree(ms); plain({z.g.constant_medium(fog.v, 0.8, ball), s1});
  } else {
    plain({ground});
    tree(layout == "one" ? std::vector<int32_t>{zoo[12]} : std::vector<int32_t>{});
    plain({s1, plain_bvh, zoo[1], zoo[9]});
  }
  return z.list(slots);
}

struct Rec { int hit; rt::HitRecord rec; };

int run_layout(const std::string& layout, int n_rays, long* hits_out) {
  rtx::FlatScene fs[2];
  for (int inst = 0; inst < 2; ++inst) {
    Zoo z;
    std::string err;
    if (!rtx::flatten_scene(z.g, make_world(z, layout, inst == 1), rtx::BuildOptions(), &fs[inst], &err)) {
      fprintf(stderr, "layout %s (%s): flatten: %s\n", layout.c_str(), inst ? "instanced" : "hoisted", err.c_str());
      return 1;
    }
  }
  if (fs[0].top_level.size() != fs[1].top_level.size()) { fprintf(stderr, "layout %s: the spellings differ in slots\n", layout.c_str()); return 1; }
  rt::HostRng pick{99};
  auto uni = [&]() { return (double)(rt::host_rng_next_u64(pick) >> 11) * 0x1.0p-53; };
  long hits = 0;
  for (int k = 0; k < n_rays; ++k) {
    const rt::Vec3 o = rt::v3(-7.0 + 14.0 * uni(), 0.05 + 5.0 * uni(), -6.0 + 12.0 * uni());
    const rt::Vec3 to = rt::v3(-5.5 + 11.0 * uni(), 0.9 * uni(), -4.4 + 7.0 * uni());
    rt::Vec3 d = to - o;
    if (k % 7 == 0) d.x = 0.0;  // axis-parallel components: 1 / d = inf in the culling ray
    if (k % 11 == 0) d.z = 0.0;
    Rec got[2];
    for (int inst = 0; inst < 2; ++inst) {
      const rt::SceneView sv = fs[inst].view();
      rt::LocalStack<128> stack;
      stack.reset();
      rt::Rng rng = rt::rng_for_sample(3, (uint64_t)k, 0);
      memset(&got[inst], 0, sizeof(Rec));
      rt::HitRecord rec;
      memset(&rec, 0, sizeof(rec));
      got[inst].hit = rt::world_hit<rt::F_ALL, false>(sv, rt::make_ray(o, d, 0.0), 0.001, RT_INFINITY, &rec, rng, stack, nullptr) ? 1 : 0;
      if (got[inst].hit) memcpy(&got[inst].rec, &rec, sizeof(rec));
    }
    if (got[0].hit != got[1].hit || (got[0].hit && (memcmp(&got[0].rec.t, &got[1].rec.t, sizeof(got[0].rec.t)) != 0 ||
                                                     memcmp(&got[0].rec.p, &got[1].rec.p, sizeof(got[0].rec.p)) != 0 ||
                                                     memcmp(&got[0].rec.normal, &got[1].rec.normal, sizeof(got[0].rec.normal)) != 0 ||
                                                     got[0].rec.mat != got[1].rec.mat || got[0].rec.front_face != got[1].rec.front_face))) {
      fprintf(stderr, "layout %s: ray %d: the instanced and the hoisted spelling differ\n", layout.c_str(), k);
      return 1;
    }
    hits += got[0].hit;
  }
  *hits_out = hits;
  return 0;
}

// a world the flattener must refuse, with a message (tests/test_instance_tree.py: test_refusals_name_the_cause...)
int refused(rtx::SceneGraph& g, int32_t world, const char* what) {
  rtx::FlatScene fs;
  std::string err;
  if (rtx::flatten_scene(g, world, rtx::BuildOptions(), &fs, &err) || err.empty()) { fprintf(stderr, "not refused: %s\n", what); return 1; }
  return 0;
}

int run_refusals() {
  Zoo z;
  rtx::SceneGraph& g = z.g;
  const int32_t s = z.sphere(0, 0, 0, 1.0, z.grey), s2 = z.sphere(3, 0, 0, 1.0, z.grey);
  const int32_t tree = g.instance_bvh_from_list(z.list({s, s2}));
  const V white = v3(1, 1, 1), a = v3(0, 0, 0), up = v3(0, 1, 0), st = v3(0, 3, 0);
  const int32_t moving = g.moving_sphere(a.v, up.v, 0.0, 1.0, 0.5, z.grey);
  int bad = 0;
  bad += refused(g, z.list({g.instance_bvh_from_list(z.list({g.constant_medium(white.v, 0.1, s), s2}))}), "a medium member");
  bad += refused(g, z.list({g.instance_bvh_from_list(z.list({z.move(1, 0, 0, moving), s2}))}), "a moving member");
  bad += refused(g, z.list({g.instance_bvh_from_list(z.list({g.bvh_from_list(z.list({moving, s}), 0.0, 1.0), s2}))}), "a BVH of a moving sphere");
  bad += refused(g, z.list({g.instance_bvh_from_list(z.list({g.gravity_sphere(st.v, 0.0, 0.5, z.grey), s2}))}), "a gravity sphere");
  bad += refused(g, z.list({g.instance_bvh_from_list(z.list({tree, s2}))}), "a tree in a tree");
  bad += refused(g, z.list({z.move(1, 0, 0, tree)}), "a tree under a Translate");
  bad += refused(g, z.list({g.rotate_y(10.0, tree)}), "a tree under a RotateY");
  bad += refused(g, z.list({g.constant_medium(white.v, 0.1, tree)}), "a tree under a medium");
  bad += refused(g, z.list({g.bvh_from_list(z.list({tree, s2}), 0.0, 1.0)}), "a tree in a BvhNode");
  bad += refused(g, g.bvh_from_list(z.list({g.rotate_y(20.0, s), s2}), 0.0, 1.0), "a BvhNode of wrapped members");
  return bad;
}
}  // namespace

int main() {
  int bad = 0;
  for (const char* layout : kLayouts) {
    long hits = 0;
    const int n = 600;
    if (run_layout(layout, n, &hits)) { bad++; continue; }
    printf("layout %-9s: %d rays, %ld hit: instanced == hoisted\n", layout, n, hits);
    if (4 * hits < n) { fprintf(stderr, "layout %s: fewer than a quarter of the rays hit\n", layout); bad++; }
  }
  bad += run_refusals();
  if (bad) { fprintf(stderr, "%d check(s) failed\n", bad); return 1; }
  printf("instance host check clean\n");
  return 0;
}
#endif
