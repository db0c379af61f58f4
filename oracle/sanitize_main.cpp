// ORACLE -- TEST INFRASTRUCTURE.  AddressSanitizer / UndefinedBehaviorSanitizer run of everything that executes on the CPU:
// the product's HOST code (scene graph, catalogue, flattener, SAH and reference-rule BVH builders, time-aware boxes) and both CPU
// checkers (O1 literal, O2 flat), compiled by g++ with -fsanitize=address,undefined into one program (`make -C oracle sanitize`;
// GPU AddressSanitizer is not available on this pool).  It builds catalogue scenes and nested worlds, flattens them
// with every builder, renders small frames with O1 and O2 and insists that they agree bit for bit; any sanitizer report aborts
// the run with a non-zero status (tests/test_sanitizers.py).  The host checker of the denoiser's feature pass
// (tests/features_host_check.cpp, both builds) runs here too, on scenes with media, textures, a BVH and moving spheres.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../ray-tracing-series-rust_amd/csrc/host/flat_scene.hpp"
#include "../ray-tracing-series-rust_amd/csrc/host/scenes.hpp"
#include "oracle_abi.h"

extern "C" int oracle_audit_flat(const void* flat, int32_t* max_depth_out);
extern "C" int oracle_audit_flat_exact(const void* flat, const void* nodes, int64_t n_nodes, int32_t flags, int32_t cluster,
                                       int32_t* max_depth_out);
extern "C" int oracle_audit_motion(const void* flat, int32_t n_times, int64_t* checked);
extern "C" int oracle_lds_walk_render(const void* flat, const OracleCamera* cam, const OracleConfig* cfg, int32_t use_motion,
                                      int32_t row_stride, double* accum_rgb, uint64_t counts[3]);

// tests/features_host_check.cpp: the f64 build and the float judge
extern "C" int features_host(const void* flat, const double* camera24, const double* background3, int32_t width, int32_t height,
                             int32_t feature_spp, int32_t max_depth, uint64_t seed, float* albedo_rgb, float* normal_xyz, int32_t* hits);
extern "C" int features_host_f32(const void* flat, const double* camera24, const double* background3, int32_t width, int32_t height,
                                 int32_t feature_spp, int32_t max_depth, uint64_t seed, float* albedo_rgb, float* normal_xyz, int32_t* hits);

namespace rtx {
// the GPU builder lives in csrc/hip/lbvh.hip: not part of a CPU-only program
int32_t build_bvh_gpu(const std::vector<double>&, int, std::vector<rt::FlatNode>*, std::vector<uint32_t>*, int32_t*, double*, std::string* err) {
  if (err) *err = "no GPU builder in the sanitizer program";
  return -1;
}
}  // namespace rtx

static int check_scene(int32_t sid, int width, double aspect, int spp, bool reference_bvh) {
  rtx::SceneGraph g(1);
  rtx::SceneOptions opt;
  opt.mesh_triangles = 3000;
  opt.book2_boxes_per_side = 6;
  opt.book2_spheres = 60;
  rtx::WorldCam wc;
  std::string err;
  if (!rtx::get_world_cam(g, sid, opt, &wc, &err)) { fprintf(stderr, "scene %d: %s\n", sid, err.c_str()); return 1; }
  rtx::BuildOptions bo;
  bo.reference_bvh = reference_bvh ? 1 : 0;
  bo.bvh_seed = 5;
  rtx::FlatScene fs;
  if (!rtx::flatten_scene(g, wc.world, bo, &fs, &err)) { fprintf(stderr, "scene %d: flatten: %s\n", sid, err.c_str()); return 1; }
  int32_t depth = 0;
  // (the reference's build rule stores a span of one object twice, bvh.rs:53-55: "every primitive in exactly one leaf" does not hold there)
  if (!reference_bvh && oracle_audit_flat(&fs, &depth) != 0) { fprintf(stderr, "scene %d: audit_flat failed\n", sid); return 1; }
  if (!reference_bvh && oracle_audit_flat_exact(&fs, nullptr, 0, ORACLE_AUDIT_ASK_FIRST, 0, &depth) != 0) { fprintf(stderr, "scene %d: audit_flat_exact failed\n", sid); return 1; }
  int64_t checked = 0;
  if (oracle_audit_motion(&fs, 8, &checked) != 0) { fprintf(stderr, "scene %d: audit_motion failed\n", sid); return 1; }
  OracleCamera cam;
  static_assert(sizeof(cam) == sizeof(wc.cam), "camera layout");
  memcpy(&cam, &wc.cam, sizeof(cam));
  OracleConfig cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.image_width = width;
  cfg.image_height = (int32_t)((double)width / aspect);
  cfg.samples_per_pixel = spp;
  cfg.max_depth = 12;
  cfg.threads = 3;
  cfg.seed = 7;
  cfg.bvh_seed = 11;
  for (int a = 0; a < 3; ++a) cfg.background[a] = wc.background[a];
  const size_t n = (size_t)cfg.image_width * (size_t)cfg.image_height * 3;
  std::vector<double> a1(n), a2(n);
  std::vector<uint8_t> r1(n), r2(n);
  if (oracle_o1_render(&g, wc.world, &cam, &cfg, a1.data(), r1.data()) != 0) { fprintf(stderr, "scene %d: O1 failed\n", sid); return 1; }
  if (oracle_o2_render(&fs, &cam, &cfg, 0, 1, 1, a2.data(), r2.data(), nullptr) != 0) { fprintf(stderr, "scene %d: O2 failed\n", sid); return 1; }
  if (memcmp(a1.data(), a2.data(), n * sizeof(double)) != 0 || memcmp(r1.data(), r2.data(), n) != 0) {
    fprintf(stderr, "scene %d: O1 and O2 differ\n", sid);
    return 1;
  }
  if (fs.top_level.size() == 1 && fs.entries[fs.top_level[0]].kind == rt::ENTRY_BVH && fs.triangles.empty() && fs.rects.empty() && fs.gravity_spheres.empty()) {
    std::vector<double> a3(n);
    uint64_t counts[3];
    if (oracle_lds_walk_render(&fs, &cam, &cfg, fs.motion32.empty() ? 0 : 1, 1, a3.data(), counts) != 0 ||
        memcmp(a3.data(), a2.data(), n * sizeof(double)) != 0) { fprintf(stderr, "scene %d: the LDS walk differs\n", sid); return 1; }
  }
  if (!reference_bvh) {  // the float checker, both builds: the converter, the narrowed scene and the float core under the sanitizers
    std::vector<double> f1(n), f2(n);
    std::vector<uint8_t> q1(n), q2(n);
    double one[3];
    if (oracle_o2f_render(&fs, &cam, &cfg, 0, 1, 1, 0, f1.data(), q1.data()) != 0 ||
        oracle_o2g_render(&fs, &cam, &cfg, 0, 1, 1, 0, f2.data(), q2.data()) != 0 ||
        oracle_o2f_sample(&fs, &cam, &cfg, 0, 0, 0, one) != 0) { fprintf(stderr, "scene %d: O2f failed\n", sid); return 1; }
  }
  printf("scene %3d%s: %zu nodes, %zu entries, %d x %d x %d spp: O1 == O2\n", sid, reference_bvh ? " (reference BVH rule)" : "", fs.nodes.size(),
         fs.entries.size(), cfg.image_width, cfg.image_height, spp);
  return 0;
}

// The feature checker on a catalogue scene, three samples per pixel: both builds run, every pixel's hit count is within
// [0, 3], the two builds agree on nearly all of them, and a pixel no sample hit has no normal.
static int check_features(int32_t sid) {
  rtx::SceneGraph g(1);
  rtx::SceneOptions opt;
  opt.mesh_triangles = 2000;
  opt.book2_boxes_per_side = 4;
  opt.book2_spheres = 50;
  rtx::WorldCam wc;
  std::string err;
  if (!rtx::get_world_cam(g, sid, opt, &wc, &err)) { fprintf(stderr, "features, scene %d: %s\n", sid, err.c_str()); return 1; }
  rtx::BuildOptions bo;
  rtx::FlatScene fs;
  if (!rtx::flatten_scene(g, wc.world, bo, &fs, &err)) { fprintf(stderr, "features, scene %d: flatten: %s\n", sid, err.c_str()); return 1; }
  const int w = 33, h = 17, spp = 3;
  std::vector<float> a64(3 * w * h), n64(3 * w * h), a32(3 * w * h), n32(3 * w * h);
  std::vector<int32_t> h64(w * h), h32(w * h);
  if (features_host(&fs, (const double*)&wc.cam, wc.background, w, h, spp, 12, 7, a64.data(), n64.data(), h64.data()) != 0 ||
      features_host_f32(&fs, (const double*)&wc.cam, wc.background, w, h, spp, 12, 7, a32.data(), n32.data(), h32.data()) != 0) {
    fprintf(stderr, "features, scene %d: the checker failed\n", sid);
    return 1;
  }
  int same = 0, hit = 0;
  for (int p = 0; p < w * h; ++p) {
    if (h64[p] < 0 || h64[p] > spp || h32[p] < 0 || h32[p] > spp) { fprintf(stderr, "features, scene %d: hit count out of range\n", sid); return 1; }
    if (h64[p] == 0 && (n64[3 * p] != 0.f || n64[3 * p + 1] != 0.f || n64[3 * p + 2] != 0.f)) { fprintf(stderr, "features, scene %d: a normal without a hit\n", sid); return 1; }
    same += h64[p] == h32[p];
    hit += h64[p];
  }
  if (10 * same < 8 * w * h) { fprintf(stderr, "features, scene %d: the float judge disagrees on %d of %d pixels\n", sid, w * h - same, w * h); return 1; }
  printf("scene %3d: features of %d x %d x %d samples, %d hits, f32 and f64 counts agree on %d pixels\n", sid, w, h, spp, hit, same);
  return 0;
}

// The texture probes on a tree of every kind: a chain of 16 checkers (the longest the flattener admits) whose leaves are a
// 3 x 2 image, a noise texture and a solid colour.  O1, the f64 core and the float core are asked at points of both
// parities, at far and non-finite coordinates and at (u, v) on, beyond and not on the unit square; O1 and the f64 core must
// agree bit for bit.  One more checker on top must be refused once a sphere of the world wears it.
static int check_textures() {
  rtx::SceneGraph g(1);
  std::vector<double> texels;
  for (int k = 0; k < 3 * 2 * 3; ++k) texels.push_back((double)(10 * k + 1));
  const int32_t image = g.image_from_texels(3, 2, texels.data());
  const int32_t noise = g.noise(4.0);
  const double red[3] = {0.9, 0.1, 0.2};
  const int32_t solid = g.solid_color(red);
  int32_t t = g.checker(image, noise);
  for (int k = 1; k < 16; ++k) t = g.checker(k % 2 ? t : solid, k % 2 ? solid : t);
  const int32_t deep = g.checker(t, t);
  if (image < 0 || noise < 0 || solid < 0 || t < 0 || deep < 0) { fprintf(stderr, "textures: construction failed: %s\n", g.error.c_str()); return 1; }
  const double c[3] = {0.0, 0.0, 0.0};
  const int32_t world = g.list_new();
  g.list_add(world, g.sphere(c, 1.0, g.diffuse_light(t)));
  g.diffuse_light(deep);  // a material nothing wears: allowed
  rtx::BuildOptions bo;
  rtx::FlatScene fs;
  std::string err;
  if (!rtx::flatten_scene(g, world, bo, &fs, &err)) { fprintf(stderr, "textures: flatten: %s\n", err.c_str()); return 1; }
  const double big = 3.0e9, inf = 1.0 / 0.0, nan = inf - inf;
  const double pts[][3] = {{0.1, 0.2, 0.3}, {-0.1, 0.2, 0.3}, {0.4, -0.7, 12.5}, {big, -big, 0.5}, {1e15, 2.5, -1e15}, {inf, 0.0, 1.0}, {nan, 1.0, 1.0}, {0.0, -0.0, 5.0}};
  const double uvs[][2] = {{0.0, 0.0}, {1.0, 1.0}, {0.5, 0.34}, {-3.0, 7.0}, {nan, nan}, {inf, -inf}};
  int n = 0;
  for (const auto& p : pts)
    for (const auto& uv : uvs)
      for (int32_t tex : {image, noise, solid, t}) {
        double a[3], b[3], f[3];
        if (oracle_o1_texture_value(&g, tex, uv[0], uv[1], p, a) != 1 || oracle_core_texture_value(&fs, tex, uv[0], uv[1], p, b) != 1 ||
            oracle_core32_texture_value(&fs, tex, uv[0], uv[1], p, f) != 1) { fprintf(stderr, "textures: a probe failed\n"); return 1; }
        if (memcmp(a, b, sizeof(a)) != 0) { fprintf(stderr, "textures: O1 and the core differ on texture %d\n", tex); return 1; }
        ++n;
      }
  double out[3];
  if (oracle_o1_texture_value(&g, -1, 0, 0, c, out) != -1 || oracle_core_texture_value(&fs, (int32_t)fs.textures.size(), 0, 0, c, out) != -1) {
    fprintf(stderr, "textures: a bad index was not refused\n");
    return 1;
  }
  const int32_t world17 = g.list_new();
  g.list_add(world17, g.sphere(c, 1.0, g.diffuse_light(deep)));
  rtx::FlatScene fs17;
  if (rtx::flatten_scene(g, world17, bo, &fs17, &err) || err.find("17 deep") == std::string::npos) { fprintf(stderr, "textures: 17 checkers were not refused\n"); return 1; }
  printf("textures: %d probes, O1 == core; 17 checkers refused\n", n);
  return 0;
}

// The scatter probes on every material kind: a fuzzy and a clamped metal, glass on both faces and past the critical angle, a
// Lambertian, a light and the phase material of a medium; unit, short and long incident directions; several streams.  O1 and
// the f64 core must agree bit for bit on the verdict, the direction, the draws consumed and (where it scattered) the
// attenuation; the float core runs beside them.
static int check_scatter() {
  rtx::SceneGraph g(1);
  const double grey[3] = {0.5, 0.25, 1.0}, c[3] = {0.0, 0.0, 0.0};
  const int32_t mats[] = {g.lambertian(g.solid_color(grey)), g.metal(grey, 0.0), g.metal(grey, 0.3), g.metal(grey, 1.7), g.metal(grey, -0.5),
                          g.dielectric(1.5), g.dielectric(1.0), g.dielectric(1.0 / 1.5), g.diffuse_light(g.solid_color(grey))};
  const int32_t world = g.list_new();
  for (int32_t m : mats) g.list_add(world, g.sphere(c, 1.0, m));
  const int32_t fog = g.constant_medium(grey, 0.5, g.sphere(c, 2.0, mats[0]));
  g.list_add(world, fog);
  if (world < 0 || fog < 0) { fprintf(stderr, "scatter: construction failed: %s\n", g.error.c_str()); return 1; }
  rtx::BuildOptions bo;
  rtx::FlatScene fs;
  std::string err;
  if (!rtx::flatten_scene(g, world, bo, &fs, &err)) { fprintf(stderr, "scatter: flatten: %s\n", err.c_str()); return 1; }
  const double dirs[][3] = {{0.0, -1.0, 0.0}, {0.6, -0.8, 0.0}, {0.0007, -0.0001, 0.0002}, {6.9, -0.7, 0.4}, {0.999, -0.04, 0.0}};
  const double o[3] = {0.0, 1.0, 0.0}, n[3] = {0.0, 1.0, 0.0};
  int count = 0;
  for (int32_t m = 0; m < (int32_t)g.materials.size(); ++m)
    for (const auto& d : dirs)
      for (int ff = 0; ff < 2; ++ff)
        for (uint64_t seed = 1; seed <= 3; ++seed) {
          double a[7], b[7], f[7];
          const int ra = oracle_o1_scatter(&g, m, o, d, 0.25, c, n, ff, 0.5, 0.5, seed, a);
          const int rb = oracle_core_scatter(&fs, m, o, d, 0.25, c, n, ff, 0.5, 0.5, seed, b);
          const int rf = oracle_core32_scatter(&fs, m, o, d, 0.25, c, n, ff, 0.5, 0.5, seed, f);
          if (ra < 0 || rb < 0 || rf < 0) { fprintf(stderr, "scatter: a probe failed on material %d\n", m); return 1; }
          if (ra != rb || memcmp(a, b, 3 * sizeof(double)) != 0 || a[6] != b[6] || a[6] < 0.0 || (ra == 1 && memcmp(a + 3, b + 3, 3 * sizeof(double)) != 0)) {
            fprintf(stderr, "scatter: O1 and the core differ on material %d\n", m);
            return 1;
          }
          ++count;
        }
  double out[7];
  if (oracle_o1_scatter(&g, -1, o, dirs[0], 0.0, c, n, 1, 0, 0, 1, out) != -1 ||
      oracle_core_scatter(&fs, (int32_t)fs.materials.size(), o, dirs[0], 0.0, c, n, 1, 0, 0, 1, out) != -1) {
    fprintf(stderr, "scatter: a bad index was not refused\n");
    return 1;
  }
  printf("scatter: %d probes, O1 == core\n", count);
  return 0;
}

int main() {
  int bad = 0;
  bad += check_textures();
  bad += check_scatter();
  for (int32_t sid : {2, 5, 6, 7, 11}) bad += check_features(sid);  // image texture; box media; Book-2; moving spheres + lens; mesh
  const int32_t scenes[] = {0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 100, 101};
  for (int32_t sid : scenes) bad += check_scene(sid, 40, sid == 4 || sid == 5 || sid == 6 || sid == 12 ? 1.0 : 1.6, 2, false);
  for (int32_t sid : {6, 13, 100}) bad += check_scene(sid, 32, 1.0, 2, true);
  if (bad) { fprintf(stderr, "%d scene(s) failed\n", bad); return 1; }
  printf("feature checker clean\n");
  printf("sanitizer run clean\n");
  return 0;
}
