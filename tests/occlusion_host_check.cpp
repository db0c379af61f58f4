// Host checker of occlusion queries (tests/test_occlusion_cases.py, tests/test_gpu_occlusion.py): the shared core's
// world_occlusion<rt::F_ALL> (core/occlusion.hpp) compiled for the CPU with the flags oracle/Makefile gives the O2 checker,
// driven by a plain loop over rays.  k_occlusion must equal it bit for bit.
//
// Built three ways:
//   as it is                 occlusion_host over the f64 flat scene (rtx_flat_arrays);
//   -DOCCLUSION_HOST_F32     the float judge: the four defines of oracle/o2_flat_f32.cpp (RT_F32, RT_REAL, rt, rtx), the scene
//                            narrowed by the product's converter through oracle_f32_images (liboracle.so), the ray, t_min and
//                            t_max narrowed with the casts k_occlusion uses, tau widened;
//   -DOCCLUSION_HOST_MAIN    the f64 build plus a main over two catalogue scenes: the stand-alone program the sanitizer test runs.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#ifdef OCCLUSION_HOST_F32
#include "../ray-tracing-series-rust_amd/csrc/host/f32_blobs.hpp"
#define RT_F32 1
#define RT_REAL float
#define rt rt32
#define rtx rtx32
#include "../ray-tracing-series-rust_amd/csrc/core/cull32.hpp"
#endif
#include "../ray-tracing-series-rust_amd/csrc/core/occlusion.hpp"
#include "../ray-tracing-series-rust_amd/csrc/host/flat_scene.hpp"

#ifdef OCCLUSION_HOST_F32
extern "C" int oracle_f32_images(const void* flat, RtxF32Blobs* blobs, void** keep);
extern "C" void oracle_f32_images_free(void* keep);

namespace {
template <class T>
bool take_blob(const RtxF32Blobs& b, int which, std::vector<T>* out) {  // csrc/hip/f32_entry.inc
  if (b.bytes[which] == 0) { out->clear(); return true; }
  if (b.elem_bytes[which] != sizeof(T) || b.bytes[which] % sizeof(T) != 0) return false;
  out->resize(b.bytes[which] / sizeof(T));
  memcpy((void*)out->data(), b.data[which], b.bytes[which]);
  return true;
}

bool narrow_scene(const void* flat, rtx::FlatScene* fs) {  // oracle/o2_flat_f32.cpp
  RtxF32Blobs b;
  void* keep = nullptr;
  if (oracle_f32_images(flat, &b, &keep) != 0) { oracle_f32_images_free(keep); return false; }
  bool ok = take_blob(b, RTX32_SPHERES, &fs->spheres) && take_blob(b, RTX32_MOVING_SPHERES, &fs->moving_spheres) &&
            take_blob(b, RTX32_RECTS, &fs->rects) && take_blob(b, RTX32_TRIANGLES, &fs->triangles) &&
            take_blob(b, RTX32_NODES, &fs->nodes) && take_blob(b, RTX32_NODES32, &fs->nodes32) &&
            take_blob(b, RTX32_REFS, &fs->refs) && take_blob(b, RTX32_ENTRIES, &fs->entries) &&
            take_blob(b, RTX32_TOP_LEVEL, &fs->top_level) && take_blob(b, RTX32_MATERIALS, &fs->materials) &&
            take_blob(b, RTX32_TEXTURES, &fs->textures) && take_blob(b, RTX32_PERLINS, &fs->perlins) &&
            take_blob(b, RTX32_IMAGES, &fs->images) && take_blob(b, RTX32_TEXELS, &fs->texels) &&
            take_blob(b, RTX32_TOP_BOX32, &fs->top_box32) && take_blob(b, RTX32_GRAVITY_SPHERES, &fs->gravity_spheres) &&
            take_blob(b, RTX32_GRAVITY_Y, &fs->gravity_y) && take_blob(b, RTX32_MOTION32, &fs->motion32);
  fs->max_stack = b.max_stack;
  fs->n_bvh = b.n_bvh;
  fs->features = b.features;
  oracle_f32_images_free(keep);
  return ok;
}
}  // namespace
#define OCCLUSION_HOST_ENTRY occlusion_host_f32
#else
#define OCCLUSION_HOST_ENTRY occlusion_host
#endif

// tau of rays 0 .. n - 1 (time NULL: 0; t_max NULL: t_max_all).  A ray later than the GravitySpheres' time limit (render.hip:
// gravity_time_limit) is not tested: NaN.  0 on success.
extern "C" int OCCLUSION_HOST_ENTRY(const void* flat, int64_t n, const double* origin, const double* direction, const double* time,
                                    const double* t_max, double t_min, double t_max_all, double* tau) {
  if (!flat || n < 0 || (n > 0 && (!origin || !direction)) || !tau) return 1;
#ifdef OCCLUSION_HOST_F32
  rtx::FlatScene narrowed;
  if (!narrow_scene(flat, &narrowed)) return 2;
  const rtx::FlatScene& fs = narrowed;
#else
  const rtx::FlatScene& fs = *(const rtx::FlatScene*)flat;
#endif
  const rt::SceneView sv = fs.view();
  double time_limit = 1e300;
  for (const rt::FlatGravitySphere& g : fs.gravity_spheres) time_limit = std::fmin(time_limit, (double)g.table_len * 0.001 + 10.0);
  std::vector<rt::LocalStack<256>> stack(1);
  for (int64_t r = 0; r < n; ++r) {
    const double t = time ? time[r] : 0.0;
    const double tm = t_max ? t_max[r] : t_max_all;
    if (t > time_limit) { tau[r] = std::nan(""); continue; }
    const rt::Ray ray = rt::make_ray(rt::v3((rt::real)origin[3 * r], (rt::real)origin[3 * r + 1], (rt::real)origin[3 * r + 2]),
                                     rt::v3((rt::real)direction[3 * r], (rt::real)direction[3 * r + 1], (rt::real)direction[3 * r + 2]),
                                     (rt::real)t);
    stack[0].reset();
    tau[r] = (double)rt::world_occlusion<rt::F_ALL>(sv, ray, (rt::real)t_min, (rt::real)tm, stack[0]);
  }
  return 0;
}

#ifdef OCCLUSION_HOST_MAIN
#include "../ray-tracing-series-rust_amd/csrc/host/scenes.hpp"

namespace rtx {
// the GPU builder lives in csrc/hip/lbvh.hip: not part of a CPU-only program
int32_t build_bvh_gpu(const std::vector<double>&, int, std::vector<rt::FlatNode>*, std::vector<uint32_t>*, int32_t*, double*, std::string* err) {
  if (err) *err = "no GPU builder in this program";
  return -1;
}
}  // namespace rtx

// A fan of rays from the scene's camera position towards a grid around its view direction, unbounded and cut short; a batch
// cut in two equals the whole.
static int check_scene(int32_t sid) {
  rtx::SceneGraph g(1);
  rtx::SceneOptions opt;
  opt.mesh_triangles = 2000;
  opt.book2_boxes_per_side = 4;
  opt.book2_spheres = 50;
  rtx::WorldCam wc;
  std::string err;
  if (!rtx::get_world_cam(g, sid, opt, &wc, &err)) { fprintf(stderr, "scene %d: %s\n", sid, err.c_str()); return 1; }
  rtx::BuildOptions bo;
  rtx::FlatScene fs;
  if (!rtx::flatten_scene(g, wc.world, bo, &fs, &err)) { fprintf(stderr, "scene %d: flatten: %s\n", sid, err.c_str()); return 1; }
  const double* cam = (const double*)&wc.cam;  // origin, lower_left_corner, horizontal, vertical, ... (FlatCamera's order)
  const int side = 24, n = side * side;
  std::vector<double> o(3 * n), d(3 * n), tm(n), reach(n);
  for (int j = 0; j < side; ++j)
    for (int i = 0; i < side; ++i) {
      const int r = j * side + i;
      const double u = (i + 0.5) / side, v = (j + 0.5) / side;
      for (int c = 0; c < 3; ++c) {
        o[3 * r + c] = cam[c];
        d[3 * r + c] = cam[3 + c] + u * cam[6 + c] + v * cam[9 + c] - cam[c];
      }
      tm[r] = 0.25 + 0.5 * u;
      reach[r] = (r % 3 == 0) ? INFINITY : 0.2 + 1.5 * v;
    }
  std::vector<double> whole(n), parts(n);
  if (occlusion_host(&fs, n, o.data(), d.data(), tm.data(), reach.data(), 0.001, INFINITY, whole.data()) != 0) return 1;
  const int cut = 211;
  if (occlusion_host(&fs, cut, o.data(), d.data(), tm.data(), reach.data(), 0.001, INFINITY, parts.data()) != 0 ||
      occlusion_host(&fs, n - cut, o.data() + 3 * cut, d.data() + 3 * cut, tm.data() + cut, reach.data() + cut, 0.001, INFINITY,
                     parts.data() + cut) != 0)
    return 1;
  int bad = 0;
  if (memcmp(whole.data(), parts.data(), n * sizeof(double)) != 0) { fprintf(stderr, "scene %d: a split batch differs from the whole\n", sid); ++bad; }
  int blocked = 0, fog = 0, clear = 0;
  for (double x : whole) {
    if (std::isinf(x)) ++blocked; else if (x > 0.0) ++fog; else if (x == 0.0) ++clear; else ++bad;
  }
  printf("scene %3d: %d rays, %d blocked, %d through fog, %d clear\n", sid, n, blocked, fog, clear);
  return bad;
}

int main() {
  int bad = 0;
  for (int32_t sid : {5, 6}) bad += check_scene(sid);  // Cornell smoke (two fog boxes); Book-2 final, reduced (fog spheres)
  if (bad) { fprintf(stderr, "%d check(s) failed\n", bad); return 1; }
  printf("occlusion_host_check: sanitizer run clean\n");
  return 0;
}
#endif
