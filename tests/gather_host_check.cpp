// Host checker of gather queries (tests/test_gather_abi.py, tests/test_gpu_gather.py): the shared core's trace_gather_sample /
// trace_gather_sample_nee (core/integrator.hpp) compiled for the CPU with the flags oracle/Makefile gives the O2 checker, driven
// by a plain loop over points and samples.  Plain sums: a point's samples are summed in sample order and their squares the way
// k_reduce_samples_moments sums them (square and add separately rounded).  Spherical-harmonic sums: for s ascending, i = 0 .. K-1,
// c = 0 .. 2, v = Y_i(dir_s) * L_s[c]; S += v; Q += v * v with core/sh_basis.hpp's Y on the sample's start direction, drawn
// again from the sample's stream as k_reduce_samples_sh draws it.  The light table is built by the same host code the upload
// uses (host/light_table.hpp).  k_gather and k_reduce_samples_sh must equal it bit for bit.
//
// Built three ways:
//   as it is              gather_host_trace over the f64 flat scene (rtx_flat_arrays);
//   -DGATHER_HOST_F32     the float judge: the four defines of oracle/o2_flat_f32.cpp (RT_F32, RT_REAL, rt, rtx), the scene narrowed
//                         by the product's converter through oracle_f32_images (liboracle.so), the point, the normal and the
//                         background narrowed with the casts k_gather and make_params use, every float sample and direction
//                         widened before it is used;
//   -DGATHER_HOST_MAIN    the f64 build plus a main that builds two catalogue scenes and gathers at a few points in both forms,
//                         with both estimators and with SH sums: the stand-alone program the sanitizer test runs.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#ifdef GATHER_HOST_F32
#include "../ray-tracing-series-rust_amd/csrc/host/f32_blobs.hpp"
#define RT_F32 1
#define RT_REAL float
#define rt rt32
#define rtx rtx32
#include "../ray-tracing-series-rust_amd/csrc/core/cull32.hpp"
#endif
#include "../ray-tracing-series-rust_amd/csrc/core/integrator.hpp"
#include "../ray-tracing-series-rust_amd/csrc/core/sh_basis.hpp"
#include "../ray-tracing-series-rust_amd/csrc/host/flat_scene.hpp"
#ifndef GATHER_HOST_F32
#include "../ray-tracing-series-rust_amd/csrc/host/light_table.hpp"
#endif

#ifdef GATHER_HOST_F32
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
#define GATHER_HOST_ENTRY gather_host_trace_f32
#else
#define GATHER_HOST_ENTRY gather_host_trace
#endif

// Samples first_sample .. first_sample + samples - 1 of points 0 .. n - 1; point r's stream key is (seed, first_point + r, sample).
// normal NULL: the probe form.  sh_order 0: sum / sumsq are [n][3]; 1 | 2 (probe form only): [n][K][3] with K = 4 | 9.
// accumulate != 0 continues sum / sumsq in place.  sumsq may be NULL.  A point later than the GravitySpheres' time limit
// (render.hip: gravity_time_limit) is not traced: NaN samples.  0 on success.
extern "C" int GATHER_HOST_ENTRY(const void* flat, int64_t n, const double* position, const double* normal, const double* time,
                                 uint64_t first_point, uint32_t first_sample, int32_t samples, int32_t max_depth, int32_t accumulate,
                                 uint64_t seed, const double* background3, int32_t light_sampling, int32_t sh_order, double* sum,
                                 double* sumsq) {
  if (!flat || n < 0 || (n > 0 && !position) || !background3 || !sum || samples < 1 || max_depth < 1) return 1;
  if (sh_order < 0 || sh_order > RT_SH_MAX_ORDER || (sh_order > 0 && normal)) return 1;
#ifdef GATHER_HOST_F32
  if (light_sampling) return 3;  // the f32 mode has no light sampling
  rtx::FlatScene narrowed;
  if (!narrow_scene(flat, &narrowed)) return 2;
  const rtx::FlatScene& fs = narrowed;
#else
  const rtx::FlatScene& fs = *(const rtx::FlatScene*)flat;
  const rtx::LightTable lt = rtx::build_light_table(fs);
  const rt::LightView lv = {lt.lights.data(), lt.slot_light.data(), (int32_t)lt.lights.size(), 0};
#endif
  const rt::SceneView sv = fs.view();
  double time_limit = 1e300;
  for (const rt::FlatGravitySphere& g : fs.gravity_spheres) time_limit = std::fmin(time_limit, (double)g.table_len * 0.001 + 10.0);
  rt::RenderParams rp;
  memset(&rp, 0, sizeof(rp));
  rp.background = rt::v3((rt::real)background3[0], (rt::real)background3[1], (rt::real)background3[2]);
  rp.samples_per_pixel = samples;
  rp.max_depth = max_depth;
  rp.seed = seed;
  const bool surface = normal != nullptr;
  const int K = sh_order > 0 ? sh_coeffs(sh_order) : 1;
  const int W = 3 * K;
  std::vector<rt::LocalStack<256>> stack(1);
  for (int64_t r = 0; r < n; ++r) {
    double* S = sum + (int64_t)W * r;
    double* Q = sumsq ? sumsq + (int64_t)W * r : nullptr;
    double s[3 * RT_SH_MAX_COEFFS], q[3 * RT_SH_MAX_COEFFS];
    for (int k = 0; k < W; ++k) {
      s[k] = accumulate ? S[k] : 0.0;
      q[k] = (accumulate && Q) ? Q[k] : 0.0;
    }
    const double t = time ? time[r] : 0.0;
    const rt::Point3 p = rt::v3((rt::real)position[3 * r], (rt::real)position[3 * r + 1], (rt::real)position[3 * r + 2]);
    rt::Vec3 nn = rt::v3(0, 0, 0);
    if (surface) nn = rt::v3((rt::real)normal[3 * r], (rt::real)normal[3 * r + 1], (rt::real)normal[3 * r + 2]);
    for (int32_t k = 0; k < samples; ++k) {
      const uint64_t index = first_point + (uint64_t)r;
      const uint32_t sample = first_sample + (uint32_t)k;
      double x[3];
      if (t > time_limit) {
        x[0] = x[1] = x[2] = std::nan("");
      } else {
        stack[0].reset();
        rt::Color c;
#ifndef GATHER_HOST_F32
        if (light_sampling)
          c = rt::trace_gather_sample_nee<rt::F_ALL, false>(sv, lv, rp, p, nn, surface, (rt::real)t, index, sample, stack[0],
                                                            (rt::TraceCounters*)nullptr);
        else
#endif
          c = rt::trace_gather_sample<rt::F_ALL, false>(sv, rp, p, nn, surface, (rt::real)t, index, sample, stack[0],
                                                        (rt::TraceCounters*)nullptr);
        x[0] = (double)c.x; x[1] = (double)c.y; x[2] = (double)c.z;  // store_sample widens
      }
      if (sh_order == 0) {
        for (int c = 0; c < 3; ++c) {
          s[c] += x[c];
          const double sq = x[c] * x[c];  // (-ffp-contract=off: the square and the add are separately rounded)
          q[c] = q[c] + sq;
        }
      } else {
        const rt::Vec3 d = rt::gather_sample_direction(seed, index, sample, false, rt::v3(0, 0, 0));
        double Y[RT_SH_MAX_COEFFS];
        sh_basis_eval(sh_order, (double)d.x, (double)d.y, (double)d.z, Y);
        for (int i = 0; i < K; ++i)
          for (int c = 0; c < 3; ++c) {
            const double v = Y[i] * x[c];
            s[3 * i + c] = s[3 * i + c] + v;
            const double sq = v * v;
            q[3 * i + c] = q[3 * i + c] + sq;
          }
      }
    }
    for (int k = 0; k < W; ++k) { S[k] = s[k]; if (Q) Q[k] = q[k]; }
  }
  return 0;
}

#ifdef GATHER_HOST_MAIN
#include "../ray-tracing-series-rust_amd/csrc/host/scenes.hpp"

namespace rtx {
// the GPU builder lives in csrc/hip/lbvh.hip: not part of a CPU-only program
int32_t build_bvh_gpu(const std::vector<double>&, int, std::vector<rt::FlatNode>*, std::vector<uint32_t>*, int32_t*, double*, std::string* err) {
  if (err) *err = "no GPU builder in this program";
  return -1;
}
}  // namespace rtx

// A grid of points inside the scene's room (both scenes fill 0 .. 555 on every axis), normals tilted off the axes and not of
// unit length: every form, estimator and output, split against whole.
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
  const int side = 5, n = side * side * side;
  std::vector<double> p(3 * n), nn(3 * n), tm(n);
  for (int r = 0; r < n; ++r) {
    const int i = r % side, j = (r / side) % side, k = r / (side * side);
    p[3 * r] = 60.0 + 108.0 * i; p[3 * r + 1] = 40.0 + 115.0 * j; p[3 * r + 2] = 70.0 + 100.0 * k;
    nn[3 * r] = 0.3 * (i - 2); nn[3 * r + 1] = 1.0 + 0.1 * j; nn[3 * r + 2] = -0.2 * (k - 2);
    tm[r] = 0.25 + 0.5 * r / n;
  }
  int bad = 0;
  // {surface form?, light sampling, sh_order}
  const int modes[][3] = {{1, 0, 0}, {1, 1, 0}, {0, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 1, 2}};
  for (const auto& m : modes) {
    const double* normals = m[0] ? nn.data() : nullptr;
    const int W = 3 * (m[2] ? sh_coeffs(m[2]) : 1);
    std::vector<double> s1((size_t)W * n), q1((size_t)W * n), s2((size_t)W * n), q2((size_t)W * n);
    if (gather_host_trace(&fs, n, p.data(), normals, tm.data(), 5, 0, 3, 6, 0, 9, wc.background, m[1], m[2], s1.data(), q1.data()) != 0) return 1;
    // the same batch cut in two by first_point and in two by first_sample
    const int cut = 50;
    for (int part = 0; part < 2; ++part) {
      const int lo = part ? cut : 0, hi = part ? n : cut;
      const double* nl = normals ? normals + 3 * lo : nullptr;
      if (gather_host_trace(&fs, hi - lo, p.data() + 3 * lo, nl, tm.data() + lo, 5 + (uint64_t)lo, 0, 1, 6, 0, 9, wc.background, m[1], m[2],
                            s2.data() + (size_t)W * lo, q2.data() + (size_t)W * lo) != 0 ||
          gather_host_trace(&fs, hi - lo, p.data() + 3 * lo, nl, tm.data() + lo, 5 + (uint64_t)lo, 1, 2, 6, 1, 9, wc.background, m[1], m[2],
                            s2.data() + (size_t)W * lo, q2.data() + (size_t)W * lo) != 0)
        return 1;
    }
    if (memcmp(s1.data(), s2.data(), s1.size() * sizeof(double)) != 0 || memcmp(q1.data(), q2.data(), q1.size() * sizeof(double)) != 0) {
      fprintf(stderr, "scene %d, surface %d, light sampling %d, sh_order %d: a split batch differs from the whole\n", sid, m[0], m[1], m[2]);
      ++bad;
    }
    double mean = 0.0;
    for (int r = 0; r < n; ++r) mean += s1[(size_t)W * r];
    printf("scene %3d, surface %d, light sampling %d, sh_order %d: %d points x 3 samples, mean first sum %.6f\n", sid, m[0], m[1], m[2], n,
           mean / (3.0 * n));
  }
  return bad;
}

int main() {
  int bad = 0;
  for (int32_t sid : {5, 6}) bad += check_scene(sid);  // Cornell smoke (a medium, a rectangle light); Book-2 final, reduced
  if (bad) { fprintf(stderr, "%d check(s) failed\n", bad); return 1; }
  printf("gather_host_check: sanitizer run clean\n");
  return 0;
}
#endif
