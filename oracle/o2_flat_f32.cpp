// ORACLE O2f -- TEST INFRASTRUCTURE, NOT A RENDER PATH OF THE PRODUCT.
//
// The float build of the flat oracle: the product's shared core (csrc/core/*.hpp) compiled for the host with the four
// defines csrc/hip/render_f32.hip compiles the device path with (RT_F32, RT_REAL float, namespaces rt32 / rtx32), driven
// by o2_flat.cpp's plain loop.  It is the CPU statement of exactly the operation the f32 kernels perform, so
//   * GPU f32 == O2f bit for bit wherever a sample reaches none of rt_math.hpp's five platform functions
//     (sinf cosf logf acosf atan2f: the only arithmetic that differs between glibc and the device), and
//   * GPU f32 ~ O2f up to a measured share of flipped pixels where it does (tests/test_gpu_f32_parity.py).
//
// What each step mirrors on the device path:
//   scene        the f64 FlatScene narrowed by the product's own converter (csrc/host/f32_layout.hpp: f32_images, run
//                by o2_flat.cpp's side of the seam below) and taken apart like csrc/hip/f32_entry.inc: take_blob --
//                the checker walks the bytes rtx_scene_upload_f32 uploads;
//   parameters   csrc/hip/render.hip: make_params -- the 24 camera doubles and the background cast to float;
//   one sample   rt::trace_sample (csrc/core/integrator.hpp), what k_trace_simple calls and every other kernel
//                restates: a float Color;
//   the sum      csrc/hip/pass_items.inc: store_sample widens the float Color to f64; csrc/hip/post_kernels.inc:
//                k_reduce_samples adds those doubles in ascending sample order starting from 0.0;
//   tone map     post_kernels.inc: k_tonemap -- the f64 sum cast to float, then rt::tone_map in float.
//
// This file is compiled twice into liboracle.so: as itself (oracle_o2f_*: glibc's float functions) and through
// o2_flat_f32_via_f64.cpp (oracle_o2g_*: the five functions computed in double and rounded -- a second faithful libm
// whose disagreement with the first is the reference-alone flip rate the GPU tests' caps are derived from).  The two
// builds live in different namespaces, so the linker cannot merge their inline functions.
//
// Only tests/ may call this.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <stdint.h>
#include <string>
#include <thread>
#include <vector>
#include "../ray-tracing-series-rust_amd/csrc/host/f32_blobs.hpp"
#include "oracle_abi.h"

#define RT_F32 1
#define RT_REAL float
#ifdef O2F_VIA_F64
#define RT_F32_MATH_VIA_F64 1
#define rt rt32d
#define rtx rtx32d
#define O2F(name) oracle_o2g_##name
#else
#define rt rt32
#define rtx rtx32
#define O2F(name) oracle_o2f_##name
#endif
#include "../ray-tracing-series-rust_amd/csrc/core/cull32.hpp"
#include "../ray-tracing-series-rust_amd/csrc/core/integrator.hpp"
#include "../ray-tracing-series-rust_amd/csrc/host/flat_scene.hpp"

// o2_flat.cpp (the f64 side of the seam): the f64 flat scene converted by the product's f32_images.  The images live in
// *keep (an opaque owner freed by oracle_f32_images_free); 0 on success.
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

bool narrow_scene(const void* flat, rtx::FlatScene* fs) {
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

rt::RenderParams make_params(const OracleCamera* cam, const OracleConfig* cfg) {  // csrc/hip/render.hip: make_params
  rt::RenderParams rp;
  static_assert(sizeof(OracleCamera) == 24 * sizeof(double) && sizeof(rt::FlatCamera) == 24 * sizeof(rt::real), "camera layout");
  for (int k = 0; k < 24; ++k) ((rt::real*)&rp.cam)[k] = (rt::real)((const double*)cam)[k];
  rp.background = rt::v3((rt::real)cfg->background[0], (rt::real)cfg->background[1], (rt::real)cfg->background[2]);
  rp.image_width = cfg->image_width;
  rp.image_height = cfg->image_height;
  rp.samples_per_pixel = cfg->samples_per_pixel;
  rp.max_depth = cfg->max_depth;
  rp.seed = cfg->seed;
  return rp;
}

}  // namespace

extern "C" {

// Samples first_sample .. first_sample + samples_per_pixel - 1 of every pixel of the shard.  first_sample = 0: a whole
// frame, the sums start at 0.0.  first_sample > 0: one more `add` of a progressive frame -- accum_rgb holds the sums of
// the samples before and each pixel's sum is continued in place, as the device continues its f64 sums; the tone map is
// that of first_sample + samples_per_pixel samples.
int O2F(render)(const void* flat, const OracleCamera* cam, const OracleConfig* cfg, int32_t shard_index, int32_t shard_count,
                int32_t block_rows, int32_t first_sample, double* accum_rgb, uint8_t* rgb8) {
  if (!flat || !cam || !cfg || shard_count <= 0 || block_rows <= 0 || first_sample < 0) return 1;
  rtx::FlatScene fs;
  if (!narrow_scene(flat, &fs)) return 2;
  const rt::SceneView sv = fs.view();
  const rt::RenderParams rp = make_params(cam, cfg);
  const int32_t w = rp.image_width, h = rp.image_height;
  std::vector<int32_t> rows;
  for (int32_t j = 0; j < h; ++j)
    if ((j / block_rows) % shard_count == shard_index) rows.push_back(j);
  const int threads = cfg->threads > 0 ? cfg->threads : 1;
  const size_t n_pix = rows.size() * (size_t)w, piece = 8;
  std::atomic<size_t> next{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t) {
    pool.emplace_back([&]() {
      rt::LocalStack<128> stack;
      stack.n = 0;
      for (;;) {
        const size_t p0 = next.fetch_add(piece);
        if (p0 >= n_pix) break;
        const size_t p1 = p0 + piece < n_pix ? p0 + piece : n_pix;
        for (size_t p = p0; p < p1; ++p) {
          const size_t lr = p / (size_t)w;
          const int32_t i = (int32_t)(p - lr * (size_t)w), j = rows[lr];
          const size_t o = 3 * p;
          double sum[3] = {0.0, 0.0, 0.0};  // k_reduce_samples: r = g = b = 0.0 on the first pass, else the sums so far
          if (first_sample > 0 && accum_rgb) { sum[0] = accum_rgb[o]; sum[1] = accum_rgb[o + 1]; sum[2] = accum_rgb[o + 2]; }
          for (int32_t s = 0; s < rp.samples_per_pixel; ++s) {
            const rt::Color c = rt::trace_sample<rt::F_ALL, false>(sv, rp, (uint32_t)i, (uint32_t)j, (uint32_t)(first_sample + s), stack, nullptr);
            sum[0] += (double)c.x; sum[1] += (double)c.y; sum[2] += (double)c.z;  // store_sample widens, k_reduce_samples adds
          }
          if (accum_rgb) { accum_rgb[o] = sum[0]; accum_rgb[o + 1] = sum[1]; accum_rgb[o + 2] = sum[2]; }
          if (rgb8) {
            int32_t c[3];
            rt::tone_map(rt::v3((rt::real)sum[0], (rt::real)sum[1], (rt::real)sum[2]), (uint32_t)(first_sample + rp.samples_per_pixel), c);  // k_tonemap
            rgb8[o] = (uint8_t)c[0]; rgb8[o + 1] = (uint8_t)c[1]; rgb8[o + 2] = (uint8_t)c[2];
          }
        }
      }
    });
  }
  for (std::thread& th : pool) th.join();
  return 0;
}

// One sample's radiance (the float Color widened): the aid for finding the first (pixel, sample) a kernel gets wrong.
int O2F(sample)(const void* flat, const OracleCamera* cam, const OracleConfig* cfg, int32_t i, int32_t j, int32_t sample,
                double rgb[3]) {
  if (!flat || !cam || !cfg) return 1;
  rtx::FlatScene fs;
  if (!narrow_scene(flat, &fs)) return 2;
  const rt::SceneView sv = fs.view();
  const rt::RenderParams rp = make_params(cam, cfg);
  rt::LocalStack<128> stack;
  stack.n = 0;
  const rt::Color c = rt::trace_sample<rt::F_ALL, false>(sv, rp, (uint32_t)i, (uint32_t)j, (uint32_t)sample, stack, nullptr);
  rgb[0] = c.x; rgb[1] = c.y; rgb[2] = c.z;
  return 0;
}

#ifndef O2F_VIA_F64
// world_hit over the narrowed scene with one float ray (o, d narrowed): out = {t, p.xyz, n.xyz, u, v, front_face}.
// t_min < 0 asks for the guard the integrator itself uses (ray_t_min).  -1: bad scene, 0: miss, 1: hit.
int oracle_core32_world_hit(const void* flat, const double o[3], const double d[3], double time, double t_min, double t_max,
                            uint64_t rng_seed, double out[10]) {
  if (!flat) return -1;
  rtx::FlatScene fs;
  if (!narrow_scene(flat, &fs)) return -1;
  const rt::SceneView sv = fs.view();
  rt::LocalStack<128> stack;
  stack.n = 0;
  rt::Rng rng = rt::rng_for_sample(rng_seed, 0, 0);
  rt::HitRecord rec;
  const rt::Ray r = rt::make_ray(rt::v3((float)o[0], (float)o[1], (float)o[2]), rt::v3((float)d[0], (float)d[1], (float)d[2]), (float)time);
  const rt::real tm = t_min < 0.0 ? rt::ray_t_min(r) : (rt::real)t_min;
  if (!rt::world_hit<rt::F_ALL, false>(sv, r, tm, (rt::real)t_max, &rec, rng, stack, nullptr)) return 0;
  out[0] = rec.t; out[1] = rec.p.x; out[2] = rec.p.y; out[3] = rec.p.z;
  out[4] = rec.normal.x; out[5] = rec.normal.y; out[6] = rec.normal.z;
  out[7] = rec.u; out[8] = rec.v; out[9] = rec.front_face ? 1.0 : 0.0;
  return 1;
}

// texture_value of one texture record of the narrowed scene at (u, v, p) narrowed: out = the float colour widened.
int oracle_core32_texture_value(const void* flat, int32_t texture_index, double u, double v, const double p[3], double out[3]) {
  if (!flat) return -1;
  rtx::FlatScene fs;
  if (!narrow_scene(flat, &fs)) return -1;
  if (texture_index < 0 || (size_t)texture_index >= fs.textures.size()) return -1;
  const rt::SceneView sv = fs.view();
  const rt::Color c = rt::texture_value<rt::F_ALL, false>(sv, texture_index, (float)u, (float)v, rt::v3((float)p[0], (float)p[1], (float)p[2]), nullptr);
  out[0] = c.x; out[1] = c.y; out[2] = c.z;
  return 1;
}

// material_scatter of one material record of the narrowed scene, ray and record narrowed: out = {direction xyz, attenuation
// xyz} widened, draws consumed (oracle_core_scatter's conventions).
int oracle_core32_scatter(const void* flat, int32_t material_index, const double o[3], const double d[3], double time,
                          const double p[3], const double normal[3], int32_t front_face, double u, double v, uint64_t rng_seed,
                          double out[7]) {
  if (!flat) return -1;
  rtx::FlatScene fs;
  if (!narrow_scene(flat, &fs)) return -1;
  if (material_index < 0 || (size_t)material_index >= fs.materials.size()) return -1;
  const rt::SceneView sv = fs.view();
  rt::HitRecord rec;
  memset(&rec, 0, sizeof(rec));
  rec.p = rt::v3((float)p[0], (float)p[1], (float)p[2]);
  rec.normal = rt::v3((float)normal[0], (float)normal[1], (float)normal[2]);
  rec.u = (float)u; rec.v = (float)v; rec.front_face = front_face != 0; rec.mat = material_index;
  rt::Rng rng = rt::rng_for_sample(rng_seed, 0, 0);
  rt::Rng walk = rng;
  rt::Ray scattered = rt::make_ray(rt::v3(0, 0, 0), rt::v3(0, 0, 0), 0.0f);
  rt::Color attenuation = rt::v3(0, 0, 0);
  const rt::Ray r_in = rt::make_ray(rt::v3((float)o[0], (float)o[1], (float)o[2]), rt::v3((float)d[0], (float)d[1], (float)d[2]), (float)time);
  const bool did = rt::material_scatter<rt::F_ALL, false>(sv, fs.materials[(size_t)material_index], r_in, rec, rng, &scattered, &attenuation, nullptr);
  out[0] = scattered.direction.x; out[1] = scattered.direction.y; out[2] = scattered.direction.z;
  out[3] = attenuation.x; out[4] = attenuation.y; out[5] = attenuation.z;
  int draws = 0;
  while ((walk.s0 != rng.s0 || walk.s1 != rng.s1) && draws < 4096) { rt::rng_next_u64(walk); ++draws; }
  out[6] = (walk.s0 == rng.s0 && walk.s1 == rng.s1) ? (double)draws : -1.0;
  return did ? 1 : 0;
}

// path_bounce_begin on a ray given as six doubles (narrowed) with `depth` bounces left: 1 when the path ends there.
int oracle_core32_path_ends(const double o[3], const double d[3], int32_t depth) {
  rt::PathState ps;
  ps.ray = rt::make_ray(rt::v3((float)o[0], (float)o[1], (float)o[2]), rt::v3((float)d[0], (float)d[1], (float)d[2]), 0.0f);
  ps.depth = depth;
  return rt::path_bounce_begin(&ps) ? 1 : 0;
}

// make_ray32 of a float ray, host branch: out = {ix, iy, iz, oix, oiy, oiz, err2, t_min}.
void oracle_core32_ray32(const double o[3], const double d[3], double out[8]) {
  const rt::Ray r = rt::make_ray(rt::v3((float)o[0], (float)o[1], (float)o[2]), rt::v3((float)d[0], (float)d[1], (float)d[2]), 0.0f);
  const rt::Ray32 q = rt::make_ray32(r, rt::ray_t_min(r));
  out[0] = q.ix; out[1] = q.iy; out[2] = q.iz; out[3] = q.oix; out[4] = q.oiy; out[5] = q.oiz; out[6] = q.err2; out[7] = q.t_min;
}

// The float building blocks as the host build evaluates them; fn and argument conventions are those of the float entries
// of rtx_device_math (csrc/hip/post_kernels.inc: k_device_math_f32).
void oracle_core32_math(int32_t fn, const double* x, const double* y, int64_t n, double* out) {
  for (int64_t k = 0; k < n; ++k) {
    const float a = (float)x[k], b = (float)y[k];
    const uint64_t raw = rt::f64_bits(x[k]), yb = rt::f64_bits(y[k]);
    rt::Rng g;
    g.s0 = raw; g.s1 = 0;
    union { uint32_t u; float f; } lo, hi;
    lo.u = (uint32_t)yb; hi.u = (uint32_t)(yb >> 32);
    float r;
    switch (fn) {
      case 32: r = rt::rt_sin(a); break;
      case 33: r = rt::rt_cos(a); break;
      case 34: r = rt::rt_log(a); break;
      case 35: r = rt::rt_acos(a); break;
      case 36: r = rt::rt_atan2(a, b); break;
      case 37: r = rt::rt_sqrt(a); break;
      case 38: r = a / b; break;
      case 39: r = (float)rt::rt_sin_sign(a); break;
      case 40: r = rt::rng_f64(g); break;
      case 41: r = rt::rng_range(g, lo.f, hi.f); break;
      case 43: r = rt::make_ray32(rt::make_ray(rt::v3(0, 0, 0), rt::v3(a, 1, 1), 0), rt::real(0.001)).ix; break;  // the slope cap, host branch
    default: r = rt::rng_range_pm1(g); break;
    }
    out[k] = (double)r;
  }
}
#endif

}  // extern "C"
