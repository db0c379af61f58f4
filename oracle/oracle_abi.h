/* ORACLE -- TEST INFRASTRUCTURE.  C entry points of liboracle.so (CPU checkers).
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library.
 * The product (ray-tracing-series-rust_amd/) never does. */
#ifndef ORACLE_ABI_H
#define ORACLE_ABI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct OracleCamera { /* same layout as RtxCamera (include/rtx_abi.h) */
  double origin[3], lower_left_corner[3], horizontal[3], vertical[3], u[3], v[3], w[3];
  double lens_radius, time1, time2;
} OracleCamera;

typedef struct OracleConfig {
  int32_t image_width, image_height;
  int32_t samples_per_pixel, max_depth;
  int32_t threads;          /* CPU threads (row bands, world.rs:1198-1227) */
  int32_t row_chunk_compat; /* 1: drop rows >= threads*floor(h/threads) like the reference */
  uint64_t seed;            /* render seed */
  uint64_t bvh_seed;        /* O1 only: stream for the reference BVH's random split axis */
  double background[3];
} OracleConfig;

typedef struct OracleCounters {
  uint64_t box_tests, sphere_tests, moving_sphere_tests, rect_tests, triangle_tests;
  uint64_t scatters, texels, perlin_calls, rays, samples;
} OracleCounters;

/* O1: literal object-graph restatement (oracle/o1_literal.cpp).  graph = rtx_builder_graph(). */
int oracle_o1_render(const void* graph, int32_t world_handle, const OracleCamera* cam,
                     const OracleConfig* cfg, double* accum_rgb, uint8_t* rgb8);
int oracle_o1_render_window(const void* graph, int32_t world_handle, const OracleCamera* cam, const OracleConfig* cfg,
                            int32_t j0, int32_t j1, int32_t i0, int32_t i1, double* accum_rgb);
/* O2: CPU loop over the product's FLATTENED arrays through the product's shared core headers
 * (oracle/o2_flat.cpp).  flat = rtx_flat_arrays().  Renders the shard
 * { j : (j / block_rows) % shard_count == shard_index } compacted, like rtx_render_device.
 * counters may be NULL. */
int oracle_o2_render(const void* flat, const OracleCamera* cam, const OracleConfig* cfg,
                     int32_t shard_index, int32_t shard_count, int32_t block_rows,
                     double* accum_rgb, uint8_t* rgb8, OracleCounters* counters);
/* One sample's radiance through O2 (debugging aid for parity failures). */
int oracle_o2_sample(const void* flat, const OracleCamera* cam, const OracleConfig* cfg, int32_t i,
                     int32_t j, int32_t sample, double rgb[3]);

/* O2f: O2 with real = float (oracle/o2_flat_f32.cpp) -- the CPU statement of what the f32 fast mode computes.  Takes the
 * f64 flat scene and narrows it with the product's converter.  Renders samples first_sample .. first_sample + spp - 1 of
 * the shard's pixels; accum_rgb is the ordered f64 sum of the widened float samples.  oracle_o2g_*: the same with the five
 * platform functions computed in double and rounded to float (o2_flat_f32_via_f64.cpp). */
int oracle_o2f_render(const void* flat, const OracleCamera* cam, const OracleConfig* cfg, int32_t shard_index,
                      int32_t shard_count, int32_t block_rows, int32_t first_sample, double* accum_rgb, uint8_t* rgb8);
int oracle_o2f_sample(const void* flat, const OracleCamera* cam, const OracleConfig* cfg, int32_t i, int32_t j,
                      int32_t sample, double rgb[3]);
int oracle_o2g_render(const void* flat, const OracleCamera* cam, const OracleConfig* cfg, int32_t shard_index,
                      int32_t shard_count, int32_t block_rows, int32_t first_sample, double* accum_rgb, uint8_t* rgb8);
int oracle_o2g_sample(const void* flat, const OracleCamera* cam, const OracleConfig* cfg, int32_t i, int32_t j,
                      int32_t sample, double rgb[3]);
/* Probes into the float build of the core: one ray through world_hit (t_min < 0: the integrator's own guard), the
 * non-finite-ray rule of path_bounce_begin, make_ray32's host branch, and the float building blocks under the function
 * codes of rtx_device_math's float entries. */
int oracle_core32_world_hit(const void* flat, const double o[3], const double d[3], double time, double t_min,
                            double t_max, uint64_t rng_seed, double out[10]);
int oracle_core32_path_ends(const double o[3], const double d[3], int32_t depth);
void oracle_core32_ray32(const double o[3], const double d[3], double out[8]);
void oracle_core32_math(int32_t fn, const double* x, const double* y, int64_t n, double* out);
int oracle_core32_texture_value(const void* flat, int32_t texture_index, double u, double v, const double p[3], double out[3]);
/* The product's f64 -> f32 scene converter (csrc/host/f32_layout.hpp) and what it is fed. */
int64_t oracle_f32_convert(const char* desc, const void* in, int64_t n, int64_t elem64, void* out);
const char* oracle_f32_desc(int32_t k, const char** name);
const void* oracle_flat_array(const void* flat, const char* name, int64_t* n, int64_t* elem_bytes);
uint32_t oracle_flat_features(const void* flat);

/* Known-answer probes into O1's restated functions. */
void oracle_o1_vec3_ops(const double a[3], const double b[3], double t, double out[24]);
void oracle_o1_tone_map(const double sum[3], uint32_t spp, int32_t out[3]);
void oracle_o1_sphere_uv(const double p[3], double uv[2]);
double oracle_o1_reflectance(double cosine, double ref_idx);
void oracle_o1_refract(const double uv[3], const double n[3], double ratio, double out[3]);
void oracle_o1_reflect(const double v[3], const double n[3], double out[3]);
int oracle_o1_aabb_hit(const double mn[3], const double mx[3], const double o[3], const double d[3],
                       double t_min, double t_max);
int oracle_o1_hit(const void* graph, int32_t handle, const double o[3], const double d[3], double time,
                  double t_min, double t_max, uint64_t rng_seed, double out[10]);
/* Texture::value of one texture: the graph's (recursing to any depth), and texture_value over the flat record of the same
 * index (a graph texture handle IS its flat index) in the f64 core; oracle_core32_texture_value is the float build's. */
int oracle_o1_texture_value(const void* graph, int32_t texture_handle, double u, double v, const double p[3], double out[3]);
int oracle_core_texture_value(const void* flat, int32_t texture_index, double u, double v, const double p[3], double out[3]);
/* Material::scatter of one material on a given ray and hit record, on the stream of rng_seed: the graph's, material_scatter over
 * the flat record of the same index in the f64 core, and the float build's.  out = {direction xyz, attenuation xyz, draws
 * consumed}; 1 scattered, 0 not (the attenuation is then unspecified), -1 no such material. */
int oracle_o1_scatter(const void* graph, int32_t material_handle, const double o[3], const double d[3], double time,
                      const double p[3], const double normal[3], int32_t front_face, double u, double v, uint64_t rng_seed,
                      double out[7]);
int oracle_core_scatter(const void* flat, int32_t material_index, const double o[3], const double d[3], double time,
                        const double p[3], const double normal[3], int32_t front_face, double u, double v, uint64_t rng_seed,
                        double out[7]);
int oracle_core32_scatter(const void* flat, int32_t material_index, const double o[3], const double d[3], double time,
                          const double p[3], const double normal[3], int32_t front_face, double u, double v, uint64_t rng_seed,
                          double out[7]);

/* The same probes into the product's shared core (ray-tracing-series-rust_amd/csrc/core). */
void oracle_core_vec3_ops(const double a[3], const double b[3], double t, double out[24]);
void oracle_core_tone_map(const double sum[3], uint32_t spp, int32_t out[3]);
void oracle_core_sphere_uv(const double p[3], double uv[2]);
double oracle_core_reflectance(double cosine, double ref_idx);
void oracle_core_refract(const double uv[3], const double n[3], double ratio, double out[3]);
void oracle_core_reflect(const double v[3], const double n[3], double out[3]);
int oracle_core_aabb_hit(const double mn[3], const double mx[3], const double o[3], const double d[3],
                         double t_min, double t_max);
int oracle_core_world_hit(const void* flat, const double o[3], const double d[3], double time, double t_min,
                          double t_max, uint64_t rng_seed, double out[10]);
int oracle_core_world_hit_mat(const void* flat, const double o[3], const double d[3], double time, double t_min,
                              double t_max, uint64_t rng_seed, double out[10], int32_t* mat);
int oracle_audit_flat(const void* flat, int32_t* max_depth_out);
/* The exact audit (o2_flat.cpp): nodes == NULL audits the scene's own node array; cluster > 0 asks for full leaves. */
#define ORACLE_AUDIT_LEAF_ORDER 1 /* leaves ascend contiguously in a depth-first walk (GPU-built trees) */
#define ORACLE_AUDIT_ASK_FIRST 2  /* split "axis" 3 is legal on a node whose child 0 is a one-primitive leaf (host SAH trees) */
int oracle_audit_flat_exact(const void* flat, const void* nodes, int64_t n_nodes, int32_t flags, int32_t cluster,
                            int32_t* max_depth_out);
int oracle_audit_motion(const void* flat, int32_t n_times, int64_t* checked);
double oracle_motion_leaf_area_ratio(const void* flat);
int oracle_lds_walk_render(const void* flat, const OracleCamera* cam, const OracleConfig* cfg, int32_t use_motion,
                           int32_t row_stride, double* accum_rgb, uint64_t counts[3]);

/* Shared-core probes (product headers compiled for the host): RNG and rt_math. */
void oracle_philox4x32_10(uint32_t ctr[4], uint32_t k0, uint32_t k1);
uint64_t oracle_splitmix64_next(uint64_t* state);
void oracle_sample_stream(uint64_t seed, uint64_t pixel, uint32_t sample, int32_t n, double* out);
void oracle_rt_math(int32_t fn, const double* x, const double* y, int64_t n, double* out);

#ifdef __cplusplus
}
#endif
#endif
