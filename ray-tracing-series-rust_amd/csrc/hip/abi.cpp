// Host-only entry points of include/rtx_abi.h: builder (one call per reference constructor),
// camera/config, scene catalogue, flatten, PPM output.  Device entry points: render.hip.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>
#include "../host/scenes.hpp"
#include "../host/light_table.hpp"
#include "../host/set_transforms.hpp"
#include "../host/set_triangles.hpp"
#include "../host/rebuild_instances.hpp"
#include "../host/set_shading.hpp"
#include "abi_internal.hpp"

static_assert(RTX_MAT_LAMBERTIAN == rt::MAT_LAMBERTIAN && RTX_MAT_METAL == rt::MAT_METAL && RTX_MAT_DIELECTRIC == rt::MAT_DIELECTRIC &&
              RTX_MAT_DIFFUSE_LIGHT == rt::MAT_DIFFUSE_LIGHT && RTX_MAT_ISOTROPIC == rt::MAT_ISOTROPIC, "RTX_MAT_* are rt::MAT_*");
static_assert(RTX_TEX_SOLID == rt::TEX_SOLID && RTX_TEX_CHECKER == rt::TEX_CHECKER && RTX_TEX_NOISE == rt::TEX_NOISE &&
              RTX_TEX_IMAGE == rt::TEX_IMAGE, "RTX_TEX_* are rt::TEX_*");
static_assert(sizeof(RtxShadingEdit) == 40 && sizeof(rt::ShadingWrite) == 40, "RtxShadingEdit layout");
static_assert(sizeof(RtxMaterialInfo) == 40 && sizeof(RtxTextureInfo) == 48 && sizeof(RtxMediumInfo) == 16, "shading inspectors' layout");

namespace rtx {
static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

// RTX_OK, or RTX_EINVAL with the message "<who>: <bad>".
static rtx_status refuse(const char* who, const char* bad) {
  if (bad) set_error(std::string(who) + ": " + bad);
  return bad ? RTX_EINVAL : RTX_OK;
}
// The rungs every ray query's check opens with (Rays: RtxRayBatch or RtxRadianceRays); NULL when they all pass.
template <class Rays>
static const char* bad_ray_columns(const rtx_scene* s, const Rays* rays, const void* out, const char* out_is_null) {
  if (!s) return "scene is NULL";
  if (!rays) return "rays is NULL";
  if (!out) return out_is_null;
  if (rays->n < 0) return "rays->n < 0";
  if (rays->n > 0 && !rays->origin) return "rays->origin is NULL";
  if (rays->n > 0 && !rays->direction) return "rays->direction is NULL";
  return nullptr;
}
rtx_status check_ray_batch(const char* who, const rtx_scene* s, const RtxRayBatch* rays, const void* out, const char* out_name) {
  const std::string out_is_null = std::string(out_name) + " is NULL";
  const char* bad = bad_ray_columns(s, rays, out, out_is_null.c_str());
  if (!bad && rays->t_min != rays->t_min) bad = "rays->t_min is NaN";
  else if (!bad && rays->t_max_all != rays->t_max_all) bad = "rays->t_max_all is NaN";
  return refuse(who, bad);
}
rtx_status check_trace_rays(const char* who, const rtx_scene* s, const RtxRadianceRays* rays, const double* sum_rgb) {
  const char* bad = bad_ray_columns(s, rays, sum_rgb, "sum_rgb is NULL");
  if (bad) {}  // (a common rung)
  else if (rays->samples < 1) bad = "rays->samples < 1";
  else if (rays->max_depth < 1) bad = "rays->max_depth < 1 (Config::new asserts max_depth > 0, world.rs:36-40)";
  else if (rays->reserved != 0) bad = "rays->reserved is not 0";
  else if (rays->light_sampling != 0 && rays->light_sampling != 1) bad = "rays->light_sampling is neither 0 nor 1";
  else if (rays->accumulate != 0 && rays->accumulate != 1) bad = "rays->accumulate is neither 0 nor 1";
  else if (rays->background[0] != rays->background[0] || rays->background[1] != rays->background[1] ||
           rays->background[2] != rays->background[2]) bad = "rays->background is NaN";
  else if ((uint64_t)rays->first_sample + (uint64_t)rays->samples > (1ull << 32)) bad = "rays->first_sample + rays->samples is past 2^32";
  return refuse(who, bad);
}
rtx_status check_gather(const char* who, const rtx_scene* s, const RtxGatherPoints* g, const double* sum) {
  const char* bad = nullptr;
  if (!s) bad = "scene is NULL";
  else if (!g) bad = "points is NULL";
  else if (!sum) bad = "sum is NULL";
  else if (g->n < 0) bad = "points->n < 0";
  else if (g->n > 0 && !g->position) bad = "points->position is NULL";
  else if (g->samples < 1) bad = "points->samples < 1";
  else if (g->max_depth < 1) bad = "points->max_depth < 1 (Config::new asserts max_depth > 0, world.rs:36-40)";
  else if (g->reserved[0] != 0 || g->reserved[1] != 0) bad = "points->reserved is not 0";
  else if (g->light_sampling != 0 && g->light_sampling != 1) bad = "points->light_sampling is neither 0 nor 1";
  else if (g->accumulate != 0 && g->accumulate != 1) bad = "points->accumulate is neither 0 nor 1";
  else if (g->sh_order < 0 || g->sh_order > 2) bad = "points->sh_order is not 0, 1 or 2";
  else if (g->sh_order > 0 && g->normal) bad = "points->sh_order > 0 with points->normal: spherical harmonics are for the probe form";
  else if (g->background[0] != g->background[0] || g->background[1] != g->background[1] ||
           g->background[2] != g->background[2]) bad = "points->background is NaN";
  else if ((uint64_t)g->first_sample + (uint64_t)g->samples > (1ull << 32)) bad = "points->first_sample + points->samples is past 2^32";
  return refuse(who, bad);
}
rtx_status check_point_batch(const char* who, const rtx_scene* s, const RtxPointBatch* b, const RtxNearest* out) {
  const char* bad = nullptr;
  if (!s) bad = "scene is NULL";
  else if (!b) bad = "points is NULL";
  else if (!out) bad = "out is NULL";
  else if (b->n < 0) bad = "points->n < 0";
  else if (b->n > 0 && !b->points) bad = "points->points is NULL";
  else if (b->r_max_all != b->r_max_all) bad = "points->r_max_all is NaN";
  else if (b->r_max_all < 0.0) bad = "points->r_max_all < 0";
  else if (b->media != 0 && b->media != 1) bad = "points->media is neither 0 nor 1";
  else if (b->reserved != 0) bad = "points->reserved is not 0";
  return refuse(who, bad);
}
rtx_status check_set_transforms(const char* who, const rtx_scene* s, const RtxSlotOps* updates, int64_t n, std::vector<RtxSlotOps>* resolved) {
  std::string err;
  if (!check_slot_ops_shape(who, s, updates, n, &err)) { set_error(err); return RTX_EINVAL; }
  *resolved = resolve_slot_ops(updates, n);
  return RTX_OK;
}
// The size check of the test hook rtx_flat_array.
static rtx_status check_array_bytes(const char* who, size_t have, const void* out, size_t bytes) {
  if (bytes != have) { set_error(std::string(who) + ": the array holds " + std::to_string(have) + " bytes, not " + std::to_string(bytes)); return RTX_EINVAL; }
  if (have && !out) { set_error(std::string(who) + ": out is NULL"); return RTX_EINVAL; }
  return RTX_OK;
}
}  // namespace rtx

using namespace rtx;

namespace {
inline rtx_handle checked(rtx_builder* b, int32_t h) {
  if (h < 0) set_error(b->graph.error.empty() ? "invalid argument" : b->graph.error);
  return h;
}
#define NEED_BUILDER(b)                                  \
  if (!(b)) { set_error("NULL builder"); return -1; }
}  // namespace

extern "C" {

int32_t rtx_abi_version(void) { return RTX_ABI_VERSION; }
const char* rtx_last_error(void) { return g_last_error.c_str(); }
const char* rtx_trace_kernel_name(int32_t kernel) {
  switch (kernel) {
    case RTX_KERNEL_SIMPLE: return "k_trace_simple";
    case RTX_KERNEL_PERSISTENT: return "k_trace_persistent";
    case RTX_KERNEL_STREAM: return "k_trace_stream";
    case RTX_KERNEL_VOTE: return "k_trace_vote";
    case RTX_KERNEL_LDS: return "k_trace_lds";
    case RTX_KERNEL_WQ: return "k_trace_wq";
    case RTX_KERNEL_WORLD: return "k_trace_world";
    case RTX_KERNEL_WAVEFRONT: return "k_wf_trace";
    case RTX_KERNEL_NEE: return "k_trace_nee";
    case RTX_KERNEL_RAYS: return "k_trace_rays";
    default: return "?";
  }
}

rtx_status rtx_builder_create(uint64_t scene_seed, rtx_builder** out) {
  if (!out) { set_error("rtx_builder_create: NULL out"); return RTX_EINVAL; }
  *out = new (std::nothrow) rtx_builder(scene_seed);
  if (!*out) { set_error("out of memory"); return RTX_ENOMEM; }
  return RTX_OK;
}
void rtx_builder_destroy(rtx_builder* b) { delete b; }
double rtx_builder_random(rtx_builder* b) { return b ? rt::host_rng_f64(b->graph.rng) : 0.0; }

rtx_handle rtx_solid_color(rtx_builder* b, const double rgb[3]) { NEED_BUILDER(b); if (!rgb) { set_error("NULL rgb"); return -1; } return checked(b, b->graph.solid_color(rgb)); }
rtx_handle rtx_checker(rtx_builder* b, rtx_handle even, rtx_handle odd) { NEED_BUILDER(b); return checked(b, b->graph.checker(even, odd)); }
rtx_handle rtx_noise(rtx_builder* b, double scale) { NEED_BUILDER(b); return checked(b, b->graph.noise(scale)); }
rtx_handle rtx_image_from_ppm(rtx_builder* b, const char* path) { NEED_BUILDER(b); if (!path) { set_error("NULL path"); return -1; } return checked(b, b->graph.image_from_ppm(path)); }
rtx_handle rtx_image_from_texels(rtx_builder* b, int32_t w, int32_t h, const double* t) { NEED_BUILDER(b); return checked(b, b->graph.image_from_texels(w, h, t)); }

rtx_handle rtx_lambertian(rtx_builder* b, rtx_handle tex) { NEED_BUILDER(b); return checked(b, b->graph.lambertian(tex)); }
rtx_handle rtx_metal(rtx_builder* b, const double albedo[3], double fuzz) { NEED_BUILDER(b); if (!albedo) { set_error("NULL albedo"); return -1; } return checked(b, b->graph.metal(albedo, fuzz)); }
rtx_handle rtx_dielectric(rtx_builder* b, double ir) { NEED_BUILDER(b); return checked(b, b->graph.dielectric(ir)); }
rtx_handle rtx_diffuse_light(rtx_builder* b, rtx_handle tex) { NEED_BUILDER(b); return checked(b, b->graph.diffuse_light(tex)); }
rtx_handle rtx_isotropic(rtx_builder* b, rtx_handle tex) { NEED_BUILDER(b); return checked(b, b->graph.isotropic(tex)); }

rtx_handle rtx_sphere(rtx_builder* b, const double c[3], double r, rtx_handle mat) { NEED_BUILDER(b); if (!c) { set_error("NULL center"); return -1; } return checked(b, b->graph.sphere(c, r, mat)); }
rtx_handle rtx_gravity_sphere(rtx_builder* b, const double start[3], double time0, double radius, rtx_handle mat) {
  if (!b || !start) { set_error("rtx_gravity_sphere: NULL argument"); return -1; }
  return checked(b, b->graph.gravity_sphere(start, time0, radius, mat));
}
rtx_handle rtx_moving_sphere(rtx_builder* b, const double c0[3], const double c1[3], double t0, double t1, double r, rtx_handle mat) {
  NEED_BUILDER(b);
  if (!c0 || !c1) { set_error("NULL center"); return -1; }
  return checked(b, b->graph.moving_sphere(c0, c1, t0, t1, r, mat));
}
rtx_handle rtx_triangle(rtx_builder* b, const double v0[3], const double v1[3], const double v2[3], rtx_handle mat) {
  NEED_BUILDER(b);
  if (!v0 || !v1 || !v2) { set_error("NULL vertex"); return -1; }
  return checked(b, b->graph.triangle(v0, v1, v2, mat));
}
rtx_handle rtx_xy_rect(rtx_builder* b, double x0, double x1, double y0, double y1, double k, rtx_handle mat) { NEED_BUILDER(b); return checked(b, b->graph.rect(H_XY_RECT, x0, x1, y0, y1, k, mat)); }
rtx_handle rtx_xz_rect(rtx_builder* b, double x0, double x1, double y0, double y1, double k, rtx_handle mat) { NEED_BUILDER(b); return checked(b, b->graph.rect(H_XZ_RECT, x0, x1, y0, y1, k, mat)); }
rtx_handle rtx_yz_rect(rtx_builder* b, double x0, double x1, double y0, double y1, double k, rtx_handle mat) { NEED_BUILDER(b); return checked(b, b->graph.rect(H_YZ_RECT, x0, x1, y0, y1, k, mat)); }
rtx_handle rtx_rect_prism(rtx_builder* b, const double p0[3], const double p1[3], rtx_handle mat) {
  NEED_BUILDER(b);
  if (!p0 || !p1) { set_error("NULL corner"); return -1; }
  return checked(b, b->graph.rect_prism(p0, p1, mat));
}
rtx_handle rtx_hittable_list_new(rtx_builder* b) { NEED_BUILDER(b); return b->graph.list_new(); }
rtx_status rtx_hittable_list_add(rtx_builder* b, rtx_handle list, rtx_handle object) {
  if (!b) { set_error("NULL builder"); return RTX_EINVAL; }
  if (!b->graph.list_add(list, object)) { set_error(b->graph.error); return RTX_EINVAL; }
  return RTX_OK;
}
rtx_handle rtx_bvh_from_list(rtx_builder* b, rtx_handle list, double t0, double t1) { NEED_BUILDER(b); return checked(b, b->graph.bvh_from_list(list, t0, t1)); }
rtx_handle rtx_instance_bvh_from_list(rtx_builder* b, rtx_handle list) { NEED_BUILDER(b); return checked(b, b->graph.instance_bvh_from_list(list)); }
rtx_handle rtx_translate(rtx_builder* b, const double offset[3], rtx_handle obj) { NEED_BUILDER(b); if (!offset) { set_error("NULL offset"); return -1; } return checked(b, b->graph.translate(offset, obj)); }
rtx_handle rtx_rotate_y(rtx_builder* b, double angle, rtx_handle obj) { NEED_BUILDER(b); return checked(b, b->graph.rotate_y(angle, obj)); }
rtx_handle rtx_constant_medium(rtx_builder* b, const double rgb[3], double density, rtx_handle boundary) {
  NEED_BUILDER(b);
  if (!rgb) { set_error("NULL rgb"); return -1; }
  return checked(b, b->graph.constant_medium(rgb, density, boundary));
}
rtx_handle rtx_triangle_model(rtx_builder* b, const char* path, double scale) { NEED_BUILDER(b); if (!path) { set_error("NULL path"); return -1; } return checked(b, b->graph.triangle_model(path, scale)); }
rtx_handle rtx_triangle_mesh(rtx_builder* b, const double* vertices, int64_t n_vertices, const int64_t* faces, int64_t n_faces, rtx_handle mat) {
  NEED_BUILDER(b);
  if (!vertices || !faces || n_vertices < 0 || n_faces < 0) { set_error("triangle_mesh: NULL or negative"); return -1; }
  return checked(b, b->graph.triangle_mesh(vertices, n_vertices, faces, n_faces, mat));
}

rtx_status rtx_camera_new(const double lookfrom[3], const double lookat[3], const double vup[3],
                          double vfov, double aspect_ratio, double aperture, double focus_dist,
                          double time1, double time2, RtxCamera* out) {
  if (!lookfrom || !lookat || !vup || !out) { set_error("rtx_camera_new: NULL argument"); return RTX_EINVAL; }
  if (!(time1 < time2)) { set_error("rtx_camera_new: time1 >= time2 (gen_range(time1..time2) panics, camera.rs:69)"); return RTX_EINVAL; }
  rt::FlatCamera c = camera_new(lookfrom, lookat, vup, vfov, aspect_ratio, aperture, focus_dist, time1, time2);
  static_assert(sizeof(RtxCamera) == sizeof(rt::FlatCamera), "camera layout");
  memcpy(out, &c, sizeof(c));
  return RTX_OK;
}

rtx_status rtx_config_new(double aspect_ratio, int32_t image_width, int32_t samples_per_pixel,
                          int32_t max_depth, int32_t threads, RtxConfig* out) {
  if (!out) { set_error("rtx_config_new: NULL out"); return RTX_EINVAL; }
  // world.rs:36-40
  if (threads <= 0) { set_error("Config::new: assert!(threads > 0)"); return RTX_EINVAL; }
  if (image_width <= 0) { set_error("Config::new: assert!(image_width > 0)"); return RTX_EINVAL; }
  if (samples_per_pixel <= 0) { set_error("Config::new: assert!(samples_per_pixel > 0)"); return RTX_EINVAL; }
  if (max_depth <= 0) { set_error("Config::new: assert!(max_depth > 0)"); return RTX_EINVAL; }
  memset(out, 0, sizeof(*out));
  out->aspect_ratio = aspect_ratio;
  out->image_width = image_width;
  out->samples_per_pixel = samples_per_pixel;
  out->max_depth = max_depth;
  out->threads = threads;
  out->seed = 1;
  out->background[0] = 0.7; out->background[1] = 0.8; out->background[2] = 1.0;
  return RTX_OK;
}

int32_t rtx_image_height(const RtxConfig* cfg) {
  if (!cfg) return 0;
  return rt::rt_f64_as_i32((double)cfg->image_width / cfg->aspect_ratio);  // world.rs:1192
}

int32_t rtx_shard_rows(const RtxConfig* cfg, const RtxShard* shard) {
  if (!cfg) return 0;
  int32_t h = rtx_image_height(cfg);
  RtxShard sh = {0, 1, 1, 0};
  if (shard) sh = *shard;
  if (sh.shard_count <= 0 || sh.block_rows <= 0) return 0;
  int n = 0;
  for (int32_t j = 0; j < h; ++j)
    if ((j / sh.block_rows) % sh.shard_count == sh.shard_index) ++n;
  return n;
}

rtx_status rtx_get_world_cam(rtx_builder* b, int32_t scene_id, const RtxSceneOptions* options,
                             rtx_handle* world_out, RtxCamera* cam_out, double background_out[3]) {
  if (!b || !world_out || !cam_out || !background_out) { set_error("rtx_get_world_cam: NULL argument"); return RTX_EINVAL; }
  SceneOptions opt;
  if (options) {
    opt.camera_aspect = options->camera_aspect;
    opt.earth_ppm = options->earth_ppm;
    opt.dragon_ply = options->dragon_ply;
    if (options->mesh_triangles > 0) opt.mesh_triangles = options->mesh_triangles;
    if (options->book2_boxes_per_side > 0) opt.book2_boxes_per_side = options->book2_boxes_per_side;
    if (options->book2_spheres > 0) opt.book2_spheres = options->book2_spheres;
  }
  WorldCam wc;
  std::string err;
  if (!get_world_cam(b->graph, scene_id, opt, &wc, &err)) {
    set_error(err);
    return scene_id == RTX_SCENE_RANDOM_MOVING ? RTX_EUNSUPPORTED : RTX_EINVAL;
  }
  *world_out = wc.world;
  memcpy(cam_out, &wc.cam, sizeof(wc.cam));
  background_out[0] = wc.background[0]; background_out[1] = wc.background[1]; background_out[2] = wc.background[2];
  return RTX_OK;
}

rtx_status rtx_flatten(const rtx_builder* b, rtx_handle world, const RtxBuildOptions* options, rtx_flat** out) {
  if (!b || !out) { set_error("rtx_flatten: NULL argument"); return RTX_EINVAL; }
  *out = nullptr;
  BuildOptions opt;
  if (options) {
    if (options->max_leaf > 0) opt.max_leaf = options->max_leaf;
    if (options->sah_bins > 0) opt.sah_bins = options->sah_bins;
    opt.reference_bvh = options->reference_bvh ? 1 : 0;
    opt.gpu_builder = options->gpu_builder ? 1 : 0;
    if (options->bvh_seed) opt.bvh_seed = options->bvh_seed;
  }
  if (const char* e = getenv("RTX_LEAF_FIRST")) opt.leaf_first = atoi(e) != 0 ? 1 : 0;  // A/B switches, never change a result
  if (const char* e = getenv("RTX_MOTION_TOPOLOGY")) opt.motion_topology = atoi(e) != 0 ? 1 : 0;
  rtx_flat* f = new (std::nothrow) rtx_flat();
  if (!f) { set_error("out of memory"); return RTX_ENOMEM; }
  std::string err;
  if (!b->graph.valid_hittable(world)) { delete f; set_error("rtx_flatten: bad world handle"); return RTX_EINVAL; }
  if (!flatten_scene(b->graph, world, opt, &f->scene, &err)) {
    delete f;
    set_error(err);
    return RTX_EUNSUPPORTED;
  }
  f->options = opt;
  *out = f;
  return RTX_OK;
}
void rtx_flat_destroy(rtx_flat* f) { delete f; }

rtx_status rtx_flat_info(const rtx_flat* f, RtxFlatInfo* o) {
  if (!f || !o) { set_error("rtx_flat_info: NULL argument"); return RTX_EINVAL; }
  const FlatScene& s = f->scene;
  o->n_spheres = (int64_t)s.spheres.size(); o->n_moving_spheres = (int64_t)s.moving_spheres.size();
  o->n_rects = (int64_t)s.rects.size(); o->n_triangles = (int64_t)s.triangles.size();
  o->n_nodes = (int64_t)s.nodes.size(); o->n_refs = (int64_t)s.refs.size();
  o->n_entries = (int64_t)s.entries.size(); o->n_top_level = (int64_t)s.top_level.size();
  o->n_materials = (int64_t)s.materials.size(); o->n_textures = (int64_t)s.textures.size();
  o->n_perlins = (int64_t)s.perlins.size(); o->n_images = (int64_t)s.images.size();
  o->n_texels = (int64_t)(s.texels.size() / 3);
  o->total_bytes = (int64_t)s.total_bytes();
  o->max_stack = s.max_stack; o->n_bvh = s.n_bvh; o->sah_cost = s.sah_cost;
  o->bvh_build_ms = s.bvh_build_ms; o->bvh_device_ms = s.bvh_device_ms;
  o->n_gravity_spheres = (int64_t)s.gravity_spheres.size();
  return RTX_OK;
}

rtx_status rtx_flat_lights(const rtx_flat* f, RtxLightInfo* o) {
  if (!f || !o) { set_error("rtx_flat_lights: NULL argument"); return RTX_EINVAL; }
  const LightTable t = build_light_table(f->scene);
  o->n_lights = (int32_t)t.lights.size();
  o->n_rect_lights = t.n_rect;
  o->n_sphere_lights = t.n_sphere;
  o->n_unsampled_emitters = t.n_unsampled;
  o->total_area = t.total_area;
  return RTX_OK;
}

rtx_status rtx_flat_instances(const rtx_flat* f, RtxInstanceInfo* o) {
  if (!f || !o) { set_error("rtx_flat_instances: NULL argument"); return RTX_EINVAL; }
  const FlatScene& s = f->scene;
  o->n_trees = s.n_instance_trees; o->n_members = s.n_instance_members;
  o->n_nodes = s.n_instance_nodes; o->max_depth = s.instance_depth;
  return RTX_OK;
}

int32_t rtx_flat_slot_chain(const rtx_flat* f, int32_t slot, int32_t kinds[4]) {
  if (!f || !kinds || slot < 0 || (size_t)slot >= f->scene.top_level.size()) return -1;
  const FlatScene& s = f->scene;
  const rt::FlatEntry* E = &s.entries[(size_t)s.top_level[(size_t)slot]];
  if (E->kind == rt::ENTRY_MEDIUM) E = &s.entries[(size_t)E->a];
  if (E->kind != rt::ENTRY_XFORM) return 0;
  for (int k = 0; k < E->b; ++k) kinds[k] = E->ops[k].op;
  return E->b;
}

rtx_status rtx_flat_instance_tree(const rtx_flat* f, int32_t k, RtxInstanceTree* o) {
  if (!f || !o) { set_error("rtx_flat_instance_tree: NULL argument"); return RTX_EINVAL; }
  const FlatScene& s = f->scene;
  int32_t seen = 0;
  for (const rt::FlatEntry& e : s.entries) {
    if (e.kind != rt::ENTRY_INSTANCE || e.a < 0 || seen++ != k) continue;
    o->first_slot = e.b; o->n_slots = e.c; o->n_nodes = e.c - 1;
    // the height in nodes, as the builder counts it: the stack entries a walk of the tree can hold
    int32_t depth = 0;
    std::vector<std::pair<int32_t, int32_t>> todo{{e.a, 1}};
    while (!todo.empty()) {
      const std::pair<int32_t, int32_t> n = todo.back();
      todo.pop_back();
      depth = std::max(depth, n.second);
      for (int c = 0; c < 2; ++c)
        if (!rt::node_child_is_leaf(s.nodes[(size_t)n.first].child[c])) todo.push_back({s.nodes[(size_t)n.first].child[c], n.second + 1});
    }
    o->depth = depth;
    return RTX_OK;
  }
  set_error("rtx_flat_instance_tree: k is out of range (the scene has " + std::to_string(s.n_instance_trees) + " instance trees)");
  return RTX_EINVAL;
}

rtx_status rtx_flat_set_transforms(rtx_flat* f, const RtxSlotOps* updates, int64_t n) {
  std::string err;
  if (!flat_set_transforms("rtx_flat_set_transforms", f ? &f->scene : nullptr, updates, n, &err)) { set_error(err); return RTX_EINVAL; }
  return RTX_OK;
}

rtx_status rtx_flat_rebuild_instance_trees(rtx_flat* f, const int32_t* trees, int32_t n, int32_t builder) {
  std::string err;
  const rtx_status st = flat_rebuild_instance_trees("rtx_flat_rebuild_instance_trees", f ? &f->scene : nullptr, f ? f->options : BuildOptions(),
                                                    trees, n, builder, &err);
  if (st != RTX_OK) set_error(err);
  return st;
}

rtx_status rtx_flat_instance_tree_cost(const rtx_flat* f, int32_t k, double* cost) {
  if (!f || !cost) { set_error("rtx_flat_instance_tree_cost: NULL argument"); return RTX_EINVAL; }
  const UpdateShadow sh = build_update_shadow(f->scene);
  if (!sh.broken.empty()) { set_error("rtx_flat_instance_tree_cost: " + sh.broken); return RTX_EINVAL; }
  if (k < 0 || (size_t)k >= sh.trees.size()) {
    set_error("rtx_flat_instance_tree_cost: k is out of range (the scene has " + std::to_string(sh.trees.size()) + " instance trees)");
    return RTX_EINVAL;
  }
  *cost = flat_instance_tree_cost(f->scene, sh.trees[(size_t)k]);
  return RTX_OK;
}

int64_t rtx_flat_triangle_ids(const rtx_flat* f, const rtx_builder* b, rtx_handle object, int32_t* ids, int64_t cap) {
  if (!f || !b || (!ids && cap > 0) || cap < 0) { set_error("rtx_flat_triangle_ids: NULL argument or cap < 0"); return -1; }
  std::string err;
  const int64_t n = flat_prim_ids(KIND_TRIANGLE, "rtx_flat_triangle_ids", f->scene, b->graph, object, ids, cap, &err);
  if (n < 0) set_error(err);
  return n;
}

rtx_status rtx_flat_set_triangles(rtx_flat* f, const int32_t* ids, int64_t n, const double* vertices) {
  std::string err;
  const rtx_status st = flat_set_triangles("rtx_flat_set_triangles", f ? &f->scene : nullptr, ids, n, vertices, &err);
  if (st != RTX_OK) set_error(err);
  return st;
}

int64_t rtx_flat_sphere_ids(const rtx_flat* f, const rtx_builder* b, rtx_handle object, int32_t* ids, int64_t cap) {
  if (!f || !b || (!ids && cap > 0) || cap < 0) { set_error("rtx_flat_sphere_ids: NULL argument or cap < 0"); return -1; }
  std::string err;
  const int64_t n = flat_prim_ids(KIND_SPHERE, "rtx_flat_sphere_ids", f->scene, b->graph, object, ids, cap, &err);
  if (n < 0) set_error(err);
  return n;
}

rtx_status rtx_flat_set_spheres(rtx_flat* f, const int32_t* ids, int64_t n, const double* spheres) {
  std::string err;
  const rtx_status st = flat_set_spheres("rtx_flat_set_spheres", f ? &f->scene : nullptr, ids, n, spheres, &err);
  if (st != RTX_OK) set_error(err);
  return st;
}

int64_t rtx_flat_moving_sphere_ids(const rtx_flat* f, const rtx_builder* b, rtx_handle object, int32_t* ids, int64_t cap) {
  if (!f || !b || (!ids && cap > 0) || cap < 0) { set_error("rtx_flat_moving_sphere_ids: NULL argument or cap < 0"); return -1; }
  std::string err;
  const int64_t n = flat_prim_ids(KIND_MOVING_SPHERE, "rtx_flat_moving_sphere_ids", f->scene, b->graph, object, ids, cap, &err);
  if (n < 0) set_error(err);
  return n;
}

rtx_status rtx_flat_set_moving_spheres(rtx_flat* f, const int32_t* ids, int64_t n, const double* movers) {
  std::string err;
  const rtx_status st = flat_set_moving_spheres("rtx_flat_set_moving_spheres", f ? &f->scene : nullptr, ids, n, movers, &err);
  if (st != RTX_OK) set_error(err);
  return st;
}

int64_t rtx_flat_rect_ids(const rtx_flat* f, const rtx_builder* b, rtx_handle object, int32_t* ids, int64_t cap) {
  if (!f || !b || (!ids && cap > 0) || cap < 0) { set_error("rtx_flat_rect_ids: NULL argument or cap < 0"); return -1; }
  std::string err;
  const int64_t n = flat_rect_ids("rtx_flat_rect_ids", f->scene, b->graph, object, ids, cap, &err);
  if (n < 0) set_error(err);
  return n;
}

rtx_status rtx_flat_set_rects(rtx_flat* f, const int32_t* ids, int64_t n, const double* rects) {
  std::string err;
  const rtx_status st = flat_set_rects("rtx_flat_set_rects", f ? &f->scene : nullptr, ids, n, rects, &err);
  if (st != RTX_OK) set_error(err);
  return st;
}

rtx_status rtx_flat_material_info(const rtx_flat* f, int32_t index, RtxMaterialInfo* o) {
  if (!f || !o) { set_error("rtx_flat_material_info: NULL argument"); return RTX_EINVAL; }
  const FlatScene& s = f->scene;
  if (index < 0 || (size_t)index >= s.materials.size()) {
    set_error("rtx_flat_material_info: index is out of range (the scene has " + std::to_string(s.materials.size()) + " materials)");
    return RTX_EINVAL;
  }
  const rt::FlatMaterial& m = s.materials[(size_t)index];
  o->kind = m.kind; o->tex = m.tex;
  for (int a = 0; a < 3; ++a) o->albedo[a] = m.albedo[a];
  o->param = m.param;
  return RTX_OK;
}

rtx_status rtx_flat_texture_info(const rtx_flat* f, int32_t index, RtxTextureInfo* o) {
  if (!f || !o) { set_error("rtx_flat_texture_info: NULL argument"); return RTX_EINVAL; }
  const FlatScene& s = f->scene;
  if (index < 0 || (size_t)index >= s.textures.size()) {
    set_error("rtx_flat_texture_info: index is out of range (the scene has " + std::to_string(s.textures.size()) + " textures)");
    return RTX_EINVAL;
  }
  const rt::FlatTexture& t = s.textures[(size_t)index];
  o->kind = t.kind; o->a = t.a; o->b = t.b; o->pad = 0;
  for (int a = 0; a < 3; ++a) o->color[a] = t.color[a];
  o->scale = t.scale;
  return RTX_OK;
}

rtx_status rtx_flat_medium_info(const rtx_flat* f, int32_t slot, RtxMediumInfo* o) {
  if (!f || !o) { set_error("rtx_flat_medium_info: NULL argument"); return RTX_EINVAL; }
  const FlatScene& s = f->scene;
  if (slot < 0 || (size_t)slot >= s.top_level.size()) {
    set_error("rtx_flat_medium_info: slot is out of range (the world list has " + std::to_string(s.top_level.size()) + " slots)");
    return RTX_EINVAL;
  }
  const rt::FlatEntry& E = s.entries[(size_t)s.top_level[(size_t)slot]];
  if (E.kind != rt::ENTRY_MEDIUM) { set_error("rtx_flat_medium_info: slot is not a ConstantMedium (rtx_flat_top_level_kind 4)"); return RTX_EINVAL; }
  o->material = E.b; o->pad = 0;
  o->neg_inv_density = E.f[0];
  return RTX_OK;
}

rtx_status rtx_flat_set_shading(rtx_flat* f, const RtxShadingEdit* edits, int64_t n) {
  std::string err;
  if (!flat_set_shading("rtx_flat_set_shading", f ? &f->scene : nullptr, edits, n, &err)) { set_error(err); return RTX_EINVAL; }
  return RTX_OK;
}

rtx_status rtx_flat_array(const rtx_flat* f, int32_t which, void* out, size_t bytes) {
  if (!f) { set_error("rtx_flat_array: NULL flat"); return RTX_EINVAL; }
  const FlatScene& s = f->scene;
  const void* p = nullptr;
  size_t have = 0;
  std::vector<rt::FlatLight> lights;  // 14: the light table as an upload would build it now (host/light_table.hpp)
  if (which == 14) {
    lights = build_light_table(s).lights;
    const rtx_status st = check_array_bytes("rtx_flat_array", lights.size() * sizeof(rt::FlatLight), out, bytes);
    if (st == RTX_OK && !lights.empty()) memcpy(out, lights.data(), lights.size() * sizeof(rt::FlatLight));
    return st;
  }
#define ARR(W, VEC) case W: p = s.VEC.data(); have = s.VEC.size() * sizeof(s.VEC[0]); break;
  switch (which) {
    ARR(0, entries) ARR(1, nodes) ARR(2, nodes32) ARR(3, motion32) ARR(5, top_level) ARR(6, member_local_box)
    ARR(10, triangles) ARR(11, top_box32) ARR(12, triangle_id) ARR(13, spheres) ARR(15, materials) ARR(16, textures)
    ARR(17, moving_spheres) ARR(19, rects)
    default: set_error("rtx_flat_array: which names no host array"); return RTX_EINVAL;
  }
#undef ARR
  const rtx_status st = check_array_bytes("rtx_flat_array", have, out, bytes);
  if (st == RTX_OK && have) memcpy(out, p, have);
  return st;
}

void rtx_ray_batch_defaults(RtxRayBatch* b) {
  if (!b) return;
  memset(b, 0, sizeof(*b));
  b->t_min = 0.001;
  b->t_max_all = HUGE_VAL;
  b->seed = 1;
}

void rtx_point_batch_defaults(RtxPointBatch* b) {
  if (!b) return;
  memset(b, 0, sizeof(*b));
  b->r_max_all = HUGE_VAL;
}

void rtx_radiance_rays_defaults(RtxRadianceRays* r) {
  if (!r) return;
  memset(r, 0, sizeof(*r));
  r->samples = 1;
  r->max_depth = 50;
  r->seed = 1;
  r->background[0] = 0.7; r->background[1] = 0.8; r->background[2] = 1.0;
}

void rtx_gather_points_defaults(RtxGatherPoints* g) {
  if (!g) return;
  memset(g, 0, sizeof(*g));
  g->samples = 1;
  g->max_depth = 50;
  g->seed = 1;
  g->background[0] = 0.7; g->background[1] = 0.8; g->background[2] = 1.0;
}

int32_t rtx_flat_top_level_kind(const rtx_flat* f, int32_t index) {
  if (!f || index < 0 || (size_t)index >= f->scene.top_level.size()) return -1;
  return f->scene.entries[f->scene.top_level[index]].kind;
}

// screen.rs:40-59 + vec3.rs:109-114: integer-valued channels printed without a decimal point.
rtx_status rtx_write_ppm(const char* path, int32_t width, int32_t height, const uint8_t* rgb8) {
  if (width <= 0 || height <= 0 || !rgb8) { set_error("rtx_write_ppm: bad argument"); return RTX_EINVAL; }
  FILE* fp = stdout;
  bool to_file = path && strcmp(path, "-") != 0;
  if (to_file) {
    fp = fopen(path, "wb");
    if (!fp) { set_error(std::string("rtx_write_ppm: cannot open ") + path); return RTX_EIO; }
  }
  std::string buf;
  buf.reserve((size_t)width * height * 12 + 32);
  char line[64];
  snprintf(line, sizeof(line), "P3\n%d %d\n255\n", width, height);
  buf += line;
  for (int32_t j = height - 1; j >= 0; --j) {
    for (int32_t i = 0; i < width; ++i) {
      const uint8_t* p = rgb8 + 3 * ((size_t)j * width + i);
      int n = snprintf(line, sizeof(line), "%u %u %u\n", (unsigned)p[0], (unsigned)p[1], (unsigned)p[2]);
      buf.append(line, (size_t)n);
    }
  }
  size_t wrote = fwrite(buf.data(), 1, buf.size(), fp);
  if (to_file) fclose(fp); else fflush(fp);
  if (wrote != buf.size()) { set_error("rtx_write_ppm: short write"); return RTX_EIO; }
  return RTX_OK;
}

const void* rtx_builder_graph(const rtx_builder* b) { return b ? (const void*)&b->graph : nullptr; }
const void* rtx_flat_arrays(const rtx_flat* f) { return f ? (const void*)&f->scene : nullptr; }

}  // extern "C"
