/* rtx_abi.h -- C ABI of the MI355X-native path-tracing hot path.
 *
 * The reference (patrickzbhe/ray-tracing-series-rust) has no FFI, plugin or operator
 * interface.  Its one seam around the hot path is
 *
 *     pub fn render_scene(world: Arc<Box<dyn Hittable + Sync>>, cam: Arc<Camera>,
 *                         background: Vec3, config: Config)        src/world.rs:1181-1186
 *
 * called from src/main.rs:13 after get_world_cam() (src/world.rs:876).  `dyn Hittable`
 * exposes only hit()/bounding_box() and all struct fields are private, so a Rust host can
 * hand its scene across a boundary only by walking its own constructors.  This header is
 * that boundary: one builder entry point per reference constructor (same argument order),
 * a flatten + upload step, and the render call that replaces render_scene's per-pixel x
 * per-sample loop (src/world.rs:1207-1226) with HIP kernels on gfx950.
 *
 * Conventions: C99, no exceptions or aborts cross this boundary; every call that can fail
 * returns an rtx_status (or a negative handle) and leaves a message for rtx_last_error().
 * Plain pointers and sizes only.  Structs are POD, little-endian, 8-byte aligned.
 * Handles (rtx_handle) are indices owned by one builder.  A builder is single-threaded.  An rtx_flat is immutable
 * after creation and may be shared between threads.  An rtx_scene's GEOMETRY is immutable, but the handle also owns the
 * render workspace (sample buffer, accumulators, work counter, timers): at most ONE render call may be in flight per
 * rtx_scene at a time -- calls on one handle must come from one thread at a time and, for rtx_render_device, on one
 * stream; concurrent renders of the same scene need one rtx_scene each (rtx_scene_upload is cheap next to a render).
 * A radiance query (rtx_scene_trace_rays*) uses that workspace and counts as a render call here; a ray query
 * (rtx_scene_cast_rays*) does not touch it.
 * The workspace is kept until rtx_scene_destroy or rtx_scene_trim (default budget of the sample buffer: 24 GiB).
 */
#ifndef RTX_ABI_H
#define RTX_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTX_ABI_VERSION 1

typedef int32_t rtx_status;
#define RTX_OK 0
#define RTX_EINVAL 1       /* bad argument; also the reference's assert!/panic! conditions */
#define RTX_ENOMEM 2
#define RTX_EHIP 3         /* a HIP runtime call failed (includes "no GPU") */
#define RTX_EUNSUPPORTED 4 /* scene shape outside what the kernels implement */
#define RTX_EIO 5          /* file could not be read/written (reference: expect()/unwrap() panics) */
#define RTX_ENCCL 6        /* RCCL could not be loaded, or a collective failed */

typedef int32_t rtx_handle; /* >= 0 valid, < 0 error */

typedef struct rtx_builder rtx_builder; /* scene graph under construction (host only) */
typedef struct rtx_flat rtx_flat;       /* flattened scene arrays + BVHs (host memory) */
typedef struct rtx_scene rtx_scene;     /* flattened scene resident in one GPU's HBM */

/* ---- library ------------------------------------------------------------------------ */
int32_t rtx_abi_version(void);
/* Thread-local; valid until the next failing call on the same thread. */
const char* rtx_last_error(void);

/* ---- scene construction: one entry point per reference constructor -------------------- */
/* scene_seed seeds the construction-time random stream (Perlin tables, catalogue scenes);
 * the reference uses rand::thread_rng() there. */
rtx_status rtx_builder_create(uint64_t scene_seed, rtx_builder** out);
void rtx_builder_destroy(rtx_builder* b); /* NULL-safe */
/* One uniform f64 in [0,1) from the construction stream (for host-side scene generators). */
double rtx_builder_random(rtx_builder* b);

/* Textures -- src/texture.rs */
rtx_handle rtx_solid_color(rtx_builder* b, const double rgb[3]);                 /* SolidColor::new            texture.rs:16-20  */
/* rtx_checker: checkers may nest, as in the reference, but a chain of at most 16 of them is followed when a texture is
 * evaluated (the reference recurses without limit).  Building a deeper texture succeeds; rtx_flatten refuses, with
 * RTX_EUNSUPPORTED and the depth in the message, a world in which a material reaches one. */
rtx_handle rtx_checker(rtx_builder* b, rtx_handle even, rtx_handle odd);        /* Checker::new               texture.rs:39-44  */
rtx_handle rtx_noise(rtx_builder* b, double scale);                             /* Noise::new (+Perlin::new)  texture.rs:72-77  */
rtx_handle rtx_image_from_ppm(rtx_builder* b, const char* path);                /* Image::from_ppm            texture.rs:95-99  */
rtx_handle rtx_image_from_texels(rtx_builder* b, int32_t width, int32_t height,
                                 const double* rgb_0_255);                      /* Screen contents, row 0 = first PPM row */
/* Materials -- src/hit.rs:992-1152 */
rtx_handle rtx_lambertian(rtx_builder* b, rtx_handle texture);                  /* Lambertian::from_pointer   hit.rs:1031-1035 */
rtx_handle rtx_metal(rtx_builder* b, const double albedo[3], double fuzz);      /* Metal::new                 hit.rs:1060-1065 */
rtx_handle rtx_dielectric(rtx_builder* b, double ir);                           /* Dielectric::new            hit.rs:1091-1093 */
rtx_handle rtx_diffuse_light(rtx_builder* b, rtx_handle texture);               /* DiffuseLight::from_pointer hit.rs:1140-1142 */
rtx_handle rtx_isotropic(rtx_builder* b, rtx_handle texture);                   /* Isotropic::from_color      hit.rs:997-1001  */
/* Hittables -- src/hit.rs, src/bvh.rs, src/model.rs */
rtx_handle rtx_sphere(rtx_builder* b, const double center[3], double radius, rtx_handle mat);          /* hit.rs:187-193 */
rtx_handle rtx_moving_sphere(rtx_builder* b, const double center0[3], const double center1[3],
                             double time0, double time1, double radius, rtx_handle mat);               /* hit.rs:257-273 */
/* GravitySphere::new(start, time0, radius, mat): the bouncing ball of the video scene; simulates and stores its ~100 002
 * heights at construction, as the reference does. */
rtx_handle rtx_gravity_sphere(rtx_builder* b, const double start[3], double time0, double radius, rtx_handle mat); /* hit.rs:340-367 */
rtx_handle rtx_triangle(rtx_builder* b, const double v0[3], const double v1[3], const double v2[3],
                        rtx_handle mat);                                                                /* hit.rs:96-107  */
rtx_handle rtx_xy_rect(rtx_builder* b, double x0, double x1, double y0, double y1, double k, rtx_handle mat); /* hit.rs:456-472 */
rtx_handle rtx_xz_rect(rtx_builder* b, double x0, double x1, double y0, double y1, double k, rtx_handle mat); /* hit.rs:521-537 */
rtx_handle rtx_yz_rect(rtx_builder* b, double x0, double x1, double y0, double y1, double k, rtx_handle mat); /* hit.rs:586-602 */
rtx_handle rtx_rect_prism(rtx_builder* b, const double p0[3], const double p1[3], rtx_handle mat);     /* hit.rs:720-775 */
rtx_handle rtx_hittable_list_new(rtx_builder* b);                                                       /* hit.rs:646-648 */
rtx_status rtx_hittable_list_add(rtx_builder* b, rtx_handle list, rtx_handle object);                   /* hit.rs:650-652 */
rtx_handle rtx_bvh_from_list(rtx_builder* b, rtx_handle list, double time0, double time1);              /* bvh.rs:85-93   */
/* An extension (no reference type): the HittableList of the list's members -- for every ray the hit of scanning them in
 * order, later member winning an exact tie (hit.rs:660-690) -- culled by a tree over the members' TRUE boxes (a RotateY
 * member's rotated box, which hit.rs:886 discards).  May stand where a slot of the world list may: in the world HittableList or
 * a list nested in it.  Members: primitives, RectPrisms, lists, BvhNodes of those, and up to 4 Translate / RotateY around one;
 * no ConstantMedium, nothing that holds a Moving- or GravitySphere, no other instance tree (rtx_flatten: RTX_EUNSUPPORTED).
 * The frame equals, bit for bit, that of the same world with the members written into the list at this position. */
rtx_handle rtx_instance_bvh_from_list(rtx_builder* b, rtx_handle list);
rtx_handle rtx_translate(rtx_builder* b, const double offset[3], rtx_handle object);                    /* hit.rs:793-798 */
rtx_handle rtx_rotate_y(rtx_builder* b, double angle_degrees, rtx_handle object);                       /* hit.rs:843-888 */
rtx_handle rtx_constant_medium(rtx_builder* b, const double rgb[3], double density, rtx_handle boundary); /* hit.rs:945-951 */
/* TriangleModel::load_from_file(path, scale).to_hittable() -> a HittableList of triangles (model.rs:13-76). */
rtx_handle rtx_triangle_model(rtx_builder* b, const char* path, double scale);
/* Same from memory: vertices = 3 doubles each, faces = 3 vertex indices each. */
rtx_handle rtx_triangle_mesh(rtx_builder* b, const double* vertices, int64_t n_vertices,
                             const int64_t* faces, int64_t n_faces, rtx_handle mat);

/* ---- camera and config --------------------------------------------------------------- */
/* The ten derived fields of src/camera.rs:6-17, as Camera::new computes them. */
typedef struct RtxCamera {
  double origin[3], lower_left_corner[3], horizontal[3], vertical[3], u[3], v[3], w[3];
  double lens_radius, time1, time2;
} RtxCamera;
/* Camera::new(lookfrom, lookat, vup, vfov, aspect_ratio, aperture, focus_dist, time1, time2)  camera.rs:20-57.
 * RTX_EINVAL if time1 >= time2 (gen_range(time1..time2) panics on an empty range, camera.rs:69). */
rtx_status rtx_camera_new(const double lookfrom[3], const double lookat[3], const double vup[3],
                          double vfov_degrees, double aspect_ratio, double aperture,
                          double focus_dist, double time1, double time2, RtxCamera* out);

/* Config::new(aspect_ratio, image_width, samples_per_pixel, max_depth, threads)  world.rs:20-50,
 * followed by the fields this build adds. */
typedef struct RtxConfig {
  double aspect_ratio;
  int32_t image_width;
  int32_t samples_per_pixel;
  int32_t max_depth;
  int32_t threads;          /* kept for API parity; only used by row_chunk_compat */
  uint64_t seed;            /* render seed of the counter-based per-(pixel,sample) streams */
  double background[3];     /* render_scene's `background` argument */
  int32_t row_chunk_compat; /* 1: leave rows >= threads*floor(h/threads) black (world.rs:1198-1202 quirk) */
  int32_t reserved;
  uint64_t sample_buffer_bytes; /* cap on the per-pass sample-radiance buffer; 0 = default */
} RtxConfig;
/* Fills the five reference fields, asserting what Config::new asserts (-> RTX_EINVAL), and
 * defaults: seed 1, background (0.7,0.8,1.0), row_chunk_compat 0. */
rtx_status rtx_config_new(double aspect_ratio, int32_t image_width, int32_t samples_per_pixel,
                          int32_t max_depth, int32_t threads, RtxConfig* out);
/* image_height = (image_width as f64 / aspect_ratio) as i32   world.rs:1192 */
int32_t rtx_image_height(const RtxConfig* cfg);

/* ---- scene catalogue: get_world_cam(config_num)  world.rs:876-1179 -------------------- */
typedef struct RtxSceneOptions {
  double camera_aspect;     /* <= 0: the reference's hard-coded aspect for that scene */
  const char* earth_ppm;    /* NULL or unreadable: procedural stand-in for "earthshit.ppm" */
  const char* dragon_ply;   /* NULL or unreadable: procedural stand-in mesh */
  int64_t mesh_triangles;   /* procedural mesh size; 0 = 871200 */
  int32_t book2_boxes_per_side; /* 0 = 20 */
  int32_t book2_spheres;        /* 0 = 1000 */
} RtxSceneOptions;
/* scene_id 0..12 and "anything else" as in the reference; 100 = canonical Book-1 final scene,
 * 101 = empty world.  options may be NULL. */
rtx_status rtx_get_world_cam(rtx_builder* b, int32_t scene_id, const RtxSceneOptions* options,
                             rtx_handle* world_out, RtxCamera* cam_out, double background_out[3]);

/* ---- flatten + upload ------------------------------------------------------------------ */
typedef struct RtxBuildOptions {
  int32_t max_leaf;      /* primitives per BVH leaf, 1..8; 0 = default (1; 2 for BVHs holding triangles) */
  int32_t sah_bins;      /* 0 = default */
  int32_t reference_bvh; /* 1: build BVHs with the reference's rule (bvh.rs:14-83) instead of SAH: same image,
                            different traversal statistics (A/B switch) */
  int32_t gpu_builder;   /* 1: BVHs of >= 1024 primitives are built on the CURRENT GPU (Morton clusters + radix tree + refit):
                            same image, milliseconds instead of a second for 871 200 triangles (replaces bvh.rs:14-83 at mesh
                            scale); rtx_flatten then needs a GPU (RTX_EUNSUPPORTED if the build cannot run) */
  uint64_t bvh_seed;     /* stream for the reference rule's random split axis */
} RtxBuildOptions;
typedef struct RtxFlatInfo {
  int64_t n_spheres, n_moving_spheres, n_rects, n_triangles;
  int64_t n_nodes, n_refs, n_entries, n_top_level, n_materials, n_textures, n_perlins, n_images, n_texels;
  int64_t total_bytes;
  int32_t max_stack, n_bvh;
  double sah_cost;
  double bvh_build_ms;  /* wall time of all BVH builds of this flatten (host SAH, reference rule or GPU builder) */
  double bvh_device_ms; /* GPU builder: device time by HIP events, box upload and node download included */
  int64_t n_gravity_spheres;
} RtxFlatInfo;
/* Host only (no GPU needed).  options may be NULL. */
rtx_status rtx_flatten(const rtx_builder* b, rtx_handle world, const RtxBuildOptions* options,
                       rtx_flat** out);
void rtx_flat_destroy(rtx_flat* f); /* NULL-safe */
rtx_status rtx_flat_info(const rtx_flat* f, RtxFlatInfo* out);
/* Kind of the index-th slot of the flattened world list (HittableList order, hit.rs:650-652): 0 primitive,
 * 1 ordered group (HittableList / RectPrism), 2 BVH, 3 Translate/RotateY chain, 4 ConstantMedium; -1 = index out
 * of range.  Inspection only (lets a host check that its scene flattened to the list it built). */
int32_t rtx_flat_top_level_kind(const rtx_flat* f, int32_t index);
/* Copies every array to the CURRENT HIP device. */
rtx_status rtx_scene_upload(const rtx_flat* f, rtx_scene** out);
/* The statistical fast mode.  The same scene, narrowed field by field to single precision, rendered by
 * the same kernels compiled with float arithmetic (csrc/hip/render_f32.hip): the image converges to the same picture
 * but is NOT bit-comparable with the reference's -- the bit-exactness this header promises elsewhere is about scenes
 * uploaded with rtx_scene_upload.  Every render entry point takes either kind of scene (rtx_multi_create_f32 for
 * several GPUs); rtx_render_count is f64 only.  The RNG stream per (pixel, sample), the sample order of the sums and the f64 accumulators
 * handed back are the same in both modes. */
rtx_status rtx_scene_upload_f32(const rtx_flat* f, rtx_scene** out);
int32_t rtx_scene_is_f32(const rtx_scene* s);
void rtx_scene_destroy(rtx_scene* s); /* NULL-safe */
/* Releases the render workspace of an idle scene (it is re-allocated by the next render); the geometry stays resident. */
rtx_status rtx_scene_trim(rtx_scene* s);

/* ---- render: replaces render_scene's sample loop ------------------------------------------- */
/* Pixel order everywhere: row-major, row j = 0 is the BOTTOM image row (Screen::update(j, i),
 * world.rs:1235; PPM output walks j downwards, screen.rs:43). */
typedef struct RtxFrame {
  double* accum_rgb; /* optional: h*w*3 per-pixel radiance sums over samples (before tone map) */
  uint8_t* rgb8;     /* optional: h*w*3 tone-mapped channels, get_normalized_color (vec3.rs:89-107) */
} RtxFrame;
/* Counters of one render (filled when requested; counting runs a separate instrumented kernel). */
typedef struct RtxRenderStats {
  uint64_t samples, rays, box_tests, sphere_tests, moving_sphere_tests, rect_tests, triangle_tests;
  uint64_t scatters, texels, perlin_calls;
  double trace_ms, reduce_ms, tonemap_ms; /* device time of the kernels of this render (HIP events) */
  int32_t trace_launches, passes;
  uint64_t sample_buffer_bytes;
  int32_t trace_kernel; /* which trace kernel the launcher chose: RTX_KERNEL_* (rtx_trace_kernel_name) */
  int32_t trace_variant; /* RTX_KERNEL_LDS: which instantiation ran, RTX_LDS_VARIANT_* bits; 0 for every other kernel */
} RtxRenderStats;
/* RtxRenderStats.trace_variant (all variants produce identical results; a frame cannot tell which ran, this word can) */
enum {
  RTX_LDS_VARIANT_TIME_BOXES = 1,   /* time-aware boxes: the shutter lies inside the (ordered) interval of the world's BVH */
  RTX_LDS_VARIANT_ONE_AXIS = 2,     /* ... whose slopes are zero except along y */
  RTX_LDS_VARIANT_COMMON_RATIO = 4  /* every MovingSphere has the same non-empty (time0, time1): one time ratio per bounce */
};
/* Trace kernels (all produce identical results; the launcher picks by world shape and LDS budget).  Ids 1, 2 and 5 are retired:
   their kernels were removed and the launcher never reports them; the ids and names stay reserved. */
enum {
  RTX_KERNEL_SIMPLE = 0,     /* grid-stride, one whole path per thread (also the counting kernel) */
  RTX_KERNEL_PERSISTENT = 1, /* retired: persistent waves + path regeneration, wave-synchronous list scan */
  RTX_KERNEL_STREAM = 2,     /* retired: stage-synchronous persistent kernel */
  RTX_KERNEL_VOTE = 3,       /* worlds that are one BVH: node/leaf voting walk, f32 culling, carry-over */
  RTX_KERNEL_LDS = 4,        /* RTX_KERNEL_VOTE with the geometry resident in LDS (sphere worlds that fit) */
  RTX_KERNEL_WQ = 5,         /* retired: workgroup-level path queues in LDS */
  RTX_KERNEL_WORLD = 6,      /* any world: per-lane scan of the world list, walks of every BVH entry carried over */
  RTX_KERNEL_WAVEFRONT = 7,  /* split-kernel integrator: path state in HBM, k_wf_generate / k_wf_trace / k_wf_shade per bounce */
  RTX_KERNEL_NEE = 8,        /* next-event estimation (rtx_render_ex with light_sampling = 1): persistent waves, whole paths per lane */
  RTX_KERNEL_RAYS = 9        /* radiance queries (rtx_scene_trace_rays*): RTX_KERNEL_NEE's scheduling, paths that start from the caller's rays */
};
const char* rtx_trace_kernel_name(int32_t kernel);
/* Blocking; host output buffers.  Renders the whole image on the current device. */
rtx_status rtx_render(const rtx_scene* s, const RtxCamera* cam, const RtxConfig* cfg, RtxFrame* out);

/* A shard = the image rows { j : (j / block_rows) % shard_count == shard_index }, compacted in
 * ascending j.  shard_count = 1 is the whole image. */
typedef struct RtxShard {
  int32_t shard_index, shard_count, block_rows, reserved;
} RtxShard;
int32_t rtx_shard_rows(const RtxConfig* cfg, const RtxShard* shard); /* number of rows in the shard */
/* Asynchronous on `hip_stream` (a hipStream_t, may be NULL = default stream); outputs are DEVICE
 * pointers sized for the shard (rows*w*3).  d_accum_rgb / d_rgb8 may each be NULL.  Scratch comes
 * from a per-scene workspace that grows on demand (the only call here that may allocate).
 * stats may be NULL; if non-NULL the call synchronises the stream to read timers.
 * One more host wait: on a scene whose k_trace_lds plan has time-aware boxes, the FIRST launch of that kernel after
 * rtx_scene_set_moving_spheres* waits once for the update to finish (see there). */
rtx_status rtx_render_device(const rtx_scene* s, const RtxCamera* cam, const RtxConfig* cfg,
                             const RtxShard* shard, double* d_accum_rgb, uint8_t* d_rgb8,
                             void* hip_stream, RtxRenderStats* stats);
/* Instrumented render of the same shard: fills the work counters of RtxRenderStats (blocking). */
rtx_status rtx_render_count(const rtx_scene* s, const RtxCamera* cam, const RtxConfig* cfg,
                            const RtxShard* shard, RtxRenderStats* stats);

/* ---- one process, several GPUs: replaces the band threads + collect loop of render_scene (world.rs:1198-1244) ---- */
/* The frame is cut into n_shards row-interleaved shards (RtxShard with shard_count = n_shards); shard r is rendered
 * by device device_ids[r] (NULL: device r) into that device's HBM, then ONE RCCL gather (ncclGather over xGMI, a
 * communicator from ncclCommInitAll) brings the shards to the first device, where they are put in row order and
 * copied to the host buffers of `out`.  The scene is uploaded to every device once, at creation, and stays resident
 * across renders.  device_ids must be all distinct -- or all equal, which renders the shards one after another on
 * that one GPU without the collective (a rehearsal of the sharding on a single-GPU box).  The frame is byte-identical
 * to rtx_render's for every shard count.  n_shards = 1 with one device goes through RCCL as well. */
typedef struct rtx_multi rtx_multi;
typedef struct RtxMultiStats {
  double render_ms_max;   /* slowest device, first launch to end of tone map (HIP events) */
  double total_ms;        /* host wall time of the call: launches + gather + reorder + copy to the host */
  uint64_t gathered_bytes;
  int32_t n_shards, n_devices, used_rccl;
  int32_t rccl_ranks;     /* ncclCommCount of the communicator the gather ran on (0 without one) */
  double gather_ms;       /* on the first device's stream: end of its own shard -> every shard gathered and put in row order
                             (includes waiting for the slowest peer) */
  double render_ms[16];   /* per device (first 16), as render_ms_max */
} RtxMultiStats;
rtx_status rtx_multi_create(const rtx_flat* f, int32_t n_shards, const int32_t* device_ids, int32_t block_rows,
                            rtx_multi** out);
/* The same with every shard's scene uploaded by rtx_scene_upload_f32 (the statistical fast mode). */
rtx_status rtx_multi_create_f32(const rtx_flat* f, int32_t n_shards, const int32_t* device_ids, int32_t block_rows,
                                rtx_multi** out);
void rtx_multi_destroy(rtx_multi* m); /* NULL-safe */
/* Blocking.  out->rgb8 and / or out->accum_rgb: host buffers of h*w*3 elements (row 0 = bottom row). stats may be NULL. */
rtx_status rtx_multi_render(rtx_multi* m, const RtxCamera* cam, const RtxConfig* cfg, RtxFrame* out, RtxMultiStats* stats);
/* Convenience: create on devices 0..n_gpus-1 (block_rows 1), render once, destroy. */
rtx_status rtx_render_multi(const rtx_flat* f, const RtxCamera* cam, const RtxConfig* cfg, int32_t n_gpus, RtxFrame* out);

/* ---- progressive rendering: one frame accumulated over several calls, with a noise estimate ----------------------- */
/* A handle owns the device accumulators of one (scene, camera, config, shard): S, the per-pixel sums of radiance, and Q,
 * their sums of squares.  cfg->samples_per_pixel is the BUDGET: rtx_progressive_add(p, n) traces the next n samples of
 * every pixel (absolute sample indices [spp_done, spp_done + n)) and returns RTX_EINVAL past the budget.  Random streams
 * are keyed by absolute (pixel, sample), and samples are added in sample order, so the frame after k samples is
 * bit-identical to a one-shot render at k spp however the k samples were split into calls.
 * The handle uses the scene's render workspace: it must not run concurrently with another render of the same scene on
 * another stream, and it must be destroyed before its scene.  Argument errors are reported before any device call. */
typedef struct rtx_progressive rtx_progressive;
typedef struct RtxNoiseStats {
  int32_t spp_done;      /* samples per pixel accumulated so far */
  int32_t pixels;        /* active pixels of the shard (row_chunk_compat's skipped rows excluded) */
  int32_t pixels_above;  /* pixels whose relative error r > target_rel_err */
  int32_t reserved;
  double max_rel_err, mean_rel_err, target_rel_err;
} RtxNoiseStats;
/* shard NULL = the whole image.  Blocking; allocates 48 bytes per pixel of the shard. */
rtx_status rtx_progressive_create(const rtx_scene* s, const RtxCamera* cam, const RtxConfig* cfg, const RtxShard* shard,
                                  rtx_progressive** out);
void rtx_progressive_destroy(rtx_progressive* p); /* NULL-safe */
int32_t rtx_progressive_spp(const rtx_progressive* p); /* samples per pixel so far (-1: NULL handle) */
/* Asynchronous on hip_stream (NULL = default stream) unless stats != NULL, as rtx_render_device.  1 <= n_samples <=
 * budget - spp_done.  A failed add leaves the handle unusable (every later call returns RTX_EINVAL). */
rtx_status rtx_progressive_add(rtx_progressive* p, int32_t n_samples, void* hip_stream, RtxRenderStats* stats);
/* Blocking.  out->accum_rgb (S), out->rgb8 (tone-mapped at spp_done; once a pixel has retired -- adaptive rounds below --
 * each pixel at its own count n_p) and sumsq_rgb (Q) are each optional host buffers of rows*w*3 elements in
 * rtx_render_device's shard layout.  Needs spp_done >= 1. */
rtx_status rtx_progressive_read(const rtx_progressive* p, RtxFrame* out, double* sumsq_rgb);
/* Blocking.  Per active pixel and channel, with n = spp_done >= 2:  m = S/n,  var = max(0, (Q - S*S/n) / (n - 1)),
 * se = sqrt(var / n),  r_c = se / (m + 1/256);  the pixel's r = max(0, max_c r_c), where a NaN r_c is ignored (a pixel
 * whose every r_c is NaN has r = 0).  Reports max r, mean r and the count of
 * r > target_rel_err (>= 0), reduced in a fixed order: the same bits on every call.  Once a pixel has retired (adaptive
 * rounds below), each pixel's r is taken at its own count n_p. */
rtx_status rtx_progressive_stats(rtx_progressive* p, double target_rel_err, RtxNoiseStats* out);
/* Blocking.  Adds `batch` samples at a time (the last batch clipped to the budget) and stops at the first batch boundary
 * where pixels_above == 0 (checked on entry too once spp_done >= 2), or at the budget.  out: the last stats. */
rtx_status rtx_progressive_until(rtx_progressive* p, int32_t batch, double target_rel_err, RtxNoiseStats* out);

/* Adaptive sampling: pixels that reach the target stop receiving samples.  An adaptive ROUND of n samples does two things:
 *  1. Retirement check, only when spp_done >= max(2, min_spp): every still-active pixel gets its r (the formula of
 *     rtx_progressive_stats, n = spp_done); a pixel with r <= target_rel_err RETIRES: its count n_p is frozen at spp_done and
 *     it never receives another sample (its S and Q no longer change, so it stays retired).
 *  2. Tracing: the absolute samples [spp_done, spp_done + n) of the still-active pixels only (spp_done then advances by n,
 *     even when no pixel is active).
 * Every active pixel therefore holds spp_done samples, and a pixel that stopped at n_p holds exactly the bits a uniform
 * render at n_p spp gives it.  The first adaptive call allocates 4 * (2 * pixels + pixels of the shard) bytes and a little
 * scratch; until a pixel retires, the handle behaves as a uniform one.  Once one has, rtx_progressive_add and
 * rtx_progressive_until return RTX_EINVAL (they would leave a gap in the retired pixels' sample indices);
 * rtx_progressive_read, _stats and _pixel_spp take each pixel at its own n_p.
 * Argument errors (NULL handle, n_samples or batch <= 0, min_spp < 2 or above the budget, a negative or NaN target, past the
 * budget) are reported before any device call. */
typedef struct RtxAdaptiveStats {
  int32_t spp_done;       /* samples of every still-active pixel */
  int32_t min_spp;        /* the rule's min_spp and target, as passed */
  int32_t pixels;         /* pixels of the shard (row_chunk_compat's skipped rows excluded) */
  int32_t pixels_active;  /* of which not retired */
  int32_t pixels_above;   /* pixels whose r > target_rel_err, each at its own n_p */
  int32_t reserved;
  uint64_t samples;       /* sum of n_p over the pixels: the (pixel, sample) paths the frame holds */
  double max_rel_err, mean_rel_err;  /* of r, each pixel at its own n_p; reduced in a fixed order (the same bits every call) */
  double target_rel_err;
} RtxAdaptiveStats;
/* One adaptive round (1 <= n_samples <= budget - spp_done).  The retirement check blocks (the host needs the count of the
 * pixels left); the tracing is asynchronous on hip_stream unless stats != NULL, as rtx_progressive_add.  stats->samples:
 * the paths this round traced. */
rtx_status rtx_progressive_add_adaptive(rtx_progressive* p, int32_t n_samples, int32_t min_spp, double target_rel_err,
                                        void* hip_stream, RtxRenderStats* stats);
/* Blocking.  Rounds of `batch` samples (the last one clipped to the budget) until no pixel is active; at the budget, a final
 * retirement check, so that out describes the finished frame. */
rtx_status rtx_progressive_until_adaptive(rtx_progressive* p, int32_t batch, int32_t min_spp, double target_rel_err,
                                          RtxAdaptiveStats* out);
/* Blocking.  spp: a host buffer of rows*w counts in rtx_render_device's shard layout -- n_p of every pixel (spp_done for one
 * still active, and for every pixel of a handle that never ran an adaptive round); rows skipped by row_chunk_compat get 0. */
rtx_status rtx_progressive_pixel_spp(const rtx_progressive* p, int32_t* spp);

/* ---- denoising a progressive frame ---------------------------------------------------------------------------------- */
/* An extension: a denoised image is a new, separate output of a handle, STATISTICAL like the f32 mode (no bit-exactness
 * claim against any reference).  It leaves S, Q, the counts and spp_done untouched: later rtx_progressive_add and
 * _add_adaptive calls behave exactly as if it had never run.
 * Features: for each feature sample s in [0, feature_spp), the primary ray of path sample s (the same jitter, lens sample and
 * shutter time) and its first world hit on that path's stream, averaged per pixel:
 *   albedo  Lambertian / Isotropic: the texture's colour at the hit (scatter's attenuation); Metal: its albedo;
 *           Dielectric, DiffuseLight: (1, 1, 1); a miss: the config's background;
 *   normal  the hit record's face-forwarded normal; (0, 0, 0) for an Isotropic hit and for a miss.
 * They depend on (scene, camera, config) only; a handle computes them on its first denoise / features call (32 bytes per
 * pixel, kept while feature_spp stays the same).
 * Filter: an edge-avoiding a-trous wavelet filter steered by each pixel's variance (Dammertz et al. 2010; Schied et al.
 * 2017).  Per pixel p at its own count n (spp_done, or n_p once it has retired):
 *   prepare (f64 -> f32)  m = S/n,  v_c = max(0, (Q - S*S/n)/(n - 1))/n  (rtx_progressive_stats' operations);
 *                         demodulated (the default): a = max(A, 1e-3) per channel, c0 = m/a, v_c = v_c/a^2, else c0 = m;
 *                         sigma2 = 0.2126^2 v_r + 0.7152^2 v_g + 0.0722^2 v_b (channel covariances ignored);
 *                         n^ = N/|N| if |N| >= 1e-3, else 0.
 *   level k = 0..K-1 (f32), step t = 2^k: taps q = p + t(dx, dy), dx, dy in -2..2, those outside the image skipped,
 *                         h = (1/16, 1/4, 3/8, 1/4, 1/16), l(c) = 0.2126 r + 0.7152 g + 0.0722 b,
 *                         w = h_dx h_dy exp(-|l(c_p) - l(c_q)| / (sigma_l sqrt(sigma2_p) + 1e-4) - |A_p - A_q|^2 / sigma_a^2) W_n,
 *                         W_n = 1 if both n^ are 0, 0 if exactly one is, else max(0, min(1, n^_p . n^_q))^sigma_n;
 *                         the centre tap's w is (3/8)^2 (its own colour and normal: e = 0, W_n = 1);
 *                         c' = sum w c_q / sum w,  sigma2' = sum w^2 sigma2_q / (sum w)^2  (taps summed dy outer, dx inner).
 *   finish                mean = c_K a (demodulated) or c_K; rgb8 = the tone map of a 1-sample sum (sqrt, clamp, * 255.9).
 * The same inputs give the same bits on every call.  Parameters (0 = the default): iterations K = 5 (1..8), feature_spp = 4
 * (1..64), sigma_luminance = 4, sigma_normal = 32, sigma_albedo = 0.3 (each in [0, 1e30]), demodulate 0 or 1 = on,
 * -1 = off.  NULL pointers (outputs excepted), parameters out of range and spp_done < 2 are RTX_EINVAL before any device
 * call; a sharded handle (shard_count > 1) or one with row_chunk_compat is RTX_EUNSUPPORTED (rows are missing there, and the
 * filter needs every neighbour). */
typedef struct RtxDenoiseParams {
  int32_t iterations, feature_spp, demodulate, reserved; /* 0 = default; reserved is ignored */
  double sigma_luminance, sigma_normal, sigma_albedo;    /* 0 = default */
} RtxDenoiseParams;
/* Blocking.  albedo_rgb, normal_xyz: optional host buffers of rows*w*3 floats in rtx_render_device's layout.  The feature
 * pass of feature_spp (1..64) samples. */
rtx_status rtx_progressive_features(rtx_progressive* p, int32_t feature_spp, float* albedo_rgb, float* normal_xyz);
/* Blocking; waits for adds still running on any stream.  Needs spp_done >= 2; params NULL = the defaults.  mean_rgb
 * (rows*w*3 doubles): the denoised per-pixel MEAN radiance (not a sum); rgb8 (rows*w*3): its tone map.  Both optional. */
rtx_status rtx_progressive_denoise(rtx_progressive* p, const RtxDenoiseParams* params, double* mean_rgb, uint8_t* rgb8);
/* Self-test: the filter above (prepare from m and v, the levels, finish) on host arrays of width*height pixels, through the
 * handle's own launch sequence.  mean_rgb, var_rgb (the variance of the mean, per channel): doubles; albedo_rgb, normal_xyz:
 * floats; 3 per pixel, row-major.  out_mean_rgb and out_rgb8 optional.  Blocking. */
rtx_status rtx_device_denoise(const double* mean_rgb, const double* var_rgb, const float* albedo_rgb, const float* normal_xyz,
                              int32_t width, int32_t height, const RtxDenoiseParams* params, double* out_mean_rgb,
                              uint8_t* out_rgb8);

/* ---- light sampling: next-event estimation with multiple importance sampling ---------------------------------------- */
/* An extension: a second, opt-in estimator, STATISTICAL like the f32 mode and the denoiser (no bit-exactness claim against
 * the reference).  The reference's estimator (world.rs:52-93) finds a light only when a scattered ray happens to hit it.
 * With light_sampling = 1, every Lambertian and Isotropic vertex also connects to a point sampled on a light:
 *   light table  the top-level slots that are a plain XyRect / XzRect / YzRect or a static Sphere with a DiffuseLight material
 *                (no transform, no medium around them).  Every other emitter -- in a BVH or a group, wrapped, moving, gravity,
 *                triangle -- is an unsampled emitter, reached by the material's own sampling with weight 1.  Light k is picked
 *                with probability proportional to area x the max channel of its emitted colour at its centre (uniform when
 *                every such product is 0).  Built on the host (rtx_flat_lights reports it), uploaded on first use, freed
 *                with the scene.
 *   per vertex   after the material's scatter has drawn (the reference's order), and only when the path may take another
 *                bounce (depth - 1 >= 0, the rule of world.rs:64-67: the connection counts as the next hit): one uniform
 *                picks the light, two more a point q on it -- a rectangle uniformly over its area (solid-angle pdf
 *                d^2 / (|cos theta_l| A), both faces emit), a sphere uniformly over the cone it subtends (pdf 1 / (2 pi
 *                (1 - cos theta_max)); 0 from inside it).  A shadow ray p -> q (direction q - p, the path's shutter time)
 *                over t in [0.001, 1 - 1e-6] is occluded by any accepted hit, a ConstantMedium's random hit included (it
 *                draws from the path's stream).  Unoccluded, the vertex adds product x f x Le x w_light / p_light with
 *                f = albedo max(0, cos) / pi (Lambertian, about the hit record's normal) or albedo / (4 pi) (Isotropic),
 *                Le the light's texture at q and w_light = p_light^2 / (p_light^2 + p_bsdf^2) (power heuristic).
 *   light hits   a scattered ray from a Lambertian / Isotropic vertex that hits a sampled light scales its emitted radiance
 *                by p_bsdf^2 / (p_bsdf^2 + p_light^2), p_light that light's pdf at that point; emitters reached from the
 *                camera, from Metal or Dielectric vertices, and unsampled emitters keep weight 1.
 * With an empty light table the estimator draws and adds exactly what the reference's does: the frame is bit-identical to
 * rtx_render's.  Results are deterministic and independent of how samples are split into calls or shards.  The f32 mode,
 * rtx_multi_*, rtx_render_count and the wavefront integrator have no light sampling. */
typedef struct RtxIntegratorOptions {   /* 16 B */
  int32_t light_sampling;  /* 0: the reference's estimator (what rtx_render does); 1: next-event estimation + MIS */
  int32_t reserved[3];     /* must be 0 */
} RtxIntegratorOptions;
typedef struct RtxLightInfo {
  int32_t n_lights, n_rect_lights, n_sphere_lights, n_unsampled_emitters;
  double total_area;       /* summed area of the sampled lights */
} RtxLightInfo;
/* Host only: no GPU needed.  The census of the light table above. */
rtx_status rtx_flat_lights(const rtx_flat* f, RtxLightInfo* out);
/* Host only: the census of a flattened scene's instance trees (rtx_instance_bvh_from_list).  A tree of fewer than two members
 * leaves no tree behind (its member is a plain slot) and is not counted. */
typedef struct RtxInstanceInfo {
  int32_t n_trees;     /* instance trees of two or more members */
  int32_t n_members;   /* their member slots, summed */
  int32_t n_nodes;     /* nodes of their culling trees, summed */
  int32_t max_depth;   /* the deepest of those trees (stack entries its walk can hold) */
} RtxInstanceInfo;
rtx_status rtx_flat_instances(const rtx_flat* f, RtxInstanceInfo* out);
/* rtx_render with options: opt NULL or light_sampling = 0 is rtx_render exactly.  stats may be NULL.  A light_sampling other
 * than 0 / 1 or a non-zero reserved word is RTX_EINVAL before any device call; an f32 scene with light_sampling = 1 is
 * RTX_EUNSUPPORTED.  Blocking, host output buffers. */
rtx_status rtx_render_ex(const rtx_scene* s, const RtxCamera* cam, const RtxConfig* cfg,
                         const RtxIntegratorOptions* opt, RtxFrame* out, RtxRenderStats* stats);
/* rtx_progressive_create with options (same errors as rtx_render_ex).  A handle made with light sampling uses it for every
 * add -- uniform, adaptive and until; its stats, read and denoise are unchanged. */
rtx_status rtx_progressive_create_ex(const rtx_scene* s, const RtxCamera* cam, const RtxConfig* cfg,
                                     const RtxShard* shard, const RtxIntegratorOptions* opt, rtx_progressive** out);

/* ---- ray queries: closest-hit casts of ray batches on a resident scene ------------------------------------------------ */
/* An extension: the caller's own rays against a resident scene -- picking, depth and visibility maps, occlusion, range
 * sensors, collision probes.  Ray r of a batch is ONE call
 *     world_hit(scene, Ray(origin_r, direction_r, time_r), t_min, t_max_r, rng_r)
 * of the shared core (HittableList::hit, hit.rs:660-690): the call a path's bounce makes.  A ConstantMedium answers with its
 * random hit, drawn from rng_r = rng_for_sample(seed + r * stream_step, 0, 0): stream_step 0 gives every ray the stream of
 * the CPU checkers' probe, 1 a stream per ray.  There is no any-hit walk (it would change what a medium draws): an occlusion
 * query is a cast that asks for `ids` alone.  Rays and results are f64 columns for both kinds of scene; an f32 scene narrows
 * each ray component, t_min and t_max to float (the conversion of its camera rays) and widens what it writes.
 * Results are deterministic and do not depend on how a batch is split into calls, provided the seed of a call whose first ray
 * is ray `first` of the batch is seed + first * stream_step.
 * On a scene with GravitySpheres a ray whose time lies more than 10 s past the spheres' stored trajectory is not cast (the
 * reference's brute-force loop is unbounded there) and reports a miss.
 * RTX_EINVAL before any device call: a NULL scene, batch or hits; n < 0; n > 0 with a NULL origin or direction; a NaN t_min or
 * t_max_all -- the message names the field.  n = 0 is RTX_OK: nothing is launched, nothing written.  An all-NULL RtxRayHits
 * with n > 0 is legal (a timing run).  Since then an any-hit walk exists that returns what the medium's draw is a sample of:
 * the section "occlusion queries" below (rtx_scene_occlusion*). */
typedef struct RtxRayBatch {
  int64_t n;                 /* rays */
  const double* origin;      /* [n][3] */
  const double* direction;   /* [n][3], not normalised, as Ray::new takes it */
  const double* time;        /* [n] or NULL: every ray at time 0 */
  const double* t_max;       /* [n] or NULL: every ray to t_max_all */
  double t_min, t_max_all;   /* the interval world_hit is called with; rtx_ray_batch_defaults: 0.001, +inf */
  uint64_t seed;             /* rtx_ray_batch_defaults: 1 */
  uint64_t stream_step;      /* 0: one stream for every ray; 1: a stream per ray */
} RtxRayBatch;
typedef struct RtxRayHits {  /* any pointer may be NULL: that column is not written */
  double* t;                 /* [n]    +inf on a miss */
  double* p;                 /* [n][3] HitRecord p      (0 on a miss) */
  double* normal;            /* [n][3] HitRecord normal, face-forwarded as the record holds it (0 on a miss) */
  double* uv;                /* [n][2] HitRecord u, v   (0 on a miss) */
  int32_t* ids;              /* [n][4] {hit 0/1, material index of the flat scene, top-level slot, front_face}; miss: {0,-1,-1,0} */
} RtxRayHits;
/* Rays staged per slice by the host entry: at most RTX_CAST_HOST_SLICE * 144 bytes of device memory (56 in, 88 out a ray),
 * whatever n is. */
#define RTX_CAST_HOST_SLICE 262144
/* Zeroes *b, then t_min = 0.001, t_max_all = +inf, seed = 1, stream_step = 0. */
void rtx_ray_batch_defaults(RtxRayBatch* b);
/* Host pointers, blocking. */
rtx_status rtx_scene_cast_rays(const rtx_scene* s, const RtxRayBatch* rays, const RtxRayHits* hits);
/* Device pointers, asynchronous on hip_stream: returns after the launch.  uv and ids are stored 16 bytes at a time and must
 * be 16-byte aligned, every other column 8: RTX_EINVAL naming the column otherwise, before any device call.  A batch of more
 * than 2^30 rays goes out as several launches, none indexing past 2^31 rays. */
rtx_status rtx_scene_cast_rays_device(const rtx_scene* s, const RtxRayBatch* rays, const RtxRayHits* hits, void* hip_stream);

/* ---- occlusion queries: any-hit segment casts with exact fog depth ----------------------------------------------------- */
/* An extension: is the segment [t_min, t_max_r] of ray r free, and how much fog lies on it -- shadows, ambient occlusion, line
 * of sight, light baking through media.  The batch is the RtxRayBatch of a cast (seed and stream_step are not read); the
 * result is ONE double per ray, tau[r]:
 *   +inf  when some non-medium top-level entry has a primitive that prim_t accepts in [t_min, t_max_r] -- the test world_hit
 *         applies, with t_max never narrowed.  The walk returns at the first such primitive (an any-hit walk: no near-first
 *         order, no record); WHICH surface blocked is not reported, it would depend on the visiting order.
 *   else  the sum over the ConstantMedium slots of the world list, in ascending slot order starting from +0.0, of each slot's
 *         optical depth.  The boundary is asked exactly as world_hit asks it: two closest queries, rec1 over (-inf, inf) and rec2
 *         from rec1.t + 0.0001.  t1 = max(rec1.t, t_min), t2 = min(rec2.t, t_max_r); the slot contributes nothing if a query
 *         misses or t1 >= t2; t1 < 0 becomes 0; the depth is ((t2 - t1) * length(direction)) / (-neg_inv_density) with the
 *         entry's f[0] as stored: one subtraction, one multiplication, one division.  Density 0 is stored as -inf and gives
 *         depth +0.  An INFINITE density gives +inf, indistinguishable from a blocker.
 *   NaN   on a scene with GravitySpheres for a ray whose time lies more than 10 s past the spheres' stored trajectory: a ray
 *         that was not tested must not read as clear (rtx_scene_trace_rays' rule, not the cast's "miss").
 * ConstantMedium::hit misses with probability exp(-density * distance_inside), so the transmittance of the segment is
 * exp(-tau): the expectation of "the closest-hit cast reports no hit at all" over independent streams (stream_step = 1),
 * the product over overlapping media included.  It is computed by the caller, never on the device.  On a scene without media,
 * or whose media all have density 0, isinf(tau[r]) equals ids[r][0] == 1 of rtx_scene_cast_rays for every ray.
 * No draw is made and only + - * / and sqrt are used: results are deterministic, independent of how a batch is split into
 * calls, and equal to the CPU core's (core/occlusion.hpp: world_occlusion) bit for bit in f64 and in f32.  An f32 scene
 * narrows the ray, t_min and t_max with the cast's conversions and widens tau.
 * The query does not use the render workspace and may run beside a render, as the cast does.
 * RTX_EINVAL before any device call and before the handle is read: a NULL scene, batch or tau; n < 0; n > 0 with a NULL origin
 * or direction; a NaN t_min or t_max_all -- the message names the field.  n = 0 is RTX_OK: nothing is launched, nothing
 * written. */
/* Host pointers, blocking; staged in slices of RTX_CAST_HOST_SLICE rays (56 B in, 8 B out a ray). */
rtx_status rtx_scene_occlusion(const rtx_scene* s, const RtxRayBatch* rays, double* tau);
/* Device pointers, asynchronous on hip_stream: returns after the launch.  d_tau and every ray column must be 8-byte aligned:
 * RTX_EINVAL naming the pointer otherwise, before any device call.  A batch of more than 2^30 rays goes out as several
 * launches. */
rtx_status rtx_scene_occlusion_device(const rtx_scene* s, const RtxRayBatch* rays, double* d_tau, void* hip_stream);

/* ---- radiance queries: the estimator's radiance along a caller's rays on a resident scene ------------------------------ */
/* An extension: what the path tracer gathers along the caller's own rays -- fisheye, equirectangular or orthographic cameras,
 * light-map and irradiance-probe bakes, radiance caches, sensor models.  Sample s of ray r is ONE path of the estimator
 * (ray_color's loop, world.rs:52-93; with light_sampling = 1 the estimator of RtxIntegratorOptions) that starts from
 * Ray(origin_r, direction_r, time_r) AS GIVEN: no jitter, lens or shutter draw is made, so the first draw of its stream
 *     rng_for_sample(seed, first_ray + r, first_sample + s)
 * belongs to the first bounce.  sum_rgb[r] is the sum of the ray's samples added in ascending sample order and sumsq_rgb[r]
 * the per-channel sum of their squares (Q of the progressive interface; square and add separately rounded).  Rays are f64
 * columns for both kinds of scene; an f32 scene narrows each ray component to float and its sums add widened floats.
 * THE CONTRACT: a ray's sums depend only on (scene, ray, first_ray + r, seed, the sample range, max_depth, background,
 * estimator) -- not on how the batch is cut into calls, staging slices, launches or passes.  With accumulate = 1, two calls
 * over the samples [0, a) and [a, a + b) leave the bits of one call over [0, a + b).
 * On a scene with GravitySpheres a ray whose time lies more than 10 s past the spheres' stored trajectory is not traced (the
 * reference's brute-force loop is unbounded there): every sample of it is NaN, so its sums are NaN -- not a dark ray.
 * A radiance query uses the scene's render workspace: the one-render-in-flight-per-rtx_scene rule at the top of this header
 * applies to it (rtx_scene_cast_rays* does not use the workspace and may run beside it).
 * RTX_EINVAL before any device call, the message naming the field: a NULL scene, struct or sum_rgb; n < 0; n > 0 with a NULL
 * origin or direction; samples < 1; max_depth < 1; a non-zero reserved; a light_sampling or accumulate other than 0 / 1; a
 * NaN background; first_sample + samples past 2^32; (device entry) a pointer that is not 8-byte aligned.  An f32 scene with
 * light_sampling = 1 is RTX_EUNSUPPORTED.  n = 0 is RTX_OK: nothing is launched, nothing written. */
typedef struct RtxRadianceRays {   /* 104 B */
  int64_t n;                 /* rays */
  const double* origin;      /* [n][3] */
  const double* direction;   /* [n][3], not normalised, as Ray::new takes it */
  const double* time;        /* [n] or NULL: every ray at time 0 */
  uint64_t first_ray;        /* index of ray 0 in the caller's whole batch: the stream key's pixel word */
  uint32_t first_sample;     /* absolute index of the first sample traced by this call */
  int32_t samples;           /* >= 1 */
  int32_t max_depth;         /* >= 1, Config::new's rule */
  int32_t accumulate;        /* 0: sums start at 0; 1: sum_rgb / sumsq_rgb are continued in place */
  uint64_t seed;
  double background[3];
  int32_t light_sampling;    /* RtxIntegratorOptions' meaning; f32 scene with 1: RTX_EUNSUPPORTED */
  int32_t reserved;          /* must be 0 */
  uint64_t sample_buffer_bytes; /* RtxConfig's meaning: 0 = the default budget */
} RtxRadianceRays;
/* Rays staged per slice by the host entry: at most RTX_TRACE_HOST_SLICE * 104 bytes of device memory (56 in, 48 of sums a ray)
 * beside the workspace, whatever n is.  Slice k traces with first_ray + its offset. */
#define RTX_TRACE_HOST_SLICE 262144
/* Zeroes *r, then samples = 1, max_depth = 50, seed = 1, background = (0.7, 0.8, 1). */
void rtx_radiance_rays_defaults(RtxRadianceRays* r);
/* Host pointers, blocking.  sum_rgb [n][3] is required, sumsq_rgb [n][3] and stats are optional.  stats->trace_kernel is
 * RTX_KERNEL_RAYS, stats->samples = n * samples. */
rtx_status rtx_scene_trace_rays(const rtx_scene* s, const RtxRadianceRays* rays, double* sum_rgb, double* sumsq_rgb,
                                RtxRenderStats* stats);
/* Device pointers, asynchronous on hip_stream: returns after the launches unless stats is not NULL, which synchronises (as in
 * rtx_render_device).  A batch of more than 2^30 rays goes out as several launches; a pass's (sample, ray) index space stays
 * below 0xFFFF0000. */
rtx_status rtx_scene_trace_rays_device(const rtx_scene* s, const RtxRadianceRays* rays, double* d_sum_rgb, double* d_sumsq_rgb,
                                       void* hip_stream, RtxRenderStats* stats);

/* ---- gather queries: light arriving at a caller's points, the start directions drawn on the device --------------------- */
/* An extension: what a light-map or an irradiance-probe bake asks of a resident scene.  A radiance query takes every ray as
 * given, so a bake would upload one ray per (point, direction); a gather query takes the POINTS (56 B each, whatever the
 * sample count) and draws each sample's start direction from the sample's own stream.  Two forms share one rule:
 *   surface gather (normal not NULL): the path starts as if it had just scattered off a white Lambertian surface at p with
 *     normal n.  The mean sample is E / pi, the radiosity of a white diffuse texel: irradiance = pi * sum / samples.
 *   probe gather (normal NULL): the start direction is uniform over the sphere.  Mean radiance = sum / samples, fluence
 *     4 pi times that.  With sh_order = 1 | 2 every sample is projected on the device onto the real orthonormal spherical
 *     harmonics of orders 0..sh_order (K = 4 or 9 coefficients per channel): coefficient estimate = 4 pi * S / samples.
 * MEANING.  Sample s of point r is one path of core/integrator.hpp (trace_gather_sample[_nee]):
 *     rng     = rng_for_sample(seed, first_point + r, first_sample + s)
 *     u       = random_unit_vector(rng)          -- the reference's rejection loop: the FIRST draws of the stream
 *     surface : dir = normal_r + u; if near_zero(dir) dir = normal_r        (Lambertian::scatter's rule, hit.rs:1039-1051)
 *     probe   : dir = u
 *     ray     = Ray(p_r, dir, time_r); product = (1, 1, 1); output = 0; depth = max_depth
 *     surface and light_sampling = 1 and the scene has sampled lights:
 *               output += the light connection of a Lambertian vertex {p_r, normal_r} of albedo (1, 1, 1), made after the
 *               scatter draw; the first ray carries that vertex' pdf (the power heuristic weighs a light it hits)
 *     then the estimator's bounce loop to the end, unchanged (ray_color's, world.rs:52-93; light_sampling = 1:
 *     RtxIntegratorOptions').
 * The normal is taken AS GIVEN and is not normalised, as Ray::new takes a direction; no two-sided flip is made.  The ray
 * leaves p with the path's own t_min, so a point that lies on a surface does not hit that surface.  A gather through a
 * non-white albedo is the caller's multiplication.  Only a UNIT normal makes the start direction the cosine lobe: E / pi is
 * what a unit normal gathers, and with light_sampling = 1 the start vertex weighs its two strategies by that lobe's density,
 * so a normal of another length biases it (a zero normal -- what a cast reports for a hit inside a medium -- gathers
 * uniformly over the sphere and, with light sampling, loses the direct light of its first segment).
 * PLAIN OUTPUT (sh_order = 0): sum [n][3] and the optional sumsq [n][3], added in ascending sample order, the square and the
 * add separately rounded -- rtx_scene_trace_rays' rule.
 * SH OUTPUT (sh_order = 1 | 2, probe form only; with normals RTX_EINVAL): with K = 4 or 9, sum [n][K][3] and the optional
 * sumsq [n][K][3] are updated for s ascending, then i = 0 .. K-1, then c = 0 .. 2 by
 *     v = Y_i(dir_s) * L_s[c];  S += v;  Q += v * v            (every operation separately rounded in f64)
 * Y_i is the real orthonormal basis in the order (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2), evaluated on
 * the start direction (a unit vector); core/sh_basis.hpp holds its constants as double literals and fixes its order of
 * operations.
 * Points are f64 columns for both kinds of scene.  An f32 scene is supported with light_sampling = 0: p and n are narrowed
 * with a (float) cast, the samples are widened before they are added, and the direction that enters Y_i is the float
 * direction, widened.
 * THE CONTRACT (rtx_scene_trace_rays'): a point's sums depend only on (scene, point, first_point + r, seed, the sample range,
 * max_depth, background, estimator, form, sh_order) -- not on how the batch is cut into calls, staging slices, launches or
 * passes.  With accumulate = 1, two calls over the samples [0, a) and [a, a + b) leave the bits of one call over [0, a + b).
 * A point later than a GravitySphere scene's time limit gives NaN sums (rtx_scene_trace_rays' rule).  The query uses the
 * scene's render workspace: the one-render-in-flight-per-rtx_scene rule applies.
 * RTX_EINVAL before any device call, the message naming the field: a NULL scene, struct or sum; n < 0; n > 0 with a NULL
 * position; samples < 1; max_depth < 1; a non-zero reserved word; a light_sampling or accumulate other than 0 / 1; an
 * sh_order other than 0 / 1 / 2; sh_order > 0 with normals; a NaN background; first_sample + samples past 2^32; (device
 * entry) a pointer that is not 8-byte aligned.  An f32 scene with light_sampling = 1 is RTX_EUNSUPPORTED.  n = 0 is RTX_OK:
 * nothing is launched, nothing written. */
typedef struct RtxGatherPoints {   /* 112 B */
  int64_t n;                 /* points */
  const double* position;    /* [n][3] */
  const double* normal;      /* [n][3], not normalised: the surface form; NULL: the probe form */
  const double* time;        /* [n] or NULL: every point at time 0 */
  uint64_t first_point;      /* index of point 0 in the caller's whole batch: the stream key's pixel word */
  uint32_t first_sample;     /* absolute index of the first sample traced by this call */
  int32_t samples;           /* >= 1 */
  int32_t max_depth;         /* >= 1: bounces AFTER the start vertex */
  int32_t accumulate;        /* 0: sums start at 0; 1: sum / sumsq are continued in place */
  uint64_t seed;
  double background[3];
  int32_t light_sampling;    /* RtxIntegratorOptions' meaning; f32 scene with 1: RTX_EUNSUPPORTED */
  int32_t sh_order;          /* 0: plain sums [n][3]; 1 | 2 (probe form only): SH sums [n][4][3] | [n][9][3] */
  uint64_t sample_buffer_bytes; /* RtxConfig's meaning: 0 = the default budget */
  int32_t reserved[2];       /* must be 0 */
} RtxGatherPoints;
/* Zeroes *g, then samples = 1, max_depth = 50, seed = 1, background = (0.7, 0.8, 1). */
void rtx_gather_points_defaults(RtxGatherPoints* g);
/* Host pointers, blocking; staged in slices of RTX_TRACE_HOST_SLICE points (56 B in, 48 B of sums a point and coefficient).
 * sum is required, sumsq and stats are optional.  stats->trace_kernel is RTX_KERNEL_RAYS (the gather kernel has k_trace_rays'
 * scheduling), stats->samples = n * samples. */
rtx_status rtx_scene_gather(const rtx_scene* s, const RtxGatherPoints* points, double* sum, double* sumsq, RtxRenderStats* stats);
/* Device pointers, asynchronous on hip_stream: returns after the launches unless stats is not NULL, which synchronises.  A
 * batch of more than 2^30 points goes out as several launches. */
rtx_status rtx_scene_gather_device(const rtx_scene* s, const RtxGatherPoints* points, double* d_sum, double* d_sumsq,
                                   void* hip_stream, RtxRenderStats* stats);
/* Host only, no device call: dir [n][samples][3] = the start directions `dir` above of samples [first_sample, first_sample +
 * samples) of points [first_point, first_point + n), computed by the core function the kernels run, in f64 arithmetic
 * (f32 = 0) or in float arithmetic, widened (f32 = 1: what an f32 scene draws).  Of the struct only n, normal, first_point,
 * first_sample, samples and seed are read.  For callers who project onto a basis of their own.  RTX_EINVAL: a NULL
 * struct or dir, n < 0, samples < 1, a sample range past 2^32, f32 other than 0 / 1. */
rtx_status rtx_gather_directions(const RtxGatherPoints* points, int32_t f32, double* dir);

/* ---- nearest-point queries: the closest surface of a resident scene per point ------------------------------------------- */
/* An extension: how far is point r from the scene, and where is the closest surface -- clearance and collision tests against
 * the objects the update calls move, distance-field bakes, snapping gather points onto a surface, proximity falloff.  Not a
 * ray: the walk prunes by a box's distance to the point against a bound that shrinks as candidates are found
 * (core/nearest.hpp: world_nearest, which states the order of every operation below once, for the kernel and the CPU alike).
 *
 * CANDIDATES of point r (p, time, r_max) are all primitives of the world list: the primitive of a PRIM slot, every ref of a
 * GROUP, every ref of a BVH, the same under an XFORM chain, the members of an instance tree (the plain slots they are).  A
 * ConstantMedium slot contributes its boundary's primitives only when media = 1, reported with the phase material
 * (FlatEntry::b); with media = 0 the slot is skipped.
 *
 * prim_nearest gives, per candidate, a point q on it.  All arithmetic is in rt::real with + - * /, sqrt, fabs, fmin, fmax only:
 *   Sphere / MovingSphere  centre c = (cx, cy, cz) or moving_sphere_center(s, time); v = p - c; len = sqrt(dot(v, v));
 *                          q = c + v * (fabs(radius) / len); when len == 0, q = c + (fabs(radius), 0, 0).
 *   Rectangle              the two in-plane coordinates of p clamped: fmin(fmax(p_a, a0), a1), fmin(fmax(p_b, b0), b1); the
 *                          third is k.  A rectangle with a0 > a1 or b0 > b1 is not a candidate (no ray can hit it either).
 *   Triangle               the closest point by barycentric region, tested in this order, with ab = v1 - v0, ac = v2 - v0,
 *                          ap = p - v0, d1 = dot(ab, ap), d2 = dot(ac, ap); bp = p - v1, d3 = dot(ab, bp), d4 = dot(ac, bp);
 *                          cp = p - v2, d5 = dot(ab, cp), d6 = dot(ac, cp):
 *                            vertex v0   d1 <= 0 and d2 <= 0                                   q = v0
 *                            vertex v1   d3 >= 0 and d4 <= d3                                  q = v1
 *                            edge v0v1   vc = d1 d4 - d3 d2 <= 0, d1 >= 0, d3 <= 0             q = v0 + ab * (d1 / (d1 - d3))
 *                            vertex v2   d6 >= 0 and d5 <= d6                                  q = v2
 *                            edge v0v2   vb = d5 d2 - d1 d6 <= 0, d2 >= 0, d6 <= 0             q = v0 + ac * (d2 / (d2 - d6))
 *                            edge v1v2   va = d3 d6 - d5 d4 <= 0, d4 - d3 >= 0, d5 - d6 >= 0   q = v1 + (v2 - v1) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))
 *                            face        denom = 1 / (va + vb + vc)                            q = (v0 + ab * (vb denom)) + ac * (vc denom)
 *                          then every coordinate of q is clamped into [min, max] of the three vertices' (a no-op unless the
 *                          region tests of a sliver cancelled).  A triangle whose stored normal is NaN has zero area and is
 *                          not a candidate.
 *   under an XFORM chain   p goes in through the ops outermost first, with xform_ray's origin arithmetic; q comes back out
 *                          innermost first, with xform_record's p arithmetic.
 * THE KEY is d2 = dot(p_local - q_local, p_local - q_local) in the frame where the primitive lives, the same for every kind.  A
 * candidate replaces the best so far when d2 < best_d2, or when d2 == best_d2 and its (slot, order) is lexicographically
 * smaller; order is the ref's position in its entry's ref list (the order of Closest), 0 for a PRIM entry.  The search starts
 * from best_d2 = r_max * r_max with nothing found: d2 == r_max^2 is found, a NaN d2 never wins (a MovingSphere with
 * time0 == time1 is never found), a NaN r_max finds nothing.  The answer is therefore a function of the flat scene's arrays
 * alone: not of visiting order or of how a batch is split, and d not of leaf size or builder either.  The builder does order
 * a BVH's ref list (and stores a mesh's triangles in that order), so among candidates that tie EXACTLY inside one BVH -- the
 * triangles sharing the mesh vertex or edge that p is nearest to -- the one named by ids, and the arithmetic its q went
 * through, are those of the first in that build's list.
 *
 * OUTPUTS, any of which may be NULL (all NULL: a timing run):
 *   d   [n]     sqrt(best_d2), +inf when nothing is found
 *   q   [n][3]  the point in the world frame, 0 when nothing is found
 *   ids [n][4]  int32 {material, top-level slot, PrimType (0 sphere, 1 moving sphere, 2 rectangle, 3 triangle), index in that
 *               type's array -- the id rtx_flat_sphere_ids / _triangle_ids / _rect_ids / _moving_sphere_ids hand out},
 *               all -1 when nothing is found
 * An f32 scene narrows p, time and r_max with the cast's conversions and widens what it writes.  Results are deterministic and
 * equal the CPU core's bit for bit in both precisions.  Under a RotateY, |p - q| equals d only to rounding: the stored sin / cos
 * are not exactly a rotation, and d is taken in the member's frame.
 *
 * NOT SUPPORTED: scenes with GravitySpheres return RTX_EUNSUPPORTED -- their BVH boxes are the union of the boxes at the two
 * ends of the interval, not of the trajectory between, so no distance bound follows from them; k > 1 neighbours; signed
 * distance.
 *
 * RTX_EINVAL before any device call, the message naming the field: a NULL scene, batch or result struct; n < 0; n > 0 with NULL
 * points; a NaN or negative r_max_all; media other than 0 / 1; a non-zero reserved word.  RTX_EUNSUPPORTED for a BVH too deep
 * for the LDS traversal stack; both are refused before the host entry stages anything.  n = 0 is RTX_OK.  A NaN coordinate
 * of p is defined -- every d2 is NaN, nothing is found -- but costly: no box bounds a NaN, so that point visits every
 * primitive of the scene.  The query does not use the render workspace and may run beside a render, as
 * the cast does. */
typedef struct RtxPointBatch {
  int64_t n;
  const double* points;  /* [n][3] */
  const double* time;    /* [n] or NULL: 0 */
  const double* r_max;   /* [n] or NULL: r_max_all */
  double r_max_all;      /* defaults: +inf */
  int32_t media;         /* 0 / 1 */
  int32_t reserved;      /* must be 0 */
} RtxPointBatch;
typedef struct RtxNearest {
  double* d;     /* [n] */
  double* q;     /* [n][3] */
  int32_t* ids;  /* [n][4] */
} RtxNearest;
/* Zeroes *b, then r_max_all = +inf. */
void rtx_point_batch_defaults(RtxPointBatch* b);
/* Host pointers, blocking; staged in slices of RTX_CAST_HOST_SLICE points (40 B in, 48 B out a point). */
rtx_status rtx_scene_nearest(const rtx_scene* s, const RtxPointBatch* points, const RtxNearest* out);
/* Device pointers, asynchronous on hip_stream: returns after the launch.  ids must be 16-byte aligned and every other column
 * 8-byte aligned: RTX_EINVAL naming the pointer otherwise, before any device call.  A batch of more than 2^30 points goes out
 * as several launches. */
rtx_status rtx_scene_nearest_device(const rtx_scene* s, const RtxPointBatch* points, const RtxNearest* out, void* hip_stream);

/* ---- moving objects: new parameters for the Translate / RotateY chains of top-level slots --------------------------------
 * Setting the ops of top-level slots on a flattened or a resident scene gives the scene that rtx_flatten (and rtx_scene_upload)
 * build from scratch with those rtx_translate offsets and rtx_rotate_y angles: every entry point answers bit for bit as it
 * does on that scene.  Three device arrays depend on a transform -- the slot's entry, its record in k_trace_world's slot table
 * and the boxes of the instance tree it is a member of -- and only those are touched: no primitive, texture or BVH is re-sent.
 *   * The chain's SHAPE is fixed: a slot's number of ops and the kind of each stay what the flattener emitted (ask
 *     rtx_flat_slot_chain); only the parameters change.  An update names ALL ops of its slot.
 *   * The instance tree's TOPOLOGY is kept: its boxes are refitted bottom-up.  A refitted tree culls less well than a rebuilt
 *     one once members have moved far: rtx_*_instance_tree_cost reports how well a tree culls as it stands, and
 *     rtx_*_rebuild_instance_trees (below) gives it a new topology for the current pose.  RtxFlatInfo::sah_cost covers the
 *     members' own BVHs only and does not depend on a pose.
 *   * A slot can be moved when its entry is a Translate / RotateY chain (rtx_flat_top_level_kind 3) or a ConstantMedium whose
 *     boundary is such a chain (kind 4), inside or outside an instance tree.
 * RTX_EINVAL, the message naming the field, nothing enqueued and the scene unchanged: a NULL argument, n < 0, a slot out of
 * range, a slot without a chain, a wrong n_ops, a wrong op kind, a slot named twice, a value that is not finite, a member whose
 * new bounding box is not finite.  n = 0 is RTX_OK and nothing is launched. */
#define RTX_XFORM_TRANSLATE 0
#define RTX_XFORM_ROTATE_Y 1
typedef struct RtxSlotOps {
  int32_t slot;   /* index in the world list */
  int32_t n_ops;  /* must equal the slot's chain length */
  struct {
    int32_t op;   /* RTX_XFORM_TRANSLATE / RTX_XFORM_ROTATE_Y: must equal the kind the chain has at this place */
    int32_t pad;
    double v[3];  /* translate: the offset; rotate_y: v[0] = the angle in DEGREES (v[1], v[2] ignored), turned into sin / cos on
                     the host exactly as rtx_rotate_y does, which is what makes the result bit-equal to a fresh build */
  } ops[4];       /* outermost first, as the wrappers are nested: Translate(RotateY(x)) is {translate, rotate_y} */
} RtxSlotOps;
/* Number of ops of the slot's chain, their kinds into kinds[0..n); 0 for a slot with no chain, -1 when the slot is out of range
 * (or f or kinds is NULL). */
int32_t rtx_flat_slot_chain(const rtx_flat* f, int32_t slot, int32_t kinds[4]);
/* Instance tree k (0 <= k < RtxInstanceInfo::n_trees, in the order of their first slots): its members are the n_slots
 * consecutive slots from first_slot, in list order with nested lists spliced in. */
typedef struct RtxInstanceTree {
  int32_t first_slot, n_slots, n_nodes, depth;
} RtxInstanceTree;
rtx_status rtx_flat_instance_tree(const rtx_flat* f, int32_t k, RtxInstanceTree* out);
/* Host only.  Edits the flat scene in place (entries, and nodes / nodes32 / the static boxes of the time-aware copy of every
 * tree that holds an updated member); it can then be uploaded, or handed to rtx_multi_create, without flattening again. */
rtx_status rtx_flat_set_transforms(rtx_flat* f, const RtxSlotOps* updates, int64_t n);
/* The same on a resident scene of either precision (an f32 scene takes the ops through the converter's (float) cast and its
 * boxes rounded outward, as rtx_scene_upload_f32 does).  `updates` is a HOST array, free for reuse on return; the work -- one
 * small copy, k_set_slot_ops, and k_refit_instance_tree once per tree that holds an updated member -- is asynchronous on
 * hip_stream.  Ordering against renders and casts on OTHER streams is the caller's business; two updates of one scene may not
 * run concurrently (issue them on one stream, or synchronise).  A progressive handle made before an update holds samples of
 * the old pose, and the features it has already computed (rtx_progressive_features / _denoise keep those
 * of the last feature_spp asked for, and compute them again only when another count is asked for) are those of the old pose
 * too: make a new one.  rtx_multi_* scenes are not covered: set the flat scene and create the handle again. */
rtx_status rtx_scene_set_transforms(rtx_scene* s, const RtxSlotOps* updates, int64_t n, void* hip_stream);
/* Test hook: copies one resident array of the scene back to the host, after everything enqueued on the device.  which:
 * 0 entries, 1 nodes, 2 nodes32, 3 the time-aware boxes, 4 k_trace_world's slot table, 7 the 4-wide culling tree (128 bytes per
 * node, indexed like nodes; 0 bytes when the scene walks its binary tree), 8 the stack levels its walks are launched with (one
 * int32, 0 without a wide tree), 9 the scene's max_stack as its binary walks are now launched with (one int32; a rebuild of
 * an instance tree changes it), 10 triangles, 11 top_box32 (6 floats per slot), 13 the static spheres (FlatSphere, 40 bytes
 * each in an f64 scene), 14 the light table of next-event estimation (FlatLight, 40 bytes each; 0 bytes without sampled
 * lights), 15 materials and 16 textures (FlatMaterial / FlatTexture: 48 bytes each in an f64 scene, 32 in an f32 scene),
 * 17 the MovingSpheres (FlatMovingSphere, 80 bytes each in an f64 scene, 44 in an f32 scene).
 * bytes must be the array's size (elements as the scene's precision lays them out); RTX_EINVAL
 * naming the size otherwise. */
rtx_status rtx_device_scene_array(const rtx_scene* s, int32_t which, void* out, size_t bytes);
/* The same for the host arrays of a flat scene, which adds 5: top_level, 6: member_local_box (6 doubles per member of an
 * instance tree, the box before the ops), 12: triangle_id (one int32 per flat triangle).  14 is the light table an upload
 * of the flat scene as it stands would build; 15 and 16 are the host's materials and textures (48 bytes each), 17 its MovingSpheres
 * (80 bytes each). */
rtx_status rtx_flat_array(const rtx_flat* f, int32_t which, void* out, size_t bytes);

/* ---- instance trees: the quality of a tree as it stands, and a rebuild for the current pose ---------------------------------
 * Cost of instance tree k (0 <= k < RtxInstanceInfo::n_trees): the sum, over the tree's nodes in ascending node index, of the
 * surface areas 2 (dx dy + dy dz + dz dx) of the node's two child boxes, divided by the area of the union of the root's two
 * child boxes -- the expected number of child boxes a random ray through the tree's box meets, up to a constant.  Areas are f64
 * from the planes as the scene stores them (an f32 scene's planes are widened first).  The resident version computes the
 * per-node terms in a kernel and adds them on the host in the same order, so it equals the flat version bit for bit on equal
 * planes; it BLOCKS: it waits for everything enqueued on the device, like rtx_device_scene_array.  RTX_EINVAL for a NULL
 * argument or k out of range. */
rtx_status rtx_flat_instance_tree_cost(const rtx_flat* f, int32_t k, double* cost);
rtx_status rtx_scene_instance_tree_cost(const rtx_scene* s, int32_t k, double* cost);
/* Rebuilding instance tree k replaces its TOPOLOGY with one built from the members' world boxes at their current ops.  The
 * members stay the same n_slots consecutive slots and the tree keeps its piece of n_slots - 1 nodes: no array grows or moves.
 * Every leaf holds one slot, every child box is the exact union of the member boxes under it, nodes32 is the narrowing of nodes,
 * the time-aware copy (where present) the static one a refit writes, and every entry point answers bit for bit as on a fresh
 * upload of that pose (a frame does not depend on a tree's topology).  rtx_*_set_transforms keeps working on a rebuilt tree.
 * The scene's max_stack is the members' part + 1 + the deepest instance tree as the trees now stand: it can rise or fall.
 *   RTX_REBUILD_MORTON  what the device does, restated on the host: 63-bit Morton codes of the box centroids, a stable sort,
 *                       Karras' radix tree.  A flat scene rebuilt this way equals the resident arrays of a scene rebuilt on
 *                       the device, byte for byte, in both precisions.
 *   RTX_REBUILD_SAH     the flattener's own builder on the current boxes: the flat scene then equals a fresh rtx_flatten of
 *                       that pose byte for byte in every array, and so does rtx_flat_info (build times aside).
 * trees: n tree indices, or NULL for every tree (n is then ignored unless negative).  RTX_EINVAL, the message naming the
 * field, nothing enqueued and the scene unchanged: a NULL scene, n < 0, a tree index out of range or named twice, an unknown
 * builder, a non-zero reserved word of *out, a scene on another device.  RTX_OK with nothing launched: a scene without instance
 * trees when trees is NULL, and n = 0 with a list.  RTX_EUNSUPPORTED, the scene unchanged: the Morton trees would need a walk
 * stack of more than 64 levels (64 KB of LDS), which no launcher accepts. */
#define RTX_REBUILD_MORTON 0
#define RTX_REBUILD_SAH 1
typedef struct RtxRebuildStats {
  int32_t trees_rebuilt;     /* trees this call rebuilt */
  int32_t max_depth;         /* the deepest of them, in nodes */
  int32_t max_stack_before;  /* the scene's max_stack before and after the call */
  int32_t max_stack_after;
  int32_t reserved[4];       /* must be 0 on entry */
} RtxRebuildStats;
/* Host only.  Edits the flat scene in place. */
rtx_status rtx_flat_rebuild_instance_trees(rtx_flat* f, const int32_t* trees, int32_t n, int32_t builder);
/* A resident scene of either precision, with the Morton builder on the device (k_member_boxes, k_member_morton, a radix sort,
 * k_rebuild_radix, k_rebuild_emit per tree, into scratch memory of the scene; then device-to-device copies into the tree's
 * piece).  The kernels run on hip_stream.  Unlike rtx_scene_set_transforms this call BLOCKS: it waits on hip_stream once, for
 * the read-back of the new depths (4 bytes per tree, and the new parent tables with them), because the stack budget of every
 * later launch depends on them and a tree that is too deep must be refused before it is committed.  out may be NULL.
 * Concurrency as for rtx_scene_set_transforms: one update or rebuild of a scene at a time, ordering against work on other
 * streams is the caller's, progressive handles made earlier hold the old pose's samples.  rtx_multi_* scenes are not covered:
 * rebuild the flat scene and create the handle again. */
rtx_status rtx_scene_rebuild_instance_trees(rtx_scene* s, const int32_t* trees, int32_t n, void* hip_stream, RtxRebuildStats* out);

/* ---- deforming meshes: new vertices for triangles of a flat scene or of a resident f64 scene (an extension) -----------------
 * The flattener stores a BVH's triangles in leaf order and gives a shared triangle private copies, so a flat triangle is not
 * named by position but by its ID: the ordinal of its first emission by the flattener, 0, 1, 2, ... in the order the world is
 * walked.  A triangle handle listed twice has one id; a private copy carries the id of its original.
 *
 * rtx_flat_triangle_ids: the ids of the triangles below `object` (a triangle, a list such as rtx_triangle_mesh returns, a
 * BvhNode, a wrapper or medium around those), in list order, a mesh's faces in face order.  Writes min(count, cap) ids,
 * returns count; -1 (and rtx_last_error) for a NULL argument, a bad handle or an object this flat scene did not flatten. */
int64_t rtx_flat_triangle_ids(const rtx_flat* f, const rtx_builder* b, rtx_handle object, int32_t* ids, int64_t cap);
/* vertices: n x 9 doubles, v0 v1 v2 of triangle ids[i].  ids: a HOST array in all three entries, free for reuse on return.
 *
 * Meaning: the scene then answers every entry point -- rtx_render* through every walker, light sampling, progressive handles
 * made afterwards and their feature pass, rtx_scene_cast_rays*, rtx_scene_trace_rays* -- bit for bit as the scene built from
 * scratch with those vertices.  One class of ray is exempt, and it is open for a fresh build too: an exact tie between two
 * primitives of different centroids inside one BVH goes by leaf order ("Not covered"), and a fresh build
 * may order leaves differently.
 *
 * What is written, and nothing else: v0 v1 v2 and normal = unit(cross(v1 - v0, v2 - v0)) of every flat copy of each id (mat is
 * untouched; a zero-area triangle gets the NaN normal a fresh build gives it); the boxes of every BVH that holds an updated
 * triangle, refitted whole and bottom-up in nodes, nodes32 and the static copy of the time-aware boxes (child codes, split axes
 * and pads stay: the TOPOLOGY is kept, where a fresh build might choose another -- culling only); on a resident scene with a
 * 4-wide tree the planes of its slots (which nodes the collapse opened is kept, so the stack levels and every launch plan
 * stand); member_local_box and the instance tree above a touched member; top_box32 and the slot record's box of a plain
 * top-level triangle.  RtxFlatInfo::sah_cost is not updated.
 *
 * RTX_EINVAL, the message naming the field, nothing enqueued and the scene unchanged: a NULL argument, n < 0, an id out of
 * range or named twice; host entries: a vertex that is not finite; device entry: a pointer that is not 8-byte aligned.  n = 0
 * is RTX_OK with nothing launched.  RTX_EUNSUPPORTED, the scene unchanged, checked before anything is enqueued: a touched BVH
 * that holds a MovingSphere or GravitySphere (its time-aware slopes would have to be derived again), and a resident f32 scene,
 * which does not hold the f64 vertices of the untouched triangles in touched leaves: update the flat scene with
 * rtx_flat_set_triangles and upload it again with rtx_scene_upload_f32. */
rtx_status rtx_flat_set_triangles(rtx_flat* f, const int32_t* ids, int64_t n, const double* vertices);
/* A resident f64 scene; vertices is a HOST array, staged with one copy.  Asynchronous on hip_stream, as
 * rtx_scene_set_transforms: k_set_prims, then per touched BVH k_refit_bvh (and k_refit_wide), k_member_local_boxes and
 * k_refit_instance_tree per touched instance tree, k_slot_boxes.  One update of a scene at a time; ordering against
 * work on other streams is the caller's; progressive handles made earlier hold the old shape.  rtx_multi_* scenes are not
 * covered: update the flat scene and create the handle again.
 * After an update (through either resident entry) that touched a member of an instance tree, the FIRST
 * rtx_scene_set_transforms that follows waits for the device once and reads the members' new local boxes back (48 bytes a
 * member) before it checks the new pose against them; that one call is not asynchronous.  Later ones are again.
 * The resident entries of both kinds check in one order: what needs no scene first (a NULL argument, n < 0, the alignment of a
 * device pointer, n = 0) -- the handle is not read before these have passed, so an argument fault on an f32 scene is
 * RTX_EINVAL and n = 0 on one is RTX_OK --, then the f32 refusal, the ids, the finiteness of host values. */
rtx_status rtx_scene_set_triangles(rtx_scene* s, const int32_t* ids, int64_t n, const double* vertices, void* hip_stream);
/* d_vertices: a DEVICE pointer (8-byte aligned), e.g. the output of the caller's own skinning kernel on hip_stream; it is read
 * by work enqueued on hip_stream and must stay valid until that work is done.  Finiteness cannot be checked without a
 * read-back: a vertex that is not finite gives that triangle and the boxes above it unspecified culling.  No index is derived
 * from a vertex, so nothing can leave an allocation. */
rtx_status rtx_scene_set_triangles_device(rtx_scene* s, const int32_t* ids, int64_t n, const double* d_vertices, void* hip_stream);

/* ---- moving spheres: a new centre and radius for static spheres of a flat scene or of a resident f64 scene (an extension) ---
 * The flattener emits a static sphere once per handle and neither permutes nor copies it, so a sphere's ID is its index in the
 * flat scene's sphere array.  A sphere handle listed twice, or listed in the world list and in a BvhNode, has one id: both
 * places move.  Moving and gravity spheres have no id.
 *
 * rtx_flat_sphere_ids: the ids of the static spheres below `object` (a sphere, a list, a BvhNode, an instance tree, a wrapper
 * or medium around those), in list order; moving and gravity spheres are skipped.  Writes min(count, cap) ids, returns count;
 * -1 (and rtx_last_error) for a NULL argument, a bad handle or an object this flat scene did not flatten. */
int64_t rtx_flat_sphere_ids(const rtx_flat* f, const rtx_builder* b, rtx_handle object, int32_t* ids, int64_t cap);
/* spheres: n x 4 doubles, cx cy cz radius of sphere ids[i].  ids: a HOST array in all three entries, free for reuse on return.
 *
 * Meaning: the scene then answers every entry point -- rtx_render* through every walker (k_trace_lds included: it copies the
 * culling boxes and the sphere records into LDS at every launch), light sampling, progressive handles made afterwards and
 * their feature pass, rtx_scene_cast_rays*, rtx_scene_trace_rays* -- bit for bit as the scene built from scratch with those
 * spheres.  Exempt, as for rtx_*_set_triangles: an exact tie inside one BVH goes by leaf order, and a box plane that is
 * exactly zero takes its sign from the order of the unions.
 *
 * What is written, and nothing else: cx cy cz radius of the flat sphere (mat is untouched); the boxes of every BVH that holds
 * an updated sphere, refitted whole and bottom-up in nodes, nodes32 and the static copy of the time-aware boxes (the TOPOLOGY
 * is kept); on a resident scene with a 4-wide tree the planes of its slots (the stack levels and every launch plan stand);
 * member_local_box and the instance tree above a touched member; top_box32 and the slot record's box of a plain top-level
 * sphere, and the slot record's box of a medium whose boundary is the sphere (with the record's flags that are derived from
 * those boxes and from the sphere's bytes); on a resident scene, when an updated sphere is a sampled light, the light table:
 * that light's area, and every light's cdf and pmf (a light's pick weight is its area times the emission at its CENTRE, so a
 * move alone can change every probability).  RtxFlatInfo::sah_cost is not updated.
 *
 * RTX_EINVAL, the message naming the field, nothing enqueued and the scene unchanged: a NULL argument, n < 0, an id out of
 * range or named twice; host entries: a value that is not finite (the radius may be negative -- the hollow glass ball -- or
 * zero: rtx_sphere applies no rule to it either); device entry: a pointer that is not 8-byte aligned.  n = 0 is RTX_OK with
 * nothing launched.  RTX_EUNSUPPORTED, the scene unchanged, checked before anything is enqueued: a touched BVH that holds a
 * MovingSphere or GravitySphere (its time-aware slopes would have to be derived again), and a resident f32 scene: update the
 * flat scene with rtx_flat_set_spheres and upload it again with rtx_scene_upload_f32. */
rtx_status rtx_flat_set_spheres(rtx_flat* f, const int32_t* ids, int64_t n, const double* spheres);
/* A resident f64 scene; spheres is a HOST array, staged with one copy.  Asynchronous on hip_stream, as
 * rtx_scene_set_triangles: k_set_prims, then per touched BVH k_refit_bvh (and k_refit_wide), k_member_local_boxes and
 * k_refit_instance_tree per touched instance tree, k_slot_boxes, k_refresh_lights.  One update of a scene at a time;
 * ordering against work on other streams is the caller's; progressive handles made earlier hold the old spheres.  rtx_multi_*
 * scenes are not covered: update the flat scene and create the handle again.  The read-back by the FIRST
 * rtx_scene_set_transforms after an update that touched a member of an instance tree applies as for rtx_scene_set_triangles. */
rtx_status rtx_scene_set_spheres(rtx_scene* s, const int32_t* ids, int64_t n, const double* spheres, void* hip_stream);
/* d_spheres: a DEVICE pointer (8-byte aligned), e.g. the output of the caller's own animation kernel on hip_stream; it is read
 * by work enqueued on hip_stream and must stay valid until that work is done.  Finiteness cannot be checked without a
 * read-back: a value that is not finite gives that sphere and the boxes above it unspecified culling.  No index is derived
 * from a value, so nothing can leave an allocation. */
rtx_status rtx_scene_set_spheres_device(rtx_scene* s, const int32_t* ids, int64_t n, const double* d_spheres, void* hip_stream);

/* ---- motion blur on a resident scene: new end centres and a radius for MovingSpheres (an extension) -------------------------
 * A MovingSphere's c0 / c1 are its centre at time0 / time1 -- with the camera's shutter, the reference's motion blur.  An
 * animation with blur gives every mover a new (c0, c1) per frame.  The flattener emits a MovingSphere once per handle, so a
 * mover's ID is its index in the flat scene's moving-sphere array (rtx_flat_array 17: FlatMovingSphere, 80 bytes each).
 *
 * rtx_flat_moving_sphere_ids: the twin of rtx_flat_sphere_ids for MovingSpheres; every other kind is skipped. */
int64_t rtx_flat_moving_sphere_ids(const rtx_flat* f, const rtx_builder* b, rtx_handle object, int32_t* ids, int64_t cap);
/* movers: n x 7 doubles, c0 xyz, c1 xyz, radius of mover ids[i]; time0, time1 and the material stay.  ids: a HOST array in all
 * three entries, free for reuse on return.
 *
 * Meaning, as for rtx_*_set_spheres: the scene then answers every entry point bit for bit as the scene built from scratch with
 * those values, with the same exemptions (a tie inside one BVH, the sign of a zero plane, a fresh build's other topology).
 *
 * What is written, and nothing else: c0, c1, radius of the record; of every BVH that holds an updated mover, refitted whole and
 * bottom-up with its TOPOLOGY kept, the boxes over the BVH's own interval in nodes and nodes32 (and the 4-wide tree's planes on
 * a resident scene that has one) and the time-aware boxes: for a BVH with time0 < time1 and no GravitySphere the planes and
 * slopes derived from the unions at its two ends, else the static copy without slopes; on a resident scene the box, the
 * "box holds for the mover's own interval" flag and its two times in the slot record of a plain mover in the world list.
 *
 * The one value-dependent fact of a launch plan follows: k_trace_lds's time-aware variant is instantiated by the axes along
 * which the time-aware boxes have slopes (RTX_LDS_VARIANT_ONE_AXIS) and sized by them.  The refit records those axes on the
 * device; on a scene with such a plan the FIRST render, cast or query that launches k_trace_lds after an update waits ON THE
 * HOST, once, for the update to finish and plans the variant again, as an upload of the new values would (rtx_render_device
 * is asynchronous but for this wait).
 *
 * RTX_EINVAL, the message naming the field, nothing enqueued and the scene unchanged: a NULL argument, n < 0, an id out of
 * range or named twice; host entries: a value that is not finite (the radius may be negative or zero, as for rtx_moving_sphere);
 * device entry: a pointer that is not 8-byte aligned.  n = 0 is RTX_OK with nothing launched.  RTX_EUNSUPPORTED, the scene
 * unchanged, checked before anything is enqueued: a resident f32 scene (update the flat scene and upload it again with
 * rtx_scene_upload_f32; this is checked before the ids, which need the tables only an f64 scene keeps), and a touched BVH
 * that also holds a GravitySphere: that centre is not linear in time and its box needs its height table.
 * rtx_*_set_spheres and rtx_*_set_triangles still refuse a BVH that holds a mover. */
rtx_status rtx_flat_set_moving_spheres(rtx_flat* f, const int32_t* ids, int64_t n, const double* movers);
/* A resident f64 scene; movers is a HOST array, staged with one copy.  Asynchronous on hip_stream, as rtx_scene_set_spheres:
 * k_set_prims, then per touched BVH k_refit_timed_bvh (and k_refit_wide), k_slot_boxes, and where a k_trace_lds plan hangs on
 * the slopes one 4-byte copy to the host behind them.  One update of a scene at a time; ordering against work on other streams
 * is the caller's; progressive handles made earlier hold the old values.  rtx_multi_* scenes are not covered. */
rtx_status rtx_scene_set_moving_spheres(rtx_scene* s, const int32_t* ids, int64_t n, const double* movers, void* hip_stream);
/* d_movers: a DEVICE pointer (8-byte aligned), e.g. the poses at shutter open and close computed by the caller's own kernel on
 * hip_stream; it is read by work enqueued on hip_stream and must stay valid until that work is done.  Finiteness cannot be
 * checked without a read-back: a value that is not finite gives that mover and the boxes above it unspecified culling.  No
 * index is derived from a value, so nothing can leave an allocation. */
rtx_status rtx_scene_set_moving_spheres_device(rtx_scene* s, const int32_t* ids, int64_t n, const double* d_movers, void* hip_stream);

/* ---- moving walls, boxes and area lights: new extents for rectangles of a flat scene or of a resident f64 scene (an extension)
 * Rectangles are what walls, the six faces of a RectPrism, the boundary box of a medium and rectangular area lights are made
 * of.  The flattener neither permutes nor copies a rectangle, so a rectangle's ID is its index in the flat scene's rectangle
 * array (rtx_flat_array 19: FlatRect, 48 bytes each -- a0 a1 b0 b1 k as doubles, then axis and material as int32).
 *
 * rtx_flat_rect_ids: the ids of every rectangle the flattener emitted from the handles below `object` (a rectangle, a
 * RectPrism, a list, a BvhNode, an instance tree, a Translate, RotateY or ConstantMedium around those), handle by handle in list
 * order, a handle's rectangles in emission order.  A rectangle handle has one id however often it is listed.  A RectPrism has
 * six per emission -- front, back, top, bottom, right, left: the order of RectPrism::new -- and is emitted anew from every place
 * it is reached from, so one prism handle under two Translates has twelve, and they are returned together, from the world and
 * from the prism's own handle alike.  No id is returned twice.  Writes min(count, cap) ids, returns count; -1 (and
 * rtx_last_error) for a NULL argument, a bad handle or an object this flat scene did not flatten. */
int64_t rtx_flat_rect_ids(const rtx_flat* f, const rtx_builder* b, rtx_handle object, int32_t* ids, int64_t cap);
/* rects: n x 5 doubles a0 a1 b0 b1 k of rectangle ids[i] -- the constructor's (x0, x1, y0, y1, k) in FlatRect's own order; the
 * axis and the material stay.  ids: a HOST array in all three entries, free for reuse on return.
 *
 * Meaning, as for rtx_*_set_spheres: the scene then answers every entry point bit for bit as the scene built from scratch with
 * those values, with the same exemptions (a tie inside one BVH, the sign of a zero plane, a fresh build's other topology).
 *
 * What is written, and nothing else: a0 a1 b0 b1 k of the record; the boxes of every BVH that holds an updated rectangle,
 * refitted whole and bottom-up with the TOPOLOGY kept (nodes, nodes32, the static copy of the time-aware boxes, the 4-wide
 * tree's planes on a resident scene that has one); member_local_box and the instance tree above a touched member -- a
 * rectangle, a prism or a BVH under a chain, also as the boundary of a medium; top_box32 and the slot record's box of a plain
 * top-level rectangle; on a resident scene, when an updated rectangle is a sampled light, the light table: that light's area
 * and every light's cdf and pmf.  On a resident scene k_trace_vote's launch argument holds a copy of up to eight top-level
 * rectangle records: the host entry rewrites the copy before it returns; the device entry, which never sees the values, gives
 * the copy up when it holds a touched rectangle, and launches walk the world list from then on -- the same image, slower by
 * the list walk's dependent loads.
 *
 * RTX_EINVAL, the message naming the field, nothing enqueued and the scene unchanged: a NULL argument, n < 0, an id out of
 * range or named twice; host entries: a value that is not finite (no other rule: an inverted or an empty extent is what the
 * constructor would store); device entry: a pointer that is not 8-byte aligned.  n = 0 is RTX_OK with nothing launched.
 * RTX_EUNSUPPORTED, the scene unchanged, checked before anything is enqueued: a touched BVH that holds a MovingSphere or
 * GravitySphere, and a resident f32 scene: update the flat scene with rtx_flat_set_rects and upload it again with
 * rtx_scene_upload_f32. */
rtx_status rtx_flat_set_rects(rtx_flat* f, const int32_t* ids, int64_t n, const double* rects);
/* A resident f64 scene; rects is a HOST array, staged with one copy.  Asynchronous on hip_stream, as rtx_scene_set_spheres:
 * k_set_prims, then per touched BVH k_refit_bvh (and k_refit_wide), k_member_local_boxes and k_refit_instance_tree per touched
 * instance tree, k_slot_boxes, k_refresh_lights.  One update of a scene at a time; ordering against work on other streams is
 * the caller's; progressive handles made earlier hold the old rectangles.  rtx_multi_* scenes are not covered. */
rtx_status rtx_scene_set_rects(rtx_scene* s, const int32_t* ids, int64_t n, const double* rects, void* hip_stream);
/* d_rects: a DEVICE pointer (8-byte aligned); it is read by work enqueued on hip_stream and must stay valid until that work is
 * done.  Finiteness cannot be checked without a read-back: a value that is not finite gives that rectangle and the boxes above
 * it unspecified culling.  No index is derived from a value, so nothing can leave an allocation. */
rtx_status rtx_scene_set_rects_device(rtx_scene* s, const int32_t* ids, int64_t n, const double* d_rects, void* hip_stream);

/* ---- relighting and look development: new shading parameters -----------------------------------------------------------------
 * Editing colours, a noise scale, a metal, a glass's index or a fog's density of a flattened or a resident scene gives the
 * scene that rtx_flatten (and rtx_scene_upload / rtx_scene_upload_f32) build from scratch when the builder calls are made with
 * the new values: byte for byte in every array a value reaches, and every entry point answers bit for bit as on that scene.
 * No primitive, BVH or image is re-sent.
 *
 * Indices.  A material or texture index is the BUILDER'S HANDLE (rtx_lambertian .. rtx_isotropic, rtx_solid_color .. rtx_image_*:
 * the graph's materials and textures flatten 1:1, in order) and what rtx_scene_cast_rays reports in ids[:, 1].  A medium is named
 * by its top-level slot (rtx_flat_top_level_kind 4); the phase material and colour texture that rtx_constant_medium made inside
 * have no handle of the caller's: walk rtx_flat_medium_info -> rtx_flat_material_info -> tex.
 *
 * What each edit writes, with the builder's own arithmetic (csrc/core/shading_edit.hpp), and nothing else:
 *   RTX_SHADE_SOLID_COLOR     the texture's colour, and the copy of it the flattener keeps in EVERY Lambertian / DiffuseLight /
 *                             Isotropic material that names the texture (kernels for worlds without checker, noise and image
 *                             textures read only that copy).  A checker that has the texture as a child holds no copy.
 *   RTX_SHADE_NOISE_SCALE     the texture's scale; its Perlin tables are kept.
 *   RTX_SHADE_METAL           albedo = r g b, fuzz clamped from above to 1 as rtx_metal does (a negative fuzz passes as it does there).
 *   RTX_SHADE_DIELECTRIC      ir, and the three constants the flattener derives from it (1 / ir, two reflectance terms), in f64.
 *   RTX_SHADE_MEDIUM_DENSITY  -1 / density in the medium's entry and, on a resident scene, in k_trace_world's slot record.
 * An f32 scene takes every value computed in f64 as above through the converter's (float) cast.  On a resident f64 scene that
 * holds a light table, a batch with a texture edit recomputes every light's pick weight, cdf and pmf on the device
 * (k_refresh_lights: the recomputation rtx_scene_set_spheres runs, by the function that built the table; when no light's colour
 * changed it leaves the same bytes).
 *
 * Refused with RTX_EINVAL, the scene unchanged, nothing enqueued, the message naming the edit's position and field, checked in
 * this order: a NULL scene, NULL edits with n > 0, n < 0; then per edit an unknown `what`, an index out of range, a target of the
 * wrong kind (the message names the spelling that works), a value that is not finite (no other rule: the builder applies none,
 * density 0 gives -inf as rtx_constant_medium does), a non-zero unused v; then one target -- (texture | material | slot, index)
 * -- named twice in the call.  Last, a resident scene on another device than the current one.  n = 0 is RTX_OK, nothing launched.
 *
 * Outside an edit: kinds do not change; which texture a material names does not change; a checker's children do not change;
 * Perlin tables do not change; image texels are not edited; RtxFlatInfo is unaffected.  rtx_multi_* scenes are not covered:
 * edit the flat scene and create the handle again. */
#define RTX_SHADE_SOLID_COLOR    0  /* index: texture (RTX_TEX_SOLID);       v = r g b      : rtx_solid_color's rgb            */
#define RTX_SHADE_NOISE_SCALE    1  /* index: texture (RTX_TEX_NOISE);       v[0] = scale   : rtx_noise's scale, tables kept   */
#define RTX_SHADE_METAL          2  /* index: material (RTX_MAT_METAL);      v = r g b fuzz : rtx_metal's arguments            */
#define RTX_SHADE_DIELECTRIC     3  /* index: material (RTX_MAT_DIELECTRIC); v[0] = ir      : rtx_dielectric's ir              */
#define RTX_SHADE_MEDIUM_DENSITY 4  /* index: top-level slot of kind 4;      v[0] = density : rtx_constant_medium's density    */
typedef struct RtxShadingEdit {     /* 40 B; unused v must be 0 */
  int32_t what, index;
  double v[4];
} RtxShadingEdit;
/* The material and texture kinds as the flat arrays hold them. */
#define RTX_MAT_LAMBERTIAN    0
#define RTX_MAT_METAL         1
#define RTX_MAT_DIELECTRIC    2
#define RTX_MAT_DIFFUSE_LIGHT 3
#define RTX_MAT_ISOTROPIC     4
#define RTX_TEX_SOLID   0
#define RTX_TEX_CHECKER 1
#define RTX_TEX_NOISE   2
#define RTX_TEX_IMAGE   3
/* Host-only inspectors: from an index to what may be edited.  RTX_EINVAL for a NULL argument, an index out of range, or (medium)
 * a slot that is not a ConstantMedium. */
typedef struct RtxMaterialInfo {    /* 40 B */
  int32_t kind, tex;                /* RTX_MAT_*; the texture a Lambertian / DiffuseLight / Isotropic names, -1 for the others */
  double albedo[3];                 /* Metal: the colour; texture-carrying kinds: the colour of `tex` when that is a SolidColor;
                                       Dielectric: 1 / ir and the two reflectance terms */
  double param;                     /* Metal: fuzz as stored (<= 1); Dielectric: ir */
} RtxMaterialInfo;
typedef struct RtxTextureInfo {     /* 48 B */
  int32_t kind, a, b, pad;          /* RTX_TEX_*; checker: a = even, b = odd; noise: a = its Perlin table; image: a = its image */
  double color[3];                  /* SolidColor */
  double scale;                     /* Noise */
} RtxTextureInfo;
typedef struct RtxMediumInfo {      /* 16 B */
  int32_t material, pad;            /* the phase material (Isotropic) rtx_constant_medium made */
  double neg_inv_density;           /* -1 / density, as stored */
} RtxMediumInfo;
rtx_status rtx_flat_material_info(const rtx_flat* f, int32_t index, RtxMaterialInfo* out);
rtx_status rtx_flat_texture_info(const rtx_flat* f, int32_t index, RtxTextureInfo* out);
rtx_status rtx_flat_medium_info(const rtx_flat* f, int32_t slot, RtxMediumInfo* out);
/* Host only.  Edits the flat scene in place (materials, textures, entries); it can then be uploaded, or handed to
 * rtx_multi_create, without flattening again. */
rtx_status rtx_flat_set_shading(rtx_flat* f, const RtxShadingEdit* edits, int64_t n);
/* The same on a resident scene of either precision.  `edits` is a HOST array, free for reuse on return; the work -- one small
 * copy, k_set_shading with one thread per written record, and k_refresh_lights after a texture edit on an f64 scene with a light
 * table -- is asynchronous on hip_stream.  Ordering against renders and casts on OTHER streams is the caller's business; two
 * updates of one scene may not run concurrently (issue them on one stream, or synchronise).  A progressive handle made before an
 * edit holds samples of the old look, and the features it has already computed are those of the old look too: make a new one. */
rtx_status rtx_scene_set_shading(rtx_scene* s, const RtxShadingEdit* edits, int64_t n, void* hip_stream);

/* ---- the time-sweep renderer: render_scene_with_time(t0, t1, path, world)  world.rs:1249-1330 ------------------------ */
/* One frame of the reference's video experiment on a scene that is ALREADY resident on the GPU (many frames, one
 * upload): 500 x 500, 500 spp, depth 50, background (0.7, 0.8, 1), camera (13,2,3) -> (0,0,0), vfov 20, aspect 1,
 * aperture 0.1, focus 10, shutter [t0, t1) -- all hard-coded there -- written to `path` as P3 PPM.  The reference
 * renders it with its THREADS = 11 row bands (world.rs:18,1284), which leaves rows 495..499 black; row_chunk_compat = 1
 * reproduces that, 0 renders every row.  `overrides` may be NULL; a non-NULL RtxConfig replaces width / spp / depth /
 * seed (its aspect_ratio, background and threads are ignored) so that tests need not trace 125 M samples per frame. */
rtx_status rtx_render_scene_with_time(const rtx_scene* s, double t0, double t1, const char* path, int32_t row_chunk_compat,
                                      const RtxConfig* overrides);

/* ---- image output: Screen::write_to_ppm_file  screen.rs:40-59 ------------------------------ */
/* rgb8 in the row order above (row 0 = bottom); writes "P3\n{w} {h}\n255\n" then one "r g b" line
 * per pixel, top row first.  path NULL or "-" = stdout (Screen::write_to_ppm). */
rtx_status rtx_write_ppm(const char* path, int32_t width, int32_t height, const uint8_t* rgb8);

/* ---- device self-test -------------------------------------------------------------------------- */
/* Evaluates one arithmetic building block of the kernels ON THE GPU for n host-side operands
 * (copied in and out), so tests can prove it is bit-identical to the host's evaluation of the same
 * source.  fn: 0 sin, 1 cos, 2 log, 3 acos, 4 atan2(x,y), 5 tan, 6 sqrt, 7 x/y, 8 x*y+x (must NOT be
 * fused), 9 floor, 10 the sort key of a 4-wide BVH step for entry distance x and t_min y
 * (clamp into [y, 3e38] with NaN -> y).  fn >= 32: the building blocks of the f32 fast mode, evaluated by the f32
 * compilation on (float)x, (float)y, the float result widened: 32 sinf, 33 cosf, 34 logf, 35 acosf, 36 atan2f(x,y), 37 sqrtf,
 * 38 x/y, 39 the sign rt_sin_sign returns, 43 the capped slope 1/x of the f32 culling ray; 40 / 41 / 42 the float forms of
 * gen::<f64>() / gen_range(lo..hi) / gen_range(-1..1) from one raw 64-bit draw given as the BITS of x (41: lo and hi as floats
 * in the low and high word of y).  rtx_device_stream: the first n uniforms of the (seed, pixel, sample) stream. */
rtx_status rtx_device_math(int32_t fn, const double* x, const double* y, int64_t n, double* out);
rtx_status rtx_device_stream(uint64_t seed, uint64_t pixel, uint32_t sample, int32_t n, double* out);
/* The f32 box tests that let every trace kernel skip subtrees (core/cull32.hpp, trace_vote.inc), asked directly.  f32: 0 the
 * f64 compilation's code, 1 the fast mode's.  Item k: box[6k..] = lo xyz, hi xyz in f64, narrowed by the host with the product's
 * outward rounding (lo down, hi up); ray[8k..] = origin xyz, direction xyz, t_min, t_max in f64 (f32 = 1: converted with a
 * (float) cast, so give it float-representable numbers).  The device builds the culling ray as a bounce does (make_ray32:
 * v_rcp_f32, and the slope cap under f32 = 1; t_max through cull_round_up) and returns
 *   ray32[8k..]  ix iy iz, oix oiy oiz, err2, t_min
 *   key[k]       the clamped entry distance a wide step sorts the child by
 *   verdict[k]   bit 0 cull32_may_hit, 1 cull32_may_hit_nf, 2 cull32_may_hit_nf_pos (bit 6 says it was asked: t_min > 0),
 *                3 and 4 the two outputs of cull32_may_hit2 for this box as both children, 5 the wide step's slab_interval_nf;
 *                a set bit = "may hit".  The near / far planes are picked as the kernels pick them (ray32_dir_neg,
 *                wide_sign_pack).
 * n <= 65536.  Blocking. */
rtx_status rtx_device_cull_verdicts(int32_t f32, int64_t n, const double* box, const double* ray, float* ray32, float* key,
                                    uint32_t* verdict);
/* One node step of a walk per item, as a lane of a 256-thread block takes it with its stack in LDS.  kind: 0 walk_node_step32
 * on FlatNode32 records (64 bytes), 1 walk_node_step4 on 4-wide records (128 bytes); bottom: 0 LdsStack, 1 LdsStackB (slot 0
 * holds "walk done" and a walk starts at n = 1).  nodes: n_nodes records in host memory.  Each lane's stack has `levels` slots
 * and four guard slots above them: a step stores into slot n + 3 at the most and n_stack + bottom <= levels is required, so no
 * item can make a store leave the block's allocation; 1 <= levels <= 60.
 * An item: the node to step at; the culling ray as DATA (no reciprocal enters); the f64 direction, which decides the binary
 * step's child order and, by its sign bits, the wide step's plane picks; t_max32; n_stack entries already on the stack -- the
 * top min(4, n_stack) of them are stack[0..], lowest first, and entry k below those holds 0x40000000 | k.  second_node >= 0:
 * after the step the lane resets its stack, as a new walk does, and takes one more step at that node.
 * out: 2 + levels + 4 words per item -- the new current item, the new n, then every slot; a slot no step wrote holds 0x0badf00d,
 * a guard slot 0x5ca1ab1e.  n <= 65536.  Blocking. */
typedef struct RtxWalkStepItem {
  int32_t node;
  int32_t second_node;
  float q[8];      /* ix iy iz, oix oiy oiz, err2, t_min */
  double dir[3];
  float t_max32;
  int32_t n_stack;
  int32_t stack[4];
} RtxWalkStepItem;
rtx_status rtx_device_walk_steps(int32_t f32, int32_t kind, int32_t bottom, const void* nodes, int64_t n_nodes, int32_t levels,
                                 int64_t n, const RtxWalkStepItem* items, int32_t* out);
/* The adaptive retirement check of rtx_progressive_add_adaptive (k_retire_flag / _scan / _scatter) on host arrays, through
 * the handle's own launch sequence.  S, Q: npix*3; active: n strictly ascending local pixels < npix; counts: npix, in/out
 * (spp at every pixel of the list with r <= target at n = spp, the rest unchanged); next: n, out (the others in order, the
 * first *kept valid).  Blocking. */
rtx_status rtx_device_retire(const double* S, const double* Q, uint32_t npix, const uint32_t* active, uint32_t n,
                             uint32_t spp, double target, int32_t* counts, uint32_t* next, uint32_t* kept);
/* The noise reduction of rtx_progressive_stats over npix pixels: k_noise_stats (counts NULL: every pixel at n = spp) or
 * k_noise_stats_counts (pixel lp at n = counts[lp], or spp where that is 0), then k_noise_stats_final.  Blocking.
 * Both entries: NULL pointers (counts excepted), spp < 2 and a negative or NaN target are RTX_EINVAL before any device
 * call; n = 0 or npix = 0 is RTX_OK with nothing kept or reduced. */
rtx_status rtx_device_noise_reduce(const double* S, const double* Q, const int32_t* counts, uint32_t npix, uint32_t spp,
                                   double target, double* max_r, double* sum_r, uint64_t* above);

/* Opaque pass-through for the CPU checkers under oracle/ (test infrastructure; not a render path). */
const void* rtx_builder_graph(const rtx_builder* b);
const void* rtx_flat_arrays(const rtx_flat* f);

#ifdef __cplusplus
}
#endif
#endif /* RTX_ABI_H */
