// HIP kernels and launcher for the per-pixel x per-sample loop of render_scene
// (/root/reference/src/world.rs:1207-1226) on gfx950.
//
//   k_trace_*        one camera path per (pixel, sample): path_begin + path_step loop
//                    (core/integrator.hpp), radiance written to the pass's sample buffer
//   k_reduce_samples per pixel, adds the pass's samples IN SAMPLE ORDER onto the accumulator
//                    (the reference's `pixel += ray_color(..)` order, world.rs:1215, so sums
//                    are bit-identical to a sequential CPU loop whatever the scheduling was)
//   k_tonemap        get_normalized_color (vec3.rs:89-107) -> RGB8
//
// No CPU fallback exists in this library: without a GPU every render entry point returns
// RTX_EHIP.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <new>
#include <type_traits>
#include <utility>
#include <string>
#include <vector>
#include "../../../include/rtx_abi.h"
#include "../core/cull32.hpp"
#include "../core/integrator.hpp"
#include "../core/occlusion.hpp"
#include "../core/nearest.hpp"
#include "../core/item_order.hpp"
#include "../core/karras.hpp"
#include "../core/mover_box.hpp"
#include "../core/prim_box.hpp"
#include "../host/flat_scene.hpp"
#include "../host/light_table.hpp"
#include "../host/update_shadow.hpp"
#include "../host/set_shading.hpp"
#include "../host/wide_tree.hpp"
#include "../host/ray_slices.hpp"  // for_ray_slices, slice_of: how the ray queries cut a batch (host-compilable: tests/ray_slices_host_check.cpp)
#include "device_buffer.hpp"
#include "f32_bridge.hpp"
#ifndef RTX_F32_TU
#include "abi_internal.hpp"
#include "../host/set_triangles.hpp"
#else
// The f32 compilation of this file (render_f32.hip) sees none of the C ABI's handle types: it exports its upload and its
// table of scene operations (f32_bridge.hpp) and render.hip proper owns the handles.
namespace rtx { void set_error(const std::string& msg); }
#endif

namespace rtx {

#include "lds_layout.inc"    // ring_bytes, LdsSceneDims, ldsk_layout: k_trace_lds's LDS layout (host-compilable: tests/lds_layout_host_check.cpp)
#include "lds_variant.inc"   // lds_common_interval, lds_trace_variant: which k_trace_lds a render launches (host-compilable: tests/lds_variant_host_check.cpp)
static_assert(LDSV_TIME_BOXES == RTX_LDS_VARIANT_TIME_BOXES && LDSV_ONE_AXIS == RTX_LDS_VARIANT_ONE_AXIS &&
              LDSV_COMMON_RATIO == RTX_LDS_VARIANT_COMMON_RATIO, "RtxRenderStats.trace_variant");
#include "pass_items.inc"    // ShardMap, item_pixel, start_path, store_sample, TRACE_CHUNK, lane_rank, queue_claim

// ------------------------------------------------------------------ device scene
typedef const FlatNode4 FlatNode4Dev;  // host/wide_tree.hpp
struct WorldDesc;

// The plain primitive entries beside the BVH in the world list (the dragon room's seven rectangles), as a kernel argument:
// list position, primitive reference and -- when all of them are rectangles -- the records themselves, for up to 8 entries.
// Read from the world list they cost three DEPENDENT scalar loads each, per ray (top_level[k] -> entries[..].a -> the
// primitive record); from the kernarg segment a record is one load at base + i * stride.  n < 0: not applicable, the kernel
// walks the list.  (Measured: the same loop fully unrolled over the 8 slots is 8 % SLOWER than the list walk -- eight copies
// of the three-axis rectangle test do not fit the instruction cache next to the rest of the kernel.)
struct VoteTop {
  int32_t n;
  int32_t all_rects;
  int32_t k[8];
  uint32_t ref[8];
  rt::FlatRect rect[8];
};

// RTX_TRACE_KERNEL: the kernel family a render is forced to (none: choose_trace_kernel decides).
enum class ForcedKernel { none, simple, vote, world, wavefront };

constexpr uint32_t RETIRE_UNSET = 0xFFFFFFFFu;
// Every RTX_* switch of the launcher, read once per rtx_scene_upload by read_switches (DESIGN section 4 lists them).  A numeric
// switch outside its range keeps the default; an on/off switch is off when set to anything atoi reads as 0.
struct TraceSwitches {
  ForcedKernel kernel = ForcedKernel::none;  // RTX_TRACE_KERNEL
  bool diag = false;  // RTX_TRACE_KERNEL=vote_diag / world_diag: region counters on stderr (never timed)
  int ring = -1, wide = -1, scene_lds = -1;  // RTX_RING / RTX_WIDE / RTX_SCENE_LDS: 0 / 1 when set, -1 when not
  bool vote_top = true, tri_direct = true, mat_lds = true, perlin_lds = true;  // RTX_VOTE_TOP / _TRI_DIRECT / _MAT_LDS / _PERLIN_LDS
  bool mv_common = true, motion = true, motion_axis = true;  // RTX_MV_COMMON / _MOTION / _MOTION_AXIS
  bool single_leaf = true, pass_pipeline = true, validate = false;  // RTX_SINGLE_LEAF / _PASS_PIPELINE; RTX_VALIDATE: set at all
  uint32_t chunk = TRACE_CHUNK;  // RTX_CHUNK [64, 65536]: sample indices a k_trace_lds wave reserves per grab
  uint32_t item_group = 0;       // RTX_ITEM_GROUP [1, 2^30]: pixels per group of a pass's item order (core/item_order.hpp); 0: WalkTuning's
  uint32_t world_threshold = 8;  // RTX_WORLD_THRESHOLD [0, 64]: k_trace_world's walk steps go first while this many lanes walk (0: majority)
  uint32_t walk_threshold = 0, regen_min = 0, leaf_weight = 0;  // RTX_WALK_THRESHOLD / _REGEN_MIN / _LEAF_WEIGHT [1, 64]; 0: WalkTuning's
  // RTX_RETIRE_DONE [0, 64] / RTX_RETIRE_MIN [0, 64]: k_trace_lds's miss-retire rule (trace_lds.inc), D and M; RETIRE_UNSET: WalkTuning's
  uint32_t retire_done = RETIRE_UNSET, retire_min = RETIRE_UNSET;
  // wavefront integrator: RTX_WF_PATHS [256, 2^27] path slots; RTX_WF_REFILL [1, 64] free lanes a wave waits for before it takes new
  // slots; RTX_WF_CHECK [1, 4096] iterations between two looks at the counters; RTX_WF_OCC [4, 6] blocks per CU k_wf_trace is
  // compiled for (mesh room); RTX_WF_VERBOSE set at all
  uint32_t wf_paths = 1u << 22, wf_refill = 16, wf_check = 8;
  int wf_occ = 4;
  bool wf_verbose = false;
};

// Render workspace, grown on demand by render calls.  Passes of one render run two deep (render_impl): odd passes on aux_stream
// with their own half of the sample buffer and their own work counter.
struct Workspace {
  DeviceBuffer<double> samples;
  DeviceBuffer<double> accum;
  DeviceBuffer<rt::TraceCounters> counters;
  DeviceBuffer<unsigned int> work_counter;  // two: one per pass stream
  DeviceBuffer<PassMap> pass_map;           // two likewise: a pass's item order and pixel map, where its trace kernel reads them (k_pass_begin)
  DeviceBuffer<unsigned long long> diag;    // region counters of the diagnostic instantiations (diag_clear / diag_print)
  hipEvent_t ev[2] = {nullptr, nullptr};  // trace time of a pass (stats)
  hipStream_t aux_stream = nullptr;
  hipEvent_t ev_pass[3] = {nullptr, nullptr, nullptr};  // reduction of an even / odd pass done; start of the render
  DeviceBuffer<unsigned char> wave_mem;   // the wavefront integrator's path pool
  uint32_t* wave_host_ctrl = nullptr;     // pinned
};

// k_trace_vote (trace_vote.inc), binary tree; the wavefront integrator applies to the same worlds.
struct VotePlan {
  bool ok = false;                // world == one BVH entry + plain primitive entries
  int32_t bvh_pos = 0;            // position of the BVH entry in the top-level list
  int32_t tri_base = -1;          // >= 0: that BVH is a pure triangle mesh whose slot s is triangle tri_base + s
  VoteTop top;                    // the plain entries beside the BVH, for the kernarg (n = -1: not applicable)
  int blocks_per_cu[2] = {1, 1};  // [preset]
  bool ring[2] = {false, false};  // a ring of ready primary rays in LDS (when it costs no occupancy)
  uint32_t tables = 0;            // wide k_trace_vote: materials | textures << 16 to keep in LDS (0: none)
  size_t tables_bytes = 0;
};

// 4-wide culling tree (FlatNode4) of every BVH of the scene, for k_trace_vote, k_trace_world and the wavefront integrator.
struct WidePlan {
  FlatNode4Dev* nodes4 = nullptr;
  int levels = 0;                 // stack levels of a wide walk
  int vote_blocks_per_cu = 1;
};

// k_trace_world (trace_world.inc).
struct WorldPlan {
  const WorldDesc* desc = nullptr;  // per-slot records of the world list
  uint32_t mat_lds = 0, tex_lds = 0;  // material / texture records it copies into LDS
  uint32_t perlin_lds = 0;          // Perlin tables it copies into LDS
  int blocks_per_cu[5][2] = {{1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}};  // [book2 preset / any / all incl. gravity spheres / no sphere media / instance trees (binary only)][binary / wide]
};

// One k_trace_lds variant fitted into the LDS of a block (fit_lds).
struct LdsFit {
  bool ok = false;
  uint32_t ring_cap = 0;          // entries per wave ring: 64 or 48 (0: no ring)
  uint32_t levels = 0;            // stack levels
  LdsSceneDims dims = {0, 0, 0, 0, 0, 0};
};

// k_trace_lds (trace_lds.inc): sphere worlds of one BVH whose geometry fits in LDS.
struct LdsPlan {
  LdsFit plain;                   // the binary tree
  // time-aware boxes: chosen per render, when the camera's shutter lies inside the BVH's time interval [motion_t0, motion_t1]
  LdsFit motion;
  int motion_axis = -1;           // 0 / 1 / 2: every slope of the time-aware boxes is zero except along this axis (-1: no such axis)
  double motion_t0 = 0.0, motion_t1 = 0.0;
  // the time-aware variant is planned: `motion` was fitted into lds_max bytes and is fitted again when the slopes change
  // (plan_lds_motion_axis; rtx_scene_set_moving_spheres)
  bool motion_planned = false;
  uint32_t lds_max = 0;
  bool mv_common = false;        // every MovingSphere of the scene has the same (time0, time1) = (mv_t0, mv_t1): one division per bounce
  double mv_t0 = 0.0, mv_t1 = 1.0;
};

// Tuning of the voting walks (k_trace_vote, k_trace_lds, k_trace_world, the wavefront integrator).
struct WalkTuning {
  uint32_t walk_threshold = 18;   // 1 = never carry a walk over; 18 measured best on C2 (12..22 within 1 %)
  uint32_t regen_min = 1;         // wide k_trace_vote: lanes that must be waiting before the wave regenerates
  uint32_t leaf_weight = 3;       // node lanes x weight >= leaf lanes -> node step
  bool single_leaf = false;       // every BVH leaf holds one primitive (k_trace_lds tests it without a loop)
  // k_trace_lds with a ring, miss retire (trace_lds.inc): a round hands its finished misses on once more than
  // retire_done (D) walks of it are complete and at least retire_min (M) of the complete ones are misses.  D = 0: off, a round
  // ends as a whole.  With the rule on a round may end later: retire_walk_threshold replaces walk_threshold for those launches.
  // Measured on C2 (short runs, Msamples/s; profiles/miss_retire/): off 8650, parent 8661 - 8712; threshold 12 with D / M
  // 40 / 12, 16, 20 -> 8694, 8792, 8798, 44 / 16, 20 -> 8762, 8778, 48 / 20 -> 8753, D >= 52 never fires; D / M 44 / 18 with
  // threshold 6, 8, 10, 14, 16 -> 8815, 8845, 8858, 8733, 8668; at 8 - 11 every D of 40, 44 and M of 16, 20 lies within 8840 - 8867.
  uint32_t retire_done = 44, retire_min = 18, retire_walk_threshold = 10;
  // Pixels per group of a pass's item order (core/item_order.hpp), per kernel family; ITEM_GROUP_MAX: one group, a wave's 64
  // consecutive items are a row strip of one sample.  RTX_ITEM_GROUP overrides all five.  (profiles/item_order/)
  // Measured (short runs, two each): k_trace_lds on C2 8304 in the row-strip order, 8699 / 8712 / 8689 / 8652 / 8592 / 8520 /
  // 8510 Msamples/s with 1 / 2 / 4 / 8 / 16 / 32 / 64; k_trace_world on C3 794 -> 825 / 826 / 827 / 827 / 823 / 819 / 814; wide
  // k_trace_vote on C4 within 0.3 % of the row-strip order for every size: kept.  Wavefront and simple: not measured, kept.
  uint32_t item_group_lds = 2, item_group_vote = rt::ITEM_GROUP_MAX, item_group_world = 4,
           item_group_wavefront = rt::ITEM_GROUP_MAX, item_group_simple = rt::ITEM_GROUP_MAX;
};

// rtx_scene_set_transforms (scene_update.inc): what an update needs beside the scene's arrays, kept from the upload.
struct SceneUpdate {
  UpdateShadow shadow;              // host: the slots' chains, the instance trees and their parent tables
  std::vector<double> local_box;    // host: FlatScene::member_local_box (an update's new boxes are checked before anything is enqueued)
  size_t n_entries = 0, n_nodes = 0, n_motion = 0, n_desc = 0;  // element counts of the arrays an update writes (rtx_device_scene_array)
  size_t n_triangles = 0, n_top = 0, n_spheres = 0, n_moving_spheres = 0, n_rects = 0;
  DeviceBuffer<double> d_local_box;
  DeviceBuffer<int32_t> d_leaf_parent, d_node_parent;
  DeviceBuffer<unsigned int> d_arrivals;        // one counter per tree node
  DeviceBuffer<rt::XformOp64> d_slot_ops64;     // the f32 compilation only: the slots' ops in f64
  StagingBuffer staging;                        // the update records of one call
  ShadingShadow shading;                        // host: what rtx_scene_set_shading checks and plans its edits against (shading_update.inc)
  // rtx_scene_rebuild_instance_trees (scene_rebuild.inc).  max_stack = member_stack + 1 + the deepest of tree_depth.
  int32_t member_stack = 0;                     // host: the members' own part of max_stack (their deepest BVH)
  std::vector<int32_t> tree_depth;              // host: per instance tree, as the trees now stand
  size_t n_perlins = 0, n_materials = 0, n_textures = 0;  // what plan_world_stacks fits into LDS beside the stacks
  // scratch of a rebuild, laid out like the shadow's per-member / per-node tables; allocated by the first rebuild
  DeviceBuffer<double> r_boxes, r_bounds, r_box64, r_terms;
  DeviceBuffer<unsigned long long> r_keys, r_keys_sorted;
  DeviceBuffer<uint32_t> r_vals, r_vals_sorted;
  DeviceBuffer<int32_t> r_children, r_parent_node, r_parent_leaf, r_leaf_parent, r_node_parent, r_depth;
  DeviceBuffer<rt::FlatNode> r_nodes;
  DeviceBuffer<rt::FlatNode32> r_nodes32;
  DeviceBuffer<rt::FlatMotion32> r_motion32;
  DeviceBuffer<unsigned char> r_sort_temp;      // the radix sort's temporary storage, grown on demand
};

#ifndef RTX_F32_TU
// rtx_scene_set_triangles and rtx_scene_set_spheres (mesh_update.inc): the shadow of the upload's meshes and spheres and what
// the device keeps of it.  f64 scenes only.
struct MeshUpdate {
  MeshShadow shadow;                             // host: id -> flat triangles, the BVHs' leaves and parent tables, members, plain slots
  bool uploaded = false;                         // the tables below are resident: done by the first update
  DeviceBuffer<int32_t> d_leaves, d_node_parent; // MeshShadow::leaves, ::node_parent
  DeviceBuffer<unsigned int> d_arrivals;         // one counter per BVH node
  StagingBuffer staging;                         // one call's vertices (host entry) and index lists; its own, so that a call does
                                                 // not wait for the copy of the last rtx_scene_set_transforms
  bool local_box_stale = false;                  // SceneUpdate::local_box lags behind d_local_box (scene_update.inc reads it back)
  std::vector<char> sphere_is_light;             // host, per flat sphere: it is a sampled light (an update of it refreshes the light table)
  std::vector<char> rect_is_light;               // the same per flat rectangle
  DeviceBuffer<double> d_light_weight;           // k_refresh_lights' pick weights, one per light; allocated by the first such update
  // rtx_scene_set_moving_spheres (k_refit_timed_bvh); allocated by the first such update
  std::vector<unsigned int> slope_mask;          // host, per BVH: the axes its time-aware boxes have a slope along, as uploaded
  DeviceBuffer<unsigned int> d_slope_mask;       // the same words, kept current by the refits
  DeviceBuffer<double> d_end_boxes;              // the climb's scratch: 24 doubles per BVH node (scene_update.inc: EndBoxes)
  ReadbackWords slope_readback;                  // d_slope_mask on its way to launch_lds, which plans k_trace_lds's instantiation by it
};
#endif

struct DeviceScene {
  int device = -1;
  std::vector<DeviceBuffer<void>> allocations;  // the uploaded arrays
  rt::SceneView view;   // device pointers into them (a kernel argument)
  size_t scene_bytes = 0;
  int n_cu = 256;
  double gravity_time_limit = 1e300;  // scenes with GravitySpheres: the largest shutter time a render accepts
  TraceSwitches sw;
  Workspace ws;
  VotePlan vote;
  WidePlan wide;
  WorldPlan world;
  LdsPlan lds;
  WalkTuning walk;
  rt::LightView lights = {nullptr, nullptr, 0, 0};  // next-event estimation's light table (k_trace_nee), uploaded with the scene
  SceneUpdate upd;
#ifndef RTX_F32_TU
  MeshUpdate mesh;
#endif
};

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess) {                                                                \
      set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                        \
      return RTX_EHIP;                                                                     \
    }                                                                                      \
  } while (0)

template <class T>
static rtx_status upload_array(DeviceScene* ds, const std::vector<T>& v, const T** out) {
  *out = nullptr;
  if (v.empty()) return RTX_OK;
  DeviceBuffer<void> b;
  size_t bytes = v.size() * sizeof(T);
  HIP_TRY(b.alloc(bytes));
  HIP_TRY(hipMemcpy(b, v.data(), bytes, hipMemcpyHostToDevice));
  ds->scene_bytes += bytes;
  *out = (const T*)(void*)b;
  ds->allocations.push_back(std::move(b));
  return RTX_OK;
}

// Releases what has no owner of its own; the buffers go with the DeviceScene.
static void free_device_scene(DeviceScene* ds) {
  if (!ds) return;
  Workspace& ws = ds->ws;
  if (ws.wave_host_ctrl) (void)hipHostFree(ws.wave_host_ctrl);
  for (int i = 0; i < 2; ++i)
    if (ws.ev[i]) (void)hipEventDestroy(ws.ev[i]);
  for (int i = 0; i < 3; ++i)
    if (ws.ev_pass[i]) (void)hipEventDestroy(ws.ev_pass[i]);
  if (ws.aux_stream) (void)hipStreamDestroy(ws.aux_stream);
  delete ds;
}

// Load through the constant address space: the address is wave-uniform, the compiler may use a scalar load.
template <class T>
__device__ __forceinline__ T dev_load_uniform(const T* p) { return *(const __attribute__((address_space(4))) T*)(p); }

// 64-bit lane mask of a predicate, straight from the compare (HIP's __ballot(int) first materialises 0/1 in a VGPR).
__device__ __forceinline__ unsigned long long wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// ------------------------------------------------------------------ LDS traversal stack
// Slot (level, lane) lives at base[level * TRACE_BLOCK]: lanes of a wave touch consecutive
// dwords -> conflict-free ds_write_b32 / ds_read_b32.
#define TRACE_BLOCK 256
struct LdsStack {
  int32_t* base;
  int n;
  static constexpr bool kBottom = false;
  __device__ __forceinline__ void reset() { n = 0; }
  __device__ __forceinline__ void push(int32_t v) { base[n * TRACE_BLOCK] = v; ++n; }
  __device__ __forceinline__ int32_t pop() { --n; return base[n * TRACE_BLOCK]; }
  __device__ __forceinline__ bool empty() const { return n == 0; }
};
// The same stack with a bottom: slot 0 of every thread holds "walk done" (0x7fffffff = WALK_DONE, trace_vote.inc) while a walk
// is on and the walk's own entries start at slot 1, so popping an "empty" stack returns "done" like any other item -- no
// emptiness test, no branch in the step functions (k_trace_vote, k_trace_world; k_trace_lds has its 16-bit twin).  The spare
// level every launcher already sizes the stacks with (tree height + 1, wide: peak + 1) is this slot.  reset() writes it anew
// for every walk: the wide step's last act on an exhausted stack is to dump its four missed children there (walk_node_step4).
struct LdsStackB {
  int32_t* base;
  int n;
  static constexpr bool kBottom = true;
  __device__ __forceinline__ void reset() { base[0] = 0x7fffffff; n = 1; }
  __device__ __forceinline__ void init() { reset(); }
  __device__ __forceinline__ void push(int32_t v) { base[n * TRACE_BLOCK] = v; ++n; }
  __device__ __forceinline__ int32_t pop() { --n; return base[n * TRACE_BLOCK]; }
  __device__ __forceinline__ int32_t top() const { return base[(n - 1) * TRACE_BLOCK]; }
  __device__ __forceinline__ bool empty() const { return n <= 1; }
};

__device__ __forceinline__ void flush_counters(const rt::TraceCounters& c, rt::TraceCounters* g) {
  atomicAdd(&g->box_tests, c.box_tests);
  atomicAdd(&g->sphere_tests, c.sphere_tests);
  atomicAdd(&g->moving_sphere_tests, c.moving_sphere_tests);
  atomicAdd(&g->rect_tests, c.rect_tests);
  atomicAdd(&g->triangle_tests, c.triangle_tests);
  atomicAdd(&g->scatters, c.scatters);
  atomicAdd(&g->texels, c.texels);
  atomicAdd(&g->perlin_calls, c.perlin_calls);
  atomicAdd(&g->rays, c.rays);
  atomicAdd(&g->samples, c.samples);
}

// ------------------------------------------------------------------ kernels
// The diagnostic instantiations' counters (k_trace_vote and k_trace_world with DIAG; run_diag below prints them): region k of a
// kernel's `dg` array gets one execution and the lanes of `mask`.  Compiled out of every other instantiation.
#define DIAG_ADD(region, mask) do { if (DIAG) { dg[2 * (region)] += 1; dg[2 * (region) + 1] += (unsigned long long)__popcll(mask); } } while (0)
#include "trace_basic.inc"   // feature presets, k_trace_simple
#include "trace_vote.inc"    // voting walk, 4-wide tree, k_trace_vote
#include "trace_world.inc"   // k_trace_world: any world, per-lane scan of the world list with carried-over walks
#include "trace_lds.inc"     // k_trace_lds (the headline kernel)
#include "trace_wave.inc"    // k_wf_generate / k_wf_trace / k_wf_shade: the split-kernel integrator (path state in HBM)
#include "post_kernels.inc"  // k_reduce_samples, k_tonemap, device self tests
#include "denoise.inc"       // k_features (first-hit albedo / normal), the a-trous filter of a progressive frame
#include "cast_rays.inc"     // QueryRays; k_cast_rays: closest-hit casts of a caller's ray batch (rtx_scene_cast_rays*)
#include "trace_rays.inc"    // k_trace_rays: the estimator's radiance along a caller's rays (rtx_scene_trace_rays*)
#include "gather.inc"        // k_gather, k_reduce_samples_sh: light arriving at a caller's points (rtx_scene_gather*)
#include "occlusion.inc"     // k_occlusion: any-hit segment casts with exact fog depth (rtx_scene_occlusion*)
#include "nearest.inc"       // k_nearest: the closest surface point of the world list per point (rtx_scene_nearest*)
#ifndef RTX_F32_TU
#include "trace_nee.inc"     // k_trace_nee: next-event estimation with MIS (rtx_render_ex, light_sampling = 1; f64 only)
#endif
#include "scene_update.inc"  // k_set_slot_ops, k_refit_instance_tree: new Translate / RotateY parameters on a resident scene
static size_t stack_bytes(uint32_t levels);
static void plan_world_stacks(DeviceScene* ds);
#include "scene_rebuild.inc" // k_member_boxes .. k_rebuild_emit: a new topology for an instance tree of a resident scene; its cost
#ifndef RTX_F32_TU
#include "mesh_update.inc"   // k_set_prims .. k_refresh_lights: new records for triangles / static spheres of a resident scene, BVHs refitted (f64 only)
#endif
#include "shading_update.inc" // k_set_shading: new colours, noise scales, metal / glass parameters and fog densities on a resident scene
#include "cull_hooks.inc"    // k_cull_verdicts, k_walk_steps: test hooks of the f32 culling code (rtx_device_cull_verdicts / _walk_steps)

// ------------------------------------------------------------------ launcher
static int shard_row_count(int32_t height, const RtxShard& sh, int32_t row_limit) {
  int n = 0;
  for (int32_t j = 0; j < height && j < row_limit; ++j)
    if ((j / sh.block_rows) % sh.shard_count == sh.shard_index) ++n;
  return n;
}

static rtx_status validate(const void* s, const RtxCamera* cam, const RtxConfig* cfg,
                           const RtxShard* shard, RtxShard* sh_out) {
  if (!s || !cam || !cfg) { set_error("render: NULL scene, camera or config"); return RTX_EINVAL; }
  if (cfg->threads <= 0 || cfg->image_width <= 0 || cfg->samples_per_pixel <= 0 || cfg->max_depth <= 0) {
    set_error("render: Config::new asserts threads, image_width, samples_per_pixel, max_depth > 0 (world.rs:36-40)");
    return RTX_EINVAL;
  }
  if (rtx_image_height(cfg) <= 0) { set_error("render: image height <= 0 (Screen::new asserts, screen.rs:14)"); return RTX_EINVAL; }
  if (!(cam->time1 < cam->time2)) { set_error("render: camera time1 >= time2 (gen_range panics on an empty range, camera.rs:69)"); return RTX_EINVAL; }
  RtxShard sh = {0, 1, 1, 0};
  if (shard) sh = *shard;
  if (sh.shard_count <= 0 || sh.shard_index < 0 || sh.shard_index >= sh.shard_count || sh.block_rows <= 0) {
    set_error("render: bad shard");
    return RTX_EINVAL;
  }
  *sh_out = sh;
  return RTX_OK;
}

static rt::RenderParams make_params(const RtxCamera* cam, const RtxConfig* cfg) {
  rt::RenderParams rp;
  static_assert(sizeof(RtxCamera) == 24 * sizeof(double) && sizeof(rt::FlatCamera) == 24 * sizeof(rt::real), "camera layout");
  for (int k = 0; k < 24; ++k) ((rt::real*)&rp.cam)[k] = (rt::real)((const double*)cam)[k];
  rp.background = rt::v3(cfg->background[0], cfg->background[1], cfg->background[2]);
  rp.image_width = cfg->image_width;
  rp.image_height = rtx_image_height(cfg);
  rp.samples_per_pixel = cfg->samples_per_pixel;
  rp.max_depth = cfg->max_depth;
  rp.seed = cfg->seed;
  return rp;
}

// ------------------------------------------------------------------ switches and common helpers
static TraceSwitches read_switches() {
  // a numeric switch: its value when set and within [lo, hi], else dflt; an on/off switch: 1 or 0 when set, -1 when not
  auto num = [](const char* n, int lo, int hi, uint32_t dflt) { const char* s = getenv(n); return s && atoi(s) >= lo && atoi(s) <= hi ? (uint32_t)atoi(s) : dflt; };
  auto flag = [](const char* n) { const char* s = getenv(n); return s ? (atoi(s) != 0 ? 1 : 0) : -1; };
  TraceSwitches sw;
  if (const char* k = getenv("RTX_TRACE_KERNEL")) {
    const std::string s = k;
    if (s == "simple") sw.kernel = ForcedKernel::simple;
    else if (s == "vote" || s == "vote_diag") sw.kernel = ForcedKernel::vote;
    else if (s == "world" || s == "world_diag") sw.kernel = ForcedKernel::world;
    else if (s == "wavefront") sw.kernel = ForcedKernel::wavefront;
    sw.diag = s == "vote_diag" || s == "world_diag";
  }
  sw.ring = flag("RTX_RING"); sw.wide = flag("RTX_WIDE"); sw.scene_lds = flag("RTX_SCENE_LDS");
  sw.vote_top = flag("RTX_VOTE_TOP") != 0; sw.tri_direct = flag("RTX_TRI_DIRECT") != 0;
  sw.mat_lds = flag("RTX_MAT_LDS") != 0; sw.perlin_lds = flag("RTX_PERLIN_LDS") != 0;
  sw.mv_common = flag("RTX_MV_COMMON") != 0; sw.motion = flag("RTX_MOTION") != 0; sw.motion_axis = flag("RTX_MOTION_AXIS") != 0;
  sw.single_leaf = flag("RTX_SINGLE_LEAF") != 0; sw.pass_pipeline = flag("RTX_PASS_PIPELINE") != 0;
  sw.validate = getenv("RTX_VALIDATE") != nullptr;
  sw.chunk = num("RTX_CHUNK", 64, 65536, sw.chunk);
  sw.item_group = num("RTX_ITEM_GROUP", 1, (int)rt::ITEM_GROUP_MAX, 0);
  sw.world_threshold = num("RTX_WORLD_THRESHOLD", 0, 64, sw.world_threshold);
  sw.walk_threshold = num("RTX_WALK_THRESHOLD", 1, 64, 0); sw.regen_min = num("RTX_REGEN_MIN", 1, 64, 0); sw.leaf_weight = num("RTX_LEAF_WEIGHT", 1, 64, 0);
  sw.retire_done = num("RTX_RETIRE_DONE", 0, 64, RETIRE_UNSET); sw.retire_min = num("RTX_RETIRE_MIN", 0, 64, RETIRE_UNSET);
  const char* wp = getenv("RTX_WF_PATHS");
  if (wp && atol(wp) >= 256 && atol(wp) <= (1l << 27)) sw.wf_paths = (uint32_t)atol(wp);
  sw.wf_refill = num("RTX_WF_REFILL", 1, 64, sw.wf_refill); sw.wf_check = num("RTX_WF_CHECK", 1, 4096, sw.wf_check);
  sw.wf_occ = (int)num("RTX_WF_OCC", 4, 6, (uint32_t)sw.wf_occ); sw.wf_verbose = getenv("RTX_WF_VERBOSE") != nullptr;
  return sw;
}

// LDS bytes of the traversal stacks of a TRACE_BLOCK-thread block
static size_t stack_bytes(uint32_t levels) { return (size_t)levels * TRACE_BLOCK * sizeof(int32_t); }

// Resident TRACE_BLOCK-thread blocks per CU of a kernel with `lds` bytes of dynamic LDS (0: the query failed).
template <class K>
static int occupancy(K kernel, size_t lds) {
  int nb = 0;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, TRACE_BLOCK, lds) == hipSuccess ? nb : 0;
}

// Grid of a persistent launch: one block per `block` work items, at most `resident` blocks.
static uint32_t grid_size(uint32_t total, uint32_t block, uint64_t resident) {
  const uint64_t want = ((uint64_t)total + block - 1) / block;
  return (uint32_t)(want < resident ? want : resident);
}

// What every trace launch of one pass takes (render_impl's pass loop).
struct PassArgs {
  rt::RenderParams rp;
  ShardMap sm;                    // points at the pass's PassMap (render_impl writes one per pass: k_pass_begin)
  uint32_t s_begin, total, npix;  // absolute index of the pass's first sample; (sample, pixel) items of the pass; pixels of the shard
  double* samples;                // this pass's half of the sample buffer, its work counter and stream
  unsigned int* work_counter;
  hipStream_t stream;
  int preset;                     // 0 spheres / 1 mesh / 2 anything (P_SPHERES, P_MESH); feat: the scene's features
  uint32_t feat;
  uint32_t stack_levels;          // of the binary tree (max_stack + 1) and the bytes of its stacks
  size_t stack_lds;
  const uint32_t* active;         // an adaptive pass: its list of active local pixels (ActiveMap, pass_items.inc); else NULL
};

// Calls launch(map) with the pass's pixel map: the shard's ShardMap, or an ActiveMap over an adaptive pass's list.  Each trace
// kernel has one instantiation per map type, so the uniform one carries neither the list nor a test for it.
template <class Launch>
static void with_map(const PassArgs& a, Launch launch) {
  if (a.active) launch(ActiveMap{a.sm, a.active});
  else launch(a.sm);
}

// The diagnostic instantiations (RTX_TRACE_KERNEL=vote_diag / world_diag) count executions and active lanes per region into
// ws.diag.  run_diag clears the counters, launches, waits for the kernel and prints one line per region into stderr; h gets
// the counters.  Never timed; scripts/kernel_diag.py and DESIGN section 5.3 read these lines.
template <class Launch>
static rtx_status run_diag(DeviceScene* ds, hipStream_t stream, Launch launch, const char* tag, int width, const char* const* names,
                           int n, unsigned long long (&h)[24]) {
  if (!ds->ws.diag) HIP_TRY(ds->ws.diag.alloc(sizeof(h)));
  HIP_TRY(hipMemsetAsync(ds->ws.diag, 0, sizeof(h), stream));
  launch();
  HIP_TRY(hipStreamSynchronize(stream));
  HIP_TRY(hipMemcpy(h, ds->ws.diag, sizeof(h), hipMemcpyDeviceToHost));
  for (int k = 0; k < n; ++k)
    fprintf(stderr, "[%s] %-*s executions %llu lanes %llu mean lanes %.2f\n", tag, width, names[k], h[2 * k], h[2 * k + 1],
            h[2 * k] ? (double)h[2 * k + 1] / (double)h[2 * k] : 0.0);
  return RTX_OK;
}

// Leaves of the scene's binary BVH nodes: the most primitives in one leaf, the end of the highest leaf slot.
struct LeafScan { uint32_t max_count = 0, max_end = 0; };
static LeafScan scan_leaves(const FlatScene& fs) {
  LeafScan s;
  for (const rt::FlatNode& nd : fs.nodes)
    for (int ch = 0; ch < 2; ++ch)
      if (nd.child[ch] < 0) {
        s.max_count = std::max(s.max_count, rt::leaf_count(nd.child[ch]));
        s.max_end = std::max(s.max_end, rt::leaf_first(nd.child[ch]) + rt::leaf_count(nd.child[ch]));
      }
  return s;
}

// ------------------------------------------------------------------ k_trace_vote
static void plan_vote(DeviceScene* ds, const FlatScene& fs) {
  VotePlan& p = ds->vote;
  const TraceSwitches& sw = ds->sw;
  const size_t lds = stack_bytes((uint32_t)fs.max_stack + 1u), lds_ring = lds + (TRACE_BLOCK / 64) * ring_bytes(64);
  const bool ring_fits = lds_ring <= 64 * 1024;
  auto fit = [&](int preset, int nb0, int nb1, bool ring_by_default) {
    p.ring[preset] = ring_by_default && nb1 > 0 && nb1 >= nb0 && ring_fits;
    if (sw.ring >= 0 && nb1 > 0 && ring_fits) p.ring[preset] = sw.ring != 0;
    const int nb = p.ring[preset] ? nb1 : nb0;
    if (nb > 0) p.blocks_per_cu[preset] = nb;
  };
  fit(0, occupancy(k_trace_vote<P_SPHERES, false, false, false>, lds), occupancy(k_trace_vote<P_SPHERES, false, true, false>, lds_ring), true);
  // measured on the mesh room: no gain from the ring, and its live state spills 50 dwords there
  fit(1, occupancy(k_trace_vote<P_MESH, false, false, false>, lds), occupancy(k_trace_vote<P_MESH, false, true, false>, lds_ring), false);

  memset(&p.top, 0, sizeof(p.top));
  p.top.n = -1;
  int n_bvh = 0, n_other = 0;
  for (size_t k = 0; k < fs.top_level.size(); ++k) {
    const int32_t kind = fs.entries[fs.top_level[k]].kind;
    if (kind == rt::ENTRY_BVH) { ++n_bvh; p.bvh_pos = (int32_t)k; }
    else if (kind != rt::ENTRY_PRIM) ++n_other;
  }
  p.ok = n_bvh == 1 && n_other == 0;
  if (p.ok && fs.top_level.size() <= 9 && sw.vote_top) {
    p.top.n = 0;
    p.top.all_rects = 1;
    for (size_t k = 0; k < fs.top_level.size(); ++k) {
      if ((int32_t)k == p.bvh_pos) continue;
      const rt::PrimRef ref = (rt::PrimRef)fs.entries[fs.top_level[k]].a;
      p.top.k[p.top.n] = (int32_t)k;
      p.top.ref[p.top.n] = (uint32_t)ref;
      if (rt::primref_type(ref) == rt::PRIM_RECT) p.top.rect[p.top.n] = fs.rects[rt::primref_index(ref)];
      else p.top.all_rects = 0;
      p.top.n += 1;
    }
    if (!p.top.all_rects) p.top.n = -1;
  }
  if (p.ok) {
    const rt::FlatEntry& be = fs.entries[fs.top_level[p.bvh_pos]];
    bool pure = be.c > 0 && rt::primref_type(fs.refs[be.b]) == rt::PRIM_TRIANGLE;
    const uint32_t t0 = pure ? rt::primref_index(fs.refs[be.b]) : 0u;
    for (int32_t k = 0; pure && k < be.c; ++k)
      pure = fs.refs[be.b + k] == rt::make_primref(rt::PRIM_TRIANGLE, t0 + (uint32_t)k);
    if (pure && sw.tri_direct) p.tri_base = (int32_t)t0;
  }
  if (!fs.materials.empty() && !fs.textures.empty() && fs.materials.size() <= 16 && fs.textures.size() <= 16 && sw.mat_lds) {
    p.tables = (uint32_t)fs.materials.size() | ((uint32_t)fs.textures.size() << 16);
    p.tables_bytes = fs.materials.size() * sizeof(rt::FlatMaterial) + fs.textures.size() * sizeof(rt::FlatTexture);
  }
}

// The wide instantiations (preset 1 with a 4-wide tree): material / texture records behind the stacks when that costs no
// resident block.
static rtx_status launch_vote_wide(DeviceScene* ds, const PassArgs& a, bool diag) {
  const VotePlan& p = ds->vote;
  const WidePlan& wt = ds->wide;
  uint32_t lds_tables = 0;
  size_t lds = stack_bytes((uint32_t)wt.levels);
  if (p.tables_bytes > 0 && lds + p.tables_bytes <= 64 * 1024 && (lds + p.tables_bytes) * (size_t)wt.vote_blocks_per_cu <= 160 * 1024) {
    lds_tables = p.tables;
    lds += p.tables_bytes;
  }
  const uint32_t grid = grid_size(a.total, TRACE_BLOCK, (uint64_t)ds->n_cu * (uint64_t)wt.vote_blocks_per_cu);
  const uint32_t threshold = ds->walk.walk_threshold | (ds->walk.regen_min << 16);
#define LAUNCH_VOTE_WIDE(FEAT, DIAGF, THRESHOLD, MAP)                                                                  \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trace_vote<FEAT, DIAGF, false, true, decltype(MAP)>), dim3(grid), dim3(TRACE_BLOCK), lds, \
                     a.stream, ds->view, a.rp, MAP, a.s_begin, a.total, a.samples, a.work_counter,             \
                     DIAGF ? ds->ws.diag : nullptr, ds->walk.leaf_weight, THRESHOLD, (uint32_t)wt.levels,              \
                     (uint32_t)p.bvh_pos, wt.nodes4, p.tri_base, lds_tables, p.top)
  // a triangle mesh in a room of rectangles, no spheres / lists / glass (the dragon room): the leaner instantiation
  const bool room = (a.feat & ~P_MESH_ROOM) == 0;
  if (diag && room) {
    unsigned long long h[24];
    static const char* const names[6] = {"outer", "regen", "node_step", "leaf_step", "shade_hit", "shade_all"};
    const rtx_status st = run_diag(ds, a.stream, [&] { LAUNCH_VOTE_WIDE(P_MESH_ROOM, true, ds->walk.walk_threshold, a.sm); }, "vote_diag", 10, names, 6, h);
    if (st != RTX_OK) return st;
    if (h[12]) {
      float v[12];
      for (int k = 0; k < 6; ++k) { uint32_t lo = (uint32_t)h[13 + k], hi = (uint32_t)(h[13 + k] >> 32); memcpy(&v[2 * k], &lo, 4); memcpy(&v[2 * k + 1], &hi, 4); }
      fprintf(stderr, "[vote_diag] %llu walks of >= 50000 node steps; the first: origin (%g %g %g) direction (%g %g %g) 1/d (%g %g %g) err2 %g t_min %g t_max %g depth left %llu\n",
              h[12], v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], h[19]);
    }
  } else if (room) {
    with_map(a, [&](auto map) { LAUNCH_VOTE_WIDE(P_MESH_ROOM, false, threshold, map); });
  } else {
    with_map(a, [&](auto map) { LAUNCH_VOTE_WIDE(P_MESH, false, threshold, map); });
  }
#undef LAUNCH_VOTE_WIDE
  return RTX_OK;
}

static rtx_status launch_vote(DeviceScene* ds, const PassArgs& a) {
  const VotePlan& p = ds->vote;
  const bool diag = ds->sw.kernel == ForcedKernel::vote && ds->sw.diag && !a.active;  // (diagnostics: uniform passes only)
  if (a.preset == 1 && ds->wide.nodes4) return launch_vote_wide(ds, a, diag);
  const bool ring = p.ring[a.preset];
  const size_t lds = a.stack_lds + (ring ? (TRACE_BLOCK / 64) * ring_bytes(64) : 0);
  const uint32_t grid = grid_size(a.total, TRACE_BLOCK, (uint64_t)ds->n_cu * (uint64_t)p.blocks_per_cu[a.preset]);
#define LAUNCH_VOTE3(FEAT, DIAGF, RINGF, MAP)                                                                            \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trace_vote<FEAT, DIAGF, RINGF, false, decltype(MAP)>), dim3(grid), dim3(TRACE_BLOCK), lds, \
                     a.stream, ds->view, a.rp, MAP, a.s_begin, a.total, a.samples, a.work_counter,              \
                     DIAGF ? ds->ws.diag : nullptr, ds->walk.leaf_weight, ds->walk.walk_threshold, a.stack_levels,      \
                     (uint32_t)p.bvh_pos, (const FlatNode4*)nullptr, p.tri_base, 0u, p.top)
#define LAUNCH_VOTE2(FEAT, RINGF) with_map(a, [&](auto map) { LAUNCH_VOTE3(FEAT, false, RINGF, map); })
#define LAUNCH_VOTE(FEAT) do { if (ring) { LAUNCH_VOTE2(FEAT, true); } else { LAUNCH_VOTE2(FEAT, false); } } while (0)
  if (diag && a.preset == 0) {  // (the diagnostic instantiations exist for the shard's map only)
    unsigned long long h[24];
    static const char* const names[6] = {"outer", "regen", "node_step", "leaf_step", "shade_hit", "walking"};
    return run_diag(ds, a.stream, [&] {
      if (ring) { LAUNCH_VOTE3(P_SPHERES, true, true, a.sm); } else { LAUNCH_VOTE3(P_SPHERES, true, false, a.sm); }
    }, "vote_diag", 10, names, 6, h);
  }
  if (a.preset == 0) { LAUNCH_VOTE(P_SPHERES); }
  else { LAUNCH_VOTE(P_MESH); }
#undef LAUNCH_VOTE
#undef LAUNCH_VOTE2
#undef LAUNCH_VOTE3
  return RTX_OK;
}

// ------------------------------------------------------------------ 4-wide tree
// Host check (RTX_VALIDATE): walk every wide tree, codes in range, stack use within `levels`.
static void validate_wide_tree(const FlatScene& fs, const std::vector<FlatNode4>& wide, int levels) {
  for (const rt::FlatEntry& e : fs.entries) {
    if (e.kind != rt::ENTRY_BVH) continue;
    std::vector<std::pair<int32_t, int>> todo;  // (code, stack entries below it)
    todo.push_back({e.a, 0});
    size_t visited = 0, bad = 0; int deepest = 0;
    while (!todo.empty()) {
      auto [code, below] = todo.back(); todo.pop_back();
      if (code < 0) { if (rt::leaf_first(code) + rt::leaf_count(code) > (uint32_t)e.c) ++bad; continue; }
      if ((size_t)code >= wide.size()) { ++bad; continue; }
      ++visited;
      int nk = 0;
      for (int k = 0; k < 4; ++k) if (wide[code].child[k] != 0x7fffffff) ++nk;
      deepest = std::max(deepest, below + nk);
      for (int k = 0; k < 4; ++k) if (wide[code].child[k] != 0x7fffffff) todo.push_back({wide[code].child[k], below + nk - 1});
    }
    fprintf(stderr, "[rtx] RTX_VALIDATE: BVH root %d refs %d: %zu wide nodes walked, %zu bad codes, deepest stack %d of %d levels, sizeof(real) %zu\n",
            e.a, e.c, visited, bad, deepest, levels, sizeof(rt::real));
  }
}

// 4-wide culling tree (see FlatNode4) for every BVH of the scene: big triangle meshes under k_trace_vote (needs VotePlan::ok),
// and any world but a sphere-only one that k_trace_world walks (Book-2: two BVHs walked per bounce, each step a dependent L2
// fetch).  RTX_WIDE=0/1 overrides the size tests.
static rtx_status plan_wide(DeviceScene* ds, const FlatScene& fs) {
  WidePlan& p = ds->wide;
  const bool spheres_preset = (fs.features & ~P_SPHERES) == 0;
  const bool mesh_preset = !spheres_preset && (fs.features & ~P_MESH) == 0;
  const int preset = spheres_preset ? 0 : (mesh_preset ? 1 : 2);
  const bool for_vote = ds->vote.ok && mesh_preset;
  const bool for_world = !(ds->vote.ok && preset < 2) && preset >= 1;
  bool want_wide = (for_vote && fs.nodes.size() >= 4096) || (for_world && fs.nodes.size() >= 256);
  if (ds->sw.wide >= 0) want_wide = (for_vote || for_world) && ds->sw.wide != 0 && !fs.nodes.empty();
  // a world with an instance tree keeps the binary tree: the slot walk and the member walks above it share one node format
  // and one stack (trace_world.inc), and a wide collapse of a slot tree has no leaf format for slots
  if (fs.features & rt::F_INSTANCE) want_wide = false;
  if (!want_wide) return RTX_OK;
  std::vector<FlatNode4> wide;
  std::vector<int32_t> roots;
  for (const rt::FlatEntry& e : fs.entries)
    if (e.kind == rt::ENTRY_BVH) roots.push_back(e.a);
  p.levels = build_wide_tree(fs.nodes, roots, &wide);  // (peak + 1: the spare level is the bottom slot of LdsStackB)
  const size_t lds = stack_bytes((uint32_t)p.levels);
  bool ok = lds <= 64 * 1024;
  if (ok && for_vote) {
    const int nb = occupancy(k_trace_vote<P_MESH, false, false, true>, lds);
    ok = nb > 0;
    if (ok) p.vote_blocks_per_cu = nb;
  }
  if (ok) {
    rtx_status st = upload_array(ds, wide, &p.nodes4);
    if (st != RTX_OK) return st;
  }
  if (ds->sw.wide >= 0) fprintf(stderr, "[rtx] RTX_WIDE: 4-wide tree %s (%d stack levels)\n", p.nodes4 ? "on" : "off", p.levels);
  if (ds->sw.validate) validate_wide_tree(fs, wide, p.levels);
  return RTX_OK;
}

// ------------------------------------------------------------------ k_trace_world
// Needs WidePlan: the LDS tables go with the stacks of the tree the kernel walks.
// What of k_trace_world's plan depends on the stack levels: the LDS tables that fit beside the stacks and the resident blocks.
// From ds->view.max_stack, so that a rebuild of an instance tree (scene_rebuild.inc), which changes it, plans again.
static void plan_world_stacks(DeviceScene* ds) {
  WorldPlan& p = ds->world;
  const TraceSwitches& sw = ds->sw;
  const SceneUpdate& u = ds->upd;
  p.perlin_lds = p.mat_lds = p.tex_lds = 0;
  for (int wd = 0; wd < 2; ++wd) {
    const uint32_t levels = (uint32_t)(wd ? ds->wide.levels : ds->view.max_stack + 1);
    size_t wl = stack_bytes(levels) + (size_t)WORLD_SLOT_F64 * TRACE_BLOCK * sizeof(rt::real);
    if (wl > 64 * 1024) continue;
    // Perlin tables in LDS when that costs no resident block (3 per CU at 168 VGPRs: up to 53 KB each)
    if ((wd != 0) == (ds->wide.nodes4 != nullptr)) {
      const size_t n_p = u.n_perlins;
      if (n_p >= 1 && n_p <= 2 && sw.perlin_lds && wl + n_p * sizeof(rt::FlatPerlin) <= 52 * 1024) {
        p.perlin_lds = (uint32_t)n_p;
        wl += n_p * sizeof(rt::FlatPerlin);
      }
      const size_t mt = u.n_materials * sizeof(rt::FlatMaterial) + u.n_textures * sizeof(rt::FlatTexture);
      if (u.n_materials != 0 && u.n_textures != 0 && u.n_materials <= 64 && u.n_textures <= 64 && sw.mat_lds &&
          wl + mt <= 52 * 1024) {
        p.mat_lds = (uint32_t)u.n_materials;
        p.tex_lds = (uint32_t)u.n_textures;
        wl += mt;
      }
    }
    int n = 0;
#define WORLD_OCC(I, FEAT) if ((n = occupancy(wd ? k_trace_world<FEAT, true, WORLD_WPS> : k_trace_world<FEAT, false, WORLD_WPS>, wl)) > 0) p.blocks_per_cu[I][wd] = n
    WORLD_OCC(0, P_BOOK2); WORLD_OCC(1, P_ANY); WORLD_OCC(2, P_ALL); WORLD_OCC(3, P_NO_SPHERE_MEDIA);
#undef WORLD_OCC
    if (wd == 0 && (n = occupancy(k_trace_world<P_INST, false, WORLD_WPS>, wl)) > 0) p.blocks_per_cu[4][0] = n;
  }
}
static rtx_status plan_world(DeviceScene* ds, const FlatScene& fs) {
  const rtx_status st = upload_array(ds, build_world_desc(fs), &ds->world.desc);
  if (st != RTX_OK) return st;
  ds->upd.n_perlins = fs.perlins.size(); ds->upd.n_materials = fs.materials.size(); ds->upd.n_textures = fs.textures.size();
  plan_world_stacks(ds);
  return RTX_OK;
}

static rtx_status launch_world(DeviceScene* ds, const PassArgs& a) {
  const WorldPlan& p = ds->world;
  const bool wide = ds->wide.nodes4 != nullptr;
  const bool book2 = (a.feat & ~P_BOOK2) == 0;
  const bool has_gravity = (a.feat & rt::F_GRAVITY_SPHERE) != 0;
  const bool no_sphere_media = (a.feat & rt::F_MEDIUM_SPHERE) == 0;
  const uint32_t levels = wide ? (uint32_t)ds->wide.levels : a.stack_levels;
  const size_t lds = stack_bytes(levels) + (size_t)WORLD_SLOT_F64 * TRACE_BLOCK * sizeof(rt::real) +
                     (size_t)p.perlin_lds * sizeof(rt::FlatPerlin) + (size_t)p.mat_lds * sizeof(rt::FlatMaterial) +
                     (size_t)p.tex_lds * sizeof(rt::FlatTexture);
  // the footprint plan_world refused to fit (it skipped the tree: no tables, no occupancy) is not launched either: the per-lane
  // slot behind the stacks leaves this kernel 50 levels where the others have 64
  if (lds > 64 * 1024) { set_error("render: BVH too deep for the LDS traversal stack of k_trace_world (stacks and per-lane slots)"); return RTX_EUNSUPPORTED; }
  const bool inst =(a.feat & rt::F_INSTANCE) != 0;  // (never wide: plan_wide)
  const int family = inst ? 4 : (has_gravity ? 2 : (book2 ? 0 : (no_sphere_media ? 3 : 1)));
  const uint32_t grid = grid_size(a.total, TRACE_BLOCK, (uint64_t)ds->n_cu * (uint64_t)p.blocks_per_cu[family][wide ? 1 : 0]);
  const rt::SceneView& v = ds->view;
#define LAUNCH_WORLD3(FEAT, WIDEF, DIAGF, MAP)                                                                               \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trace_world<FEAT, WIDEF, WORLD_WPS, DIAGF, decltype(MAP)>), dim3(grid), dim3(TRACE_BLOCK), lds, \
                     a.stream, v, a.rp, MAP, a.s_begin, a.total, a.samples, a.work_counter, v.entries, v.top_level, v.spheres, \
                     v.moving_spheres, v.rects, v.triangles, v.materials, v.textures, v.refs, ds->wide.nodes4, p.desc,     \
                     ds->walk.leaf_weight, ds->sw.world_threshold, levels, p.perlin_lds, p.mat_lds, p.tex_lds,             \
                     DIAGF ? ds->ws.diag : nullptr)
#define LAUNCH_WORLD2(FEAT, WIDEF) with_map(a, [&](auto map) { LAUNCH_WORLD3(FEAT, WIDEF, false, map); })
#define LAUNCH_WORLD(FEAT) do { if (wide) { LAUNCH_WORLD2(FEAT, true); } else { LAUNCH_WORLD2(FEAT, false); } } while (0)
  if (ds->sw.kernel == ForcedKernel::world && ds->sw.diag && book2 && wide && !a.active) {  // (uniform passes only)
    unsigned long long h[24];
    static const char* const names[8] = {"node_step", "leaf_step", "sweep", "shade(lean)", "regen", "direct_entry(all)", "direct_entry(run)", "shade(rare)"};
    return run_diag(ds, a.stream, [&] { LAUNCH_WORLD3(P_BOOK2, true, true, a.sm); }, "world_diag", 18, names, 8, h);
  }
  if (inst) {
    if (wide) { set_error("render: a world with an instance tree has no 4-wide tree"); return RTX_EUNSUPPORTED; }
    LAUNCH_WORLD2(P_INST, false);
  }
  else if (has_gravity) { LAUNCH_WORLD(P_ALL); }  // the bouncing-ball scene: the instantiation that carries GravitySphere code
  else if (book2) { LAUNCH_WORLD(P_BOOK2); }
  else if (no_sphere_media) { LAUNCH_WORLD(P_NO_SPHERE_MEDIA); }
  else { LAUNCH_WORLD(P_ANY); }
#undef LAUNCH_WORLD
#undef LAUNCH_WORLD2
#undef LAUNCH_WORLD3
  return RTX_OK;
}

// ------------------------------------------------------------------ k_trace_lds
// Fits one k_trace_lds variant (f->levels, f->dims) into lds_max bytes: with a primary-ray ring of 64, else 48 entries when
// want_ring, else without one.  (A small ring is worse than none: its refills run with that few lanes -- HEAD Book-1, ring of
// 16: 3137 Msamples/s against 3774 without; ring of 32 on the final build of round 3: 4963 against 5196.)
static void fit_lds(LdsFit* f, bool want_ring, uint32_t lds_max) {
  for (uint32_t cap : {64u, 48u, 0u})
    if ((want_ring || cap == 0u) && ldsk_layout(f->levels, cap, f->dims).total <= lds_max) {
      f->ok = true;
      f->ring_cap = cap;
      return;
    }
}

// What k_trace_lds's time-aware variant takes from the VALUES of the time-aware boxes, the one value-dependent fact of a launch
// plan.  slope_mask: the axes along which any record has a slope (core/mover_box.hpp: bit 0 x, 1 y, 2 z).  Slopes along y and
// nowhere else select the instantiation whose node records carry no x / z slopes (the y-only one exists: Book-1 at HEAD); the
// record size enters the LDS layout, so the variant is fitted again.  At upload (plan_lds) and at the first k_trace_lds launch
// after rtx_scene_set_moving_spheres changed the boxes (launch_lds).
static void plan_lds_motion_axis(LdsPlan* p, const TraceSwitches& sw, uint32_t slope_mask) {
  const bool y_only = slope_mask == 2u && sw.motion_axis;
  p->motion_axis = y_only ? 1 : -1;
  p->motion.dims.node_dwords = y_only ? LDSK_MOTION1_NODE_DWORDS : LDSK_MOTION_NODE_DWORDS;
  p->motion.ok = false;
  p->motion.ring_cap = 0;
  if (p->motion_planned && p->plain.ok) fit_lds(&p->motion, sw.ring != 0, p->lds_max);
}

// The plain and time-aware variants for a sphere world of one BVH.  The record dims chosen here must match the
// instantiation launch_lds picks for the scene (UNI: trace_lds.inc).
static rtx_status plan_lds(DeviceScene* ds, const FlatScene& fs, const LeafScan& leaves) {
  const bool single_bvh = fs.top_level.size() == 1 && fs.entries[fs.top_level[0]].kind == rt::ENTRY_BVH;
  if (!single_bvh || (fs.features & ~P_SPHERES) != 0 || fs.nodes32.size() > LDSK_MAX_NODES) return RTX_OK;
  LdsPlan& p = ds->lds;
  const TraceSwitches& sw = ds->sw;
  const uint32_t max_end = leaves.max_end, levels = (uint32_t)fs.max_stack + 1u;
  int lds_max = 0;
  (void)hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ds->device);
  if (lds_max > (int)LDSK_LDS_MAX) lds_max = (int)LDSK_LDS_MAX;
  // primitive records in LDS: one per leaf slot, in slot order (trace_lds.inc) -- spheres, or moving spheres when the scene has any
  p.plain.levels = levels;
  p.plain.dims = {(uint32_t)fs.nodes32.size(), max_end, max_end, 0u, LDSK_NODE_DWORDS, 0u};
  p.mv_common = sw.mv_common && lds_common_interval(fs.moving_spheres.data(), fs.moving_spheres.size(), &p.mv_t0, &p.mv_t1);
  // the record kind follows the instantiation launch_lds picks, not the scene's primitives (lds_variant.inc)
  uint32_t counts[3];
  lds_record_counts(fs.features, P_STATIC_SPHERES, (uint32_t)fs.spheres.size(), max_end, counts);
  p.plain.dims.n_spheres = counts[0]; p.plain.dims.n_moving = counts[1]; p.plain.dims.n_uni = counts[2];
  p.motion.levels = levels;
  p.motion.dims = p.plain.dims;
  p.motion.dims.node_dwords = LDSK_MOTION_NODE_DWORDS;
  if (leaves.max_count <= 4 && max_end <= LDSK_MAX_SLOTS && sw.scene_lds != 0 && lds_max > 0) {
    const bool want_ring = sw.ring != 0;
    fit_lds(&p.plain, want_ring, (uint32_t)lds_max);
    const rt::FlatEntry& be = fs.entries[fs.top_level[0]];
    // the time-aware instantiation: the world's one BVH holds moving spheres and came with an interval
    if (p.plain.ok && !fs.motion32.empty() && (fs.features & rt::F_MOVING_SPHERE) && lds_motion_interval_ok((double)be.f[0], (double)be.f[1]) && sw.motion) {
      p.motion_t0 = (double)be.f[0]; p.motion_t1 = (double)be.f[1];
      p.motion_planned = true;
      p.lds_max = (uint32_t)lds_max;
    }
  }
  // slopes along one axis only?  (a scene whose spheres all move the same way)  The record size and the fit follow.
  plan_lds_motion_axis(&p, sw, rt::motion_slope_mask(fs.motion32.data(), fs.motion32.size()));
  if (p.plain.ok) {
    // the limit is a property of the function, not of this scene: raise it to the device maximum once, so that
    // scenes uploaded earlier (with other LDS sizes) keep launching
    // ... and the kernel addresses its node array absolutely, from LDSK_OFF_NODES = 0: that is where its dynamic LDS block starts as
    // long as it has no static LDS in front of it.  Asked of the code object here, once; an instantiation that ever grows a static
    // __shared__ takes k_trace_lds out of the plan (the other kernels render the scene) instead of reading nodes at the wrong place.
    hipError_t ae = hipSuccess;
    bool static_lds = false;
    hipFuncAttributes fa;
#define LDS_ATTR1(K)                                                                                                   \
  if (ae == hipSuccess) ae = hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max); \
  if (ae == hipSuccess) ae = hipFuncGetAttributes(&fa, (const void*)K);                                                \
  if (ae == hipSuccess && fa.sharedSizeBytes != 0) static_lds = true
#define LDS_ATTR(FEAT, RINGF, MOTIONF) LDS_ATTR1((k_trace_lds<FEAT, RINGF, MOTIONF>)); LDS_ATTR1((k_trace_lds<FEAT, RINGF, MOTIONF, ActiveMap>))
    LDS_ATTR(P_SPHERES, true, 0u); LDS_ATTR(P_SPHERES, false, 0u); LDS_ATTR(P_STATIC_SPHERES, true, 0u); LDS_ATTR(P_STATIC_SPHERES, false, 0u);
    LDS_ATTR(P_SPHERES, true, 1u); LDS_ATTR(P_SPHERES, false, 1u); LDS_ATTR(P_SPHERES, true, 3u); LDS_ATTR(P_SPHERES, false, 3u);
#undef LDS_ATTR
#undef LDS_ATTR1
    if (ae != hipSuccess) { (void)hipGetLastError(); p.plain.ok = false; p.motion.ok = false; }
    if (static_lds) {
      fprintf(stderr, "[rtx] k_trace_lds has static LDS in front of its node array: not used\n");
      p.plain.ok = false; p.motion.ok = false;
    }
  }
  if (sw.scene_lds >= 0) {
    auto bytes = [](const LdsFit& f) { return f.ok ? ldsk_layout(f.levels, f.ring_cap, f.dims).total : 0u; };
    fprintf(stderr, "[rtx] RTX_SCENE_LDS: k_trace_lds %s (ring of %u, %u B of LDS); time-aware boxes %s (ring of %u, %u B)\n",
            p.plain.ok ? "on" : "off", p.plain.ring_cap, ldsk_layout(levels, p.plain.ring_cap, p.plain.dims).total,
            p.motion.ok ? "on" : "off", p.motion.ring_cap, bytes(p.motion));
  }
  return RTX_OK;
}

// *variant: the instantiation launched, as RtxRenderStats.trace_variant reports it (lds_variant.inc).
static rtx_status launch_lds(DeviceScene* ds, const PassArgs& a, const RtxCamera* cam, int32_t* variant) {
#ifndef RTX_F32_TU
  if (ds->mesh.slope_readback.pending()) {
    // rtx_scene_set_moving_spheres* refitted the time-aware boxes since the last launch: ONE host wait for the axes their slopes
    // now run along (the scene's one BVH: plan_lds), and the variant is planned by them as at upload
    const unsigned int* words = nullptr;
    HIP_TRY(ds->mesh.slope_readback.wait(&words));
    plan_lds_motion_axis(&ds->lds, ds->sw, words[0]);
  }
#endif
  const LdsPlan& p = ds->lds;
  // time-aware boxes when the scene has them and every ray's time lies inside the BVH's interval (camera.rs:69: [time1, time2))
  *variant = lds_trace_variant(p.motion.ok, p.motion_t0, p.motion_t1, (double)cam->time1, (double)cam->time2, p.motion_axis, p.mv_common);
  const bool motion = (*variant & LDSV_TIME_BOXES) != 0;
  const LdsFit& f = motion ? p.motion : p.plain;
  const bool ring = f.ring_cap != 0u;
  const rt::real m_t0 = (rt::real)p.motion_t0, m_inv = (rt::real)(1.0 / (p.motion_t1 - p.motion_t0));
  const LdsKernelLayout L = ldsk_layout(f.levels, f.ring_cap, f.dims);
  const uint32_t grid = grid_size(a.total, LDSK_BLOCK, (uint64_t)ds->n_cu);
  const WalkTuning& wk = ds->walk;
  // the tuning word of trace_lds.inc: threshold, "one primitive per leaf", D (off travels as 127: no wave has that many walkers), M
  const uint32_t tuning = ((ring && wk.retire_done) ? wk.retire_walk_threshold : wk.walk_threshold) | (wk.single_leaf ? 0x100u : 0u) |
                          ((wk.retire_done ? wk.retire_done : 127u) << 16) | (wk.retire_min << 24);
#define LAUNCH_LDS2(FEAT, RINGF, MOTIONF)                                                                               \
  with_map(a, [&](auto map) {                                                                                           \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trace_lds<FEAT, RINGF, MOTIONF, decltype(map)>), dim3(grid), dim3(LDSK_BLOCK), L.total, \
                       a.stream, ds->view, a.rp, map, a.s_begin, a.total, a.samples, a.work_counter, wk.leaf_weight, \
                       tuning, ds->sw.chunk, f.ring_cap, f.levels, f.dims,  \
                       m_t0, m_inv, p.mv_common ? 1u : 0u, (rt::real)p.mv_t0, (rt::real)p.mv_t1);                        \
  })
#define LAUNCH_LDS(FEAT, MOTIONF) do { if (ring) { LAUNCH_LDS2(FEAT, true, MOTIONF); } else { LAUNCH_LDS2(FEAT, false, MOTIONF); } } while (0)
  // static spheres without checker textures (the Book-1 final scene): the leaner instantiation
  if (!lds_records_are_moving(a.feat, P_STATIC_SPHERES)) { LAUNCH_LDS(P_STATIC_SPHERES, 0u); }
  else if (*variant & LDSV_ONE_AXIS) { LAUNCH_LDS(P_SPHERES, 3u); }  // slopes along y only (Book-1 at HEAD)
  else if (motion) { LAUNCH_LDS(P_SPHERES, 1u); }
  else { LAUNCH_LDS(P_SPHERES, 0u); }
#undef LAUNCH_LDS
#undef LAUNCH_LDS2
  return RTX_OK;
}

// ------------------------------------------------------------------ k_trace_simple
template <bool COUNT>
static void launch_simple(const DeviceScene* ds, const PassArgs& a) {
  const uint32_t grid = grid_size(a.total, TRACE_BLOCK, (uint64_t)ds->n_cu * 8);
#define LAUNCH_SIMPLE2(FEAT, MAP)                                                                                       \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trace_simple<FEAT, COUNT, decltype(MAP)>), dim3(grid), dim3(TRACE_BLOCK), a.stack_lds, \
                     a.stream, ds->view, a.rp, MAP, a.s_begin, a.total, a.samples, ds->ws.counters)
#define LAUNCH_SIMPLE(FEAT) with_map(a, [&](auto map) { LAUNCH_SIMPLE2(FEAT, map); })
  const bool inst = (a.feat & rt::F_INSTANCE) != 0;
  if constexpr (COUNT) {  // (counting renders are never adaptive)
    if (inst) { LAUNCH_SIMPLE2(P_INST, a.sm); } else { LAUNCH_SIMPLE2(P_ALL, a.sm); }
  } else {
    if (a.preset == 0) { LAUNCH_SIMPLE(P_SPHERES); }
    else if (a.preset == 1) { LAUNCH_SIMPLE(P_MESH); }
    else if (inst) { LAUNCH_SIMPLE(P_INST); }
    else { LAUNCH_SIMPLE(P_ALL); }
  }
#undef LAUNCH_SIMPLE
#undef LAUNCH_SIMPLE2
}

#ifndef RTX_F32_TU
// ------------------------------------------------------------------ k_trace_nee
// Three presets cover every world the default launcher accepts: the dragon room exactly, any world without GravitySpheres, and
// everything.  Persistent: as many blocks as are resident, at most one per TRACE_CHUNK items.
static rtx_status launch_nee(const DeviceScene* ds, const PassArgs& a) {
  const int preset = (a.feat & rt::F_INSTANCE) ? 3 : ((a.feat & ~P_MESH_ROOM) == 0 ? 0 : ((a.feat & rt::F_GRAVITY_SPHERE) ? 2 : 1));
#define LAUNCH_NEE(FEAT, MAP)                                                                                                   \
  do {                                                                                                                          \
    const int nb = occupancy(k_trace_nee<FEAT, decltype(MAP)>, a.stack_lds);                                                    \
    const uint32_t grid = grid_size(a.total, TRACE_CHUNK, (uint64_t)ds->n_cu * (uint64_t)(nb > 0 ? nb : 1) * (TRACE_BLOCK / 64)); \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trace_nee<FEAT, decltype(MAP)>), dim3((grid + TRACE_BLOCK / 64 - 1) / (TRACE_BLOCK / 64)),     \
                       dim3(TRACE_BLOCK), a.stack_lds, a.stream, ds->view, ds->lights, a.rp, MAP, a.s_begin, a.total,     \
                       a.samples, a.work_counter);                                                                              \
  } while (0)
  with_map(a, [&](auto map) {
    if (preset == 0) LAUNCH_NEE(P_MESH_ROOM, map);
    else if (preset == 1) LAUNCH_NEE(P_ANY, map);
    else if (preset == 3) LAUNCH_NEE(P_INST, map);
    else LAUNCH_NEE(P_ALL, map);
  });
#undef LAUNCH_NEE
  return RTX_OK;
}
#endif  // !RTX_F32_TU

// ------------------------------------------------------------------ wavefront integrator
// One pass (a.total (sample, pixel) items) through the wavefront integrator: iterations of generate -> trace -> shade over the P
// path slots until every sample of the pass has been written.  It applies where k_trace_vote does (VotePlan::ok).
static rtx_status wave_pass(DeviceScene* ds, const PassArgs& a) {
  Workspace& ws = ds->ws;
  const hipStream_t stream = a.stream;
  uint32_t P = ds->sw.wf_paths;
  if ((uint64_t)P > (uint64_t)a.total) P = a.total;
  P = (P + WF_SEG - 1u) & ~(WF_SEG - 1u);
  const uint32_t n_seg = P / WF_SEG;
  const size_t R = sizeof(rt::real);
  const size_t bytes = 64 + (size_t)P * (16 + 7 * R + 3 * R + 3 * R + R + 4 + 4 + 4 + 4) + (size_t)n_seg * 8;
  HIP_TRY(ws.wave_mem.grow(bytes, stream));
  if (!ws.wave_host_ctrl) HIP_TRY(hipHostMalloc((void**)&ws.wave_host_ctrl, 4 * sizeof(uint32_t), hipHostMallocDefault));
  WavePool pool;
  {
    unsigned char* m = ws.wave_mem;
    pool.ctrl = (uint32_t*)m; m += 64;
    pool.rng = (unsigned long long*)m; m += (size_t)P * 16;
    pool.ray = (rt::real*)m; m += (size_t)P * 7 * R;
    pool.product = (rt::real*)m; m += (size_t)P * 3 * R;
    pool.output = (rt::real*)m; m += (size_t)P * 3 * R;
    pool.hit_t = (rt::real*)m; m += (size_t)P * R;
    pool.depth = (int32_t*)m; m += (size_t)P * 4;
    pool.g = (uint32_t*)m; m += (size_t)P * 4;
    pool.hit_ref = (uint32_t*)m; m += (size_t)P * 4;
    pool.free_list = (uint32_t*)m; m += (size_t)P * 4;
    pool.n_free = (uint32_t*)m; m += (size_t)n_seg * 4;
    pool.cursor = (uint32_t*)m; m += (size_t)n_seg * 4;
    pool.P = P;
  }
  const int preset = a.preset;
  const bool wide = preset == 1 && ds->wide.nodes4 != nullptr;
  const uint32_t levels = wide ? (uint32_t)ds->wide.levels : a.stack_levels;
  const size_t lds = stack_bytes(levels);
  if (lds > 64 * 1024) { set_error("render: BVH too deep for the LDS traversal stack"); return RTX_EUNSUPPORTED; }
  const bool room = (a.feat & ~P_MESH_ROOM) == 0;
  const int occ = ds->sw.wf_occ;
  const uint32_t leaf_weight = ds->walk.leaf_weight, refill = ds->sw.wf_refill, bvh_pos = (uint32_t)ds->vote.bvh_pos;
  // every combination the launcher can ask for, once: (trace kernel, shade kernel) by preset / tree / occupancy target
#define WF_CASES(X)                                                                                                          \
  if (preset == 0) { X(P_SPHERES, false, 4); }                                                                               \
  else if (!wide) { X(P_MESH, false, 4); }                                                                                   \
  else if (room && occ == 5) { X(P_MESH_ROOM, true, 5); }                                                                    \
  else if (room && occ == 6) { X(P_MESH_ROOM, true, 6); }                                                                    \
  else if (room) { X(P_MESH_ROOM, true, 4); }                                                                                \
  else { X(P_MESH, true, 4); }
  int nb = 0;
  hipError_t oe = hipSuccess;
#define WF_OCC(FEAT, WIDEF, MB) oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_wf_trace<FEAT, WIDEF, MB>, TRACE_BLOCK, lds)
  WF_CASES(WF_OCC)
#undef WF_OCC
  if (oe != hipSuccess || nb <= 0) { (void)hipGetLastError(); nb = 1; }
  const uint32_t tgrid = grid_size(P, TRACE_BLOCK, (uint64_t)ds->n_cu * (uint64_t)nb);
  hipLaunchKernelGGL(k_wf_init, dim3((P + 255u) / 256u), dim3(256), 0, stream, pool);
  uint32_t check_every = ds->sw.wf_check;
  int it = 0;
  for (;; ++it) {
    with_map(a, [&](auto map) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wf_generate<decltype(map)>), dim3(n_seg), dim3(WF_SEG), 0, stream, pool, a.rp, map,
                         a.s_begin, a.total);
    });
    if ((uint32_t)(it + 1) % check_every == 0u) {
      HIP_TRY(hipMemsetAsync(pool.ctrl, 0, 16, stream));
      hipLaunchKernelGGL(k_wf_count, dim3(256), dim3(256), 0, stream, pool);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(ws.wave_host_ctrl, pool.ctrl, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      HIP_TRY(hipStreamSynchronize(stream));
      // no path alive after a generation: every segment's share of the pass is used up and every path has ended
      if (ws.wave_host_ctrl[0] == 0u) break;
      if (ws.wave_host_ctrl[0] < P / 2u) check_every = 2;  // the tail: the pool drains within max_depth iterations
      if (it > 100000000) { set_error("render: wavefront integrator did not converge"); return RTX_EHIP; }
    }
#define WF_LAUNCH(FEAT, WIDEF, MB)                                                                                           \
  do {                                                                                                                       \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wf_trace<FEAT, WIDEF, MB>), dim3(tgrid), dim3(TRACE_BLOCK), lds, stream, ds->view, pool, \
                       leaf_weight, refill, bvh_pos, ds->wide.nodes4, ds->vote.tri_base);                                    \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wf_shade<FEAT>), dim3(n_seg), dim3(WF_SEG), 0, stream, ds->view, pool, a.rp, a.samples, bvh_pos); \
  } while (0)
    WF_CASES(WF_LAUNCH)
#undef WF_LAUNCH
  }
#undef WF_CASES
  if (ds->sw.wf_verbose) fprintf(stderr, "[rtx] wavefront: %u slots, %d iterations, %d blocks per CU (%u stack levels)\n", P, it + 1, nb, levels);
  return RTX_OK;
}

// ------------------------------------------------------------------ walk tuning
// Needs WidePlan and LdsPlan.  A leaf step costs about (primitives per leaf) x 1.3 node steps for spheres: vote weight 1 for
// single-primitive leaves, 3 otherwise (measured on C2 / HEAD / C4).
static void plan_walk(DeviceScene* ds, const LeafScan& leaves) {
  WalkTuning& w = ds->walk;
  const TraceSwitches& sw = ds->sw;
  w.leaf_weight = leaves.max_count <= 1 ? 1u : 3u;
  w.single_leaf = leaves.max_count <= 1;
  // latency-bound wide walks: measured best on the dragon room (639 vs 575 Msamples/s)
  if (ds->wide.nodes4) { w.leaf_weight = 1u; w.walk_threshold = 24u; w.regen_min = 8u; }  // regeneration waits for 8 lanes: 803 -> 824 on C4 (4: 817, 16: 801)
  // k_trace_lds since the ground is asked first and the node step got shorter (round 3): C2 10 / 12 / 14 / 16 / 18 -> 6153 / 6188 /
  // 6185 / 6170 / 6140, HEAD Book-1 3859 / 3850 / 3830 / 3808 / 3750 Msamples/s
  else if (ds->lds.plain.ok) w.walk_threshold = 12u;
  if (sw.regen_min) w.regen_min = sw.regen_min;
  if (sw.leaf_weight) w.leaf_weight = sw.leaf_weight;
  if (!sw.single_leaf) w.single_leaf = false;
  if (sw.walk_threshold) w.walk_threshold = w.retire_walk_threshold = sw.walk_threshold;
  if (sw.retire_done != RETIRE_UNSET) w.retire_done = sw.retire_done;
  if (sw.retire_min != RETIRE_UNSET) w.retire_min = sw.retire_min;
  if (sw.item_group) w.item_group_lds = w.item_group_vote = w.item_group_world = w.item_group_wavefront = w.item_group_simple = sw.item_group;
}

// Pixels per group of the item order of a pass traced by `kernel` (k_trace_nee: the world kernel's).
static uint32_t item_group_of(const WalkTuning& w, int32_t kernel) {
  switch (kernel) {
    case RTX_KERNEL_SIMPLE: return w.item_group_simple;
    case RTX_KERNEL_LDS: return w.item_group_lds;
    case RTX_KERNEL_WAVEFRONT: return w.item_group_wavefront;
    case RTX_KERNEL_VOTE: return w.item_group_vote;
    default: return w.item_group_world;
  }
}

// ------------------------------------------------------------------ render
// The trace kernel of every pass of a render (RtxRenderStats.trace_kernel), in this order of precedence:
static int32_t choose_trace_kernel(const DeviceScene* ds, int preset, bool count) {
  const ForcedKernel k = ds->sw.kernel;
  if (count || k == ForcedKernel::simple) return RTX_KERNEL_SIMPLE;  // the counting kernel
  if (ds->lds.plain.ok && preset == 0 && k == ForcedKernel::none) return RTX_KERNEL_LDS;
  if (ds->vote.ok && preset < 2 && k == ForcedKernel::wavefront) return RTX_KERNEL_WAVEFRONT;
  if (ds->vote.ok && preset < 2 && k != ForcedKernel::world) return RTX_KERNEL_VOTE;
  return RTX_KERNEL_WORLD;
}

// The slice of a frame's samples one call traces (progressive rendering, progressive.inc): the absolute sample indices
// [first, first + count), added onto the sums already in the accumulator when cont != 0, with the per-pixel sum of
// squares kept in sumsq when it is not NULL.  A render without one (range == NULL) is the whole frame from sample 0.
// An adaptive range (active != NULL: the ascending list of the n_active local pixels still active) traces those pixels only;
// they replace the shard's pixels as the items of every pass (pass_items.inc), and it needs cont and sumsq.
// light_sampling: trace with next-event estimation (k_trace_nee) instead of the reference's estimator.
typedef RtxSampleRange SampleRange;  // (f32_bridge.hpp: one struct for both compilations)

// How one render is cut into passes: samples of every pixel per pass, passes two deep or not, bytes of the sample buffer.
struct PassPlan {
  uint32_t spp_pass;
  bool pipeline;
  size_t sample_bytes;
};

// Sizes the passes of a render of spp samples of npix pixels (a radiance query: rays) and grows the workspace for them (accum:
// the caller's accumulator, or NULL for the scene's own).  sample_buffer_bytes: RtxConfig's field, 0 for the default budget.
// serial: the counting / timing entry points, which synchronise per pass.
static rtx_status prepare_workspace(DeviceScene* ds, uint64_t sample_buffer_bytes, uint64_t npix, uint64_t npix_all, uint32_t spp,
                                    bool serial, hipStream_t stream, double** accum, PassPlan* pp) {
  Workspace& ws = ds->ws;
  // Default budget: 24 GiB (of 288 GB: C5 takes 16 passes instead of 67, C3 10 instead of 40), but never more than a third of the
  // HBM that is free right now plus what this handle already holds -- other scene handles, a second frame in flight, torch's caching
  // allocator or a smaller part shrink it, and a frame then takes more passes instead of failing.  An explicit
  // sample_buffer_bytes is taken as given.
  uint64_t budget = sample_buffer_bytes;
  if (budget == 0) {
    budget = 24ull << 30;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      const uint64_t avail = ((uint64_t)free_b + ws.samples.bytes()) / 3;
      if (avail < budget) budget = avail;
    } else {
      (void)hipGetLastError();
    }
    if (budget < ws.samples.bytes()) budget = ws.samples.bytes();  // what is already there can be used
  }
  const uint64_t per_sample_plane = npix * 24ull;
  uint32_t spp_pass = spp;
  // Two passes in flight (render_impl) when the render needs several passes anyway (C5: 16, C3: 10): each pass then gets half of
  // the buffer.  A render that fits one pass stays one launch -- cut in two it gains the overlapped half of its reduction and loses
  // as much to the second launch (C2: 6550 against 6574 Msamples/s; with two FRAMES in flight on top, 6644 against 6722), whereas
  // C5 gains 1.7 %.
  const bool pipeline = ds->sw.pass_pipeline && !serial && ds->sw.kernel != ForcedKernel::simple && per_sample_plane > 0 &&
                        (uint64_t)spp * per_sample_plane > budget && budget / 2 >= per_sample_plane;
  const uint64_t pass_budget = pipeline ? budget / 2 : budget;
  if (per_sample_plane > 0 && (uint64_t)spp_pass * per_sample_plane > pass_budget) {
    spp_pass = (uint32_t)(pass_budget / per_sample_plane);
    if (spp_pass < 1) spp_pass = 1;
  }
  // a pass's (sample, pixel) index space is addressed with 32-bit indices
  while (spp_pass > 1 && (uint64_t)spp_pass * npix >= 0xFFFF0000ull) --spp_pass;
  if ((uint64_t)spp_pass * npix >= 0xFFFF0000ull) { set_error("render: shard too large for one pass"); return RTX_EINVAL; }
  size_t need_samples = (size_t)spp_pass * per_sample_plane * (pipeline ? 2 : 1);
  if (need_samples > ws.samples.bytes()) {
    if (ws.samples) { HIP_TRY(hipStreamSynchronize(stream)); HIP_TRY(ws.samples.release()); }
    // out of memory: halve the pass until the buffer fits (down to one sample per pass) before giving up
    for (;;) {
      hipError_t me = ws.samples.alloc(need_samples);
      if (me == hipSuccess) break;
      (void)hipGetLastError();
      if (me != hipErrorOutOfMemory || spp_pass <= 1) {
        set_error(std::string("render: sample buffer of ") + std::to_string(need_samples) + " bytes: " + hipGetErrorString(me));
        return me == hipErrorOutOfMemory ? RTX_ENOMEM : RTX_EHIP;
      }
      spp_pass = (spp_pass + 1) / 2;
      need_samples = (size_t)spp_pass * per_sample_plane * (pipeline ? 2 : 1);
    }
  }
  if (!*accum) {
    HIP_TRY(ws.accum.grow((size_t)npix_all * 24, stream));
    *accum = ws.accum;
  }
  if (!ws.counters) HIP_TRY(ws.counters.alloc(sizeof(rt::TraceCounters)));
  if (!ws.work_counter) HIP_TRY(ws.work_counter.alloc(2 * sizeof(unsigned int)));
  if (!ws.pass_map) HIP_TRY(ws.pass_map.alloc(2 * sizeof(PassMap)));
  if (pipeline && !ws.aux_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&ws.aux_stream, hipStreamNonBlocking));
    for (int i = 0; i < 3; ++i) HIP_TRY(hipEventCreateWithFlags(&ws.ev_pass[i], hipEventDisableTiming));
  }
  if (!ws.ev[0]) { HIP_TRY(hipEventCreate(&ws.ev[0])); HIP_TRY(hipEventCreate(&ws.ev[1])); }
  *pp = {spp_pass, pipeline, need_samples};
  return RTX_OK;
}

template <bool COUNT>
static rtx_status render_impl(DeviceScene* ds, const RtxCamera* cam, const RtxConfig* cfg,
                              const RtxShard* shard, double* d_accum_out, uint8_t* d_rgb8_out,
                              hipStream_t stream, RtxRenderStats* stats, const SampleRange* range = nullptr) {
  RtxShard sh;
  rtx_status st = validate(ds, cam, cfg, shard, &sh);
  if (st != RTX_OK) return st;
  int cur = -1;
  HIP_TRY(hipGetDevice(&cur));
  if (cur != ds->device) { set_error("render: scene was uploaded to a different device than the current one"); return RTX_EINVAL; }
  if ((ds->view.features & rt::F_GRAVITY_SPHERE) && !(cam->time2 <= ds->gravity_time_limit)) {
    set_error("render: shutter time " + std::to_string(cam->time2) + " is beyond the GravitySpheres' stored trajectory (limit " +
              std::to_string(ds->gravity_time_limit) + " s): get_center's fallback loop (hit.rs:380-390) would run unbounded on the GPU");
    return RTX_EINVAL;
  }

  const rt::RenderParams rp = make_params(cam, cfg);
  const int32_t w = rp.image_width, h = rp.image_height;
  // world.rs:1198-1202: chunk_size = h / threads; rows >= threads * chunk_size are never rendered.
  int32_t row_limit = h;
  if (cfg->row_chunk_compat) row_limit = (h / cfg->threads) * cfg->threads;
  const int rows_all = shard_row_count(h, sh, h);
  const int rows_active = shard_row_count(h, sh, row_limit);
  const uint64_t npix_all = (uint64_t)rows_all * w, npix = (uint64_t)rows_active * w;
  if (npix_all >= (1ull << 31)) { set_error("render: shard larger than 2^31 pixels"); return RTX_EINVAL; }
  if (stats) memset(stats, 0, sizeof(*stats));
  if (npix_all == 0) return RTX_OK;

  const uint32_t s_first = range ? range->first : 0u;
  const uint32_t spp = range ? range->count : (uint32_t)cfg->samples_per_pixel;  // samples of every pixel this call traces
  const bool adaptive = range && range->active;
  if (adaptive && (!range->cont || !range->sumsq || d_rgb8_out || range->n_active > npix)) {
    set_error("render: an adaptive sample range continues S and Q of at most the shard's pixels");
    return RTX_EINVAL;
  }
  const uint64_t nitem = adaptive ? range->n_active : npix;  // pixels of every sample of a pass
  double* accum = d_accum_out;
  PassPlan pp;
  st = prepare_workspace(ds, cfg->sample_buffer_bytes, nitem, npix_all, spp, COUNT || stats != nullptr, stream, &accum, &pp);
  if (st != RTX_OK) return st;
  Workspace& ws = ds->ws;
  if (COUNT) HIP_TRY(hipMemsetAsync(ws.counters, 0, sizeof(rt::TraceCounters), stream));

  // rows skipped by row_chunk_compat stay (0,0,0) as in the reference's Screen::new
  if (npix < npix_all) {
    HIP_TRY(hipMemsetAsync(accum + 3 * npix, 0, (size_t)(npix_all - npix) * 24, stream));
    if (d_rgb8_out) HIP_TRY(hipMemsetAsync(d_rgb8_out + 3 * npix, 0, (size_t)(npix_all - npix) * 3, stream));
    if (range && range->sumsq) HIP_TRY(hipMemsetAsync(range->sumsq + 3 * npix, 0, (size_t)(npix_all - npix) * 24, stream));
  }

  const uint32_t stack_levels = (uint32_t)ds->view.max_stack + 1u;
  if (stack_bytes(stack_levels) > 64 * 1024) { set_error("render: BVH too deep for the LDS traversal stack"); return RTX_EUNSUPPORTED; }
  const uint32_t feat = ds->view.features;
  const int preset = ((feat & ~P_SPHERES) == 0) ? 0 : (((feat & ~P_MESH) == 0) ? 1 : 2);
  const bool nee = range && range->light_sampling;
  if (nee && COUNT) { set_error("render: light sampling has no counting kernel"); return RTX_EUNSUPPORTED; }
#ifdef RTX_F32_TU
  if (nee) { set_error("render: light sampling is f64 only"); return RTX_EUNSUPPORTED; }  // (the *_ex entries reject it first)
#endif
  const int32_t kernel = nee ? (int32_t)RTX_KERNEL_NEE : choose_trace_kernel(ds, preset, COUNT);
  PassArgs a = {rp, {nullptr}, 0u, 0u, (uint32_t)nitem, nullptr, nullptr, stream,
                preset, feat, stack_levels, stack_bytes(stack_levels), adaptive ? range->active : nullptr};

  float trace_ms = 0.f;
  int passes = 0;
  int32_t variant = 0;  // of k_trace_lds (launch_lds); every other kernel has one form
  if (nitem > 0) {
    // Passes two deep: even passes on the caller's stream, odd ones on ws.aux_stream, each with its own half of the sample
    // buffer and its own work counter.  Within a stream: trace(k), reduce(k), trace(k + 2), ... -- so a half is not overwritten
    // before it has been summed; across streams reduce(k) waits for reduce(k - 1) -- so every pixel's samples are still added in
    // ascending order, bit for bit what one stream does.  What overlaps: the last waves of trace(k) (a few long paths in
    // otherwise idle CUs), reduce(k) and the first waves of trace(k + 1).
    if (pp.pipeline) {
      HIP_TRY(hipEventRecord(ws.ev_pass[2], stream));
      HIP_TRY(hipStreamWaitEvent(ws.aux_stream, ws.ev_pass[2], 0));
    }
    for (uint32_t s_off = 0; s_off < spp; s_off += pp.spp_pass, ++passes) {
      const int half = pp.pipeline ? (passes & 1) : 0;
      const uint32_t s_count = spp - s_off < pp.spp_pass ? spp - s_off : pp.spp_pass;
      a.s_begin = s_first + s_off;  // absolute index of the pass's first sample: the key of its random streams
      a.total = (uint32_t)((uint64_t)s_count * nitem);
      a.stream = half ? ws.aux_stream : stream;  // every launch of the pass goes to this stream
      a.samples = ws.samples + (size_t)half * (size_t)pp.spp_pass * (size_t)nitem * 3u;
      a.work_counter = ws.work_counter + half;
      a.sm.pass = ws.pass_map + half;
      if (stats) HIP_TRY(hipEventRecord(ws.ev[0], a.stream));
      const PassMap pm = {rt::make_item_order((uint32_t)nitem, s_count, item_group_of(ds->walk, kernel)), rt::make_div32((uint32_t)w),
                          rt::make_div32((uint32_t)sh.block_rows), (uint32_t)sh.shard_index, (uint32_t)sh.shard_count};
      hipLaunchKernelGGL(k_pass_begin, dim3(1), dim3(64), 0, a.stream, a.work_counter, ws.pass_map + half, pm);
      switch (kernel) {
        case RTX_KERNEL_SIMPLE: launch_simple<COUNT>(ds, a); break;
        case RTX_KERNEL_LDS: st = launch_lds(ds, a, cam, &variant); break;
        case RTX_KERNEL_WAVEFRONT: st = wave_pass(ds, a); break;
        case RTX_KERNEL_VOTE: st = launch_vote(ds, a); break;
#ifndef RTX_F32_TU
        case RTX_KERNEL_NEE: st = launch_nee(ds, a); break;
#endif
        default: st = launch_world(ds, a); break;  // RTX_KERNEL_WORLD
      }
      if (st != RTX_OK) return st;
      HIP_TRY(hipGetLastError());
      if (stats) {
        HIP_TRY(hipEventRecord(ws.ev[1], a.stream));
        HIP_TRY(hipEventSynchronize(ws.ev[1]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]));
        trace_ms += ms;
      }
      uint32_t pgrid = (uint32_t)((nitem + 255) / 256);
      if (pp.pipeline && passes > 0) HIP_TRY(hipStreamWaitEvent(a.stream, ws.ev_pass[1 - half], 0));  // the previous pass's sums are in
      const int first_pass = s_off == 0 && !(range && range->cont) ? 1 : 0;
      if (adaptive)
        hipLaunchKernelGGL(k_reduce_samples_moments_active, dim3(pgrid), dim3(256), 0, a.stream, a.samples, accum, range->sumsq,
                           range->active, (uint32_t)nitem, s_count);
      else if (range && range->sumsq)
        hipLaunchKernelGGL(k_reduce_samples_moments, dim3(pgrid), dim3(256), 0, a.stream, a.samples, accum, range->sumsq,
                           (uint32_t)npix, s_count, first_pass);
      else
        hipLaunchKernelGGL(k_reduce_samples, dim3(pgrid), dim3(256), 0, a.stream, a.samples, accum, (uint32_t)npix, s_count, first_pass);
      HIP_TRY(hipGetLastError());
      if (pp.pipeline) HIP_TRY(hipEventRecord(ws.ev_pass[half], a.stream));
    }
    if (pp.pipeline && passes > 0 && ((passes - 1) & 1)) HIP_TRY(hipStreamWaitEvent(stream, ws.ev_pass[1], 0));
    if (d_rgb8_out) {
      uint32_t pgrid = (uint32_t)((npix + 255) / 256);
      hipLaunchKernelGGL(k_tonemap, dim3(pgrid), dim3(256), 0, stream, accum, d_rgb8_out, (uint32_t)npix, s_first + spp);
      HIP_TRY(hipGetLastError());
    }
  }
  if (stats) {
    HIP_TRY(hipStreamSynchronize(stream));
    stats->trace_ms = trace_ms;
    stats->trace_launches = passes;
    stats->passes = passes;
    stats->trace_kernel = passes > 0 ? kernel : RTX_KERNEL_SIMPLE;  // (nothing traced: no kernel ran)
    stats->trace_variant = variant;
    stats->sample_buffer_bytes = pp.sample_bytes;
    stats->samples = (uint64_t)spp * nitem;  // (pixel, sample) paths this call traced; the work counters below only in count mode
    if (COUNT) {
      rt::TraceCounters c;
      HIP_TRY(hipMemcpy(&c, ws.counters, sizeof(c), hipMemcpyDeviceToHost));
      stats->samples = c.samples; stats->rays = c.rays; stats->box_tests = c.box_tests;
      stats->sphere_tests = c.sphere_tests; stats->moving_sphere_tests = c.moving_sphere_tests;
      stats->rect_tests = c.rect_tests; stats->triangle_tests = c.triangle_tests;
      stats->scatters = c.scatters; stats->texels = c.texels; stats->perlin_calls = c.perlin_calls;
    }
  }
  return RTX_OK;
}

// Tone map of an accumulator holding spp samples per pixel (progressive.inc reads a frame at any sample count) -- or, for an
// adaptive frame (counts not NULL), counts[lp] samples in pixel lp, spp where that is 0 (still active).
static rtx_status tonemap_impl(const double* accum, uint8_t* rgb8, const int32_t* counts, uint32_t npix, uint32_t spp,
                               hipStream_t stream) {
  if (npix == 0) return RTX_OK;
  if (counts) hipLaunchKernelGGL(k_tonemap_counts, dim3((npix + 255) / 256), dim3(256), 0, stream, accum, rgb8, counts, npix, spp);
  else hipLaunchKernelGGL(k_tonemap, dim3((npix + 255) / 256), dim3(256), 0, stream, accum, rgb8, npix, spp);
  HIP_TRY(hipGetLastError());
  return RTX_OK;
}

#include "queries.inc"       // check_walk_launch, with_query_preset, launch_cast_rays, launch_occlusion, trace_rays_impl: the launchers of
                             // the ray queries (here, not beside their kernels: they plan passes with prepare_workspace)

// The feature pass of a whole-image progressive handle (denoise.inc: k_features): feature_spp first hits per pixel into the
// float4 albedo / normal buffers of w * h pixels.  Asynchronous on stream.
static rtx_status features_impl(DeviceScene* ds, const RtxCamera* cam, const RtxConfig* cfg, int32_t feature_spp,
                                float4* d_albedo, float4* d_normal, hipStream_t stream) {
  size_t stack_lds = 0;
  const rtx_status st = check_walk_launch(ds, "features", &stack_lds);
  if (st != RTX_OK) return st;
  if ((ds->view.features & rt::F_GRAVITY_SPHERE) && !(cam->time2 <= ds->gravity_time_limit)) {
    set_error("features: shutter time beyond the GravitySpheres' stored trajectory");
    return RTX_EINVAL;
  }
  const rt::RenderParams rp = make_params(cam, cfg);
  const uint64_t npix = (uint64_t)rp.image_width * (uint64_t)rp.image_height;
  if (npix == 0) return RTX_OK;
  const uint32_t grid = grid_size((uint32_t)npix, TRACE_BLOCK, (uint64_t)ds->n_cu * 8);
  if (ds->view.features & rt::F_INSTANCE)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_features<P_INST>), dim3(grid), dim3(TRACE_BLOCK), stack_lds, stream, ds->view,
                       rp, (uint32_t)npix, (uint32_t)feature_spp, d_albedo, d_normal);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_features<P_ALL>), dim3(grid), dim3(TRACE_BLOCK), stack_lds, stream, ds->view,
                       rp, (uint32_t)npix, (uint32_t)feature_spp, d_albedo, d_normal);
  HIP_TRY(hipGetLastError());
  return RTX_OK;
}

// Upload one flattened scene to the current device and plan the launches of every kernel family for it.
static rtx_status scene_upload_impl(const FlatScene& fs, DeviceScene** out) {
  *out = nullptr;
  DeviceScene* ds = new (std::nothrow) DeviceScene();
  if (!ds) { set_error("out of memory"); return RTX_ENOMEM; }
  hipError_t e = hipGetDevice(&ds->device);
  if (e != hipSuccess) {
    set_error(std::string("hipGetDevice: ") + hipGetErrorString(e) + " (this library has no CPU render path)");
    delete ds;
    return RTX_EHIP;
  }
  rt::SceneView& v = ds->view;
  memset(&v, 0, sizeof(v));
  rtx_status st;
#define UP(field, vec) if ((st = upload_array(ds, fs.vec, &v.field)) != RTX_OK) { free_device_scene(ds); return st; }
  UP(spheres, spheres) UP(moving_spheres, moving_spheres) UP(rects, rects) UP(triangles, triangles)
  UP(nodes, nodes) UP(nodes32, nodes32) UP(motion32, motion32) UP(refs, refs) UP(entries, entries) UP(top_level, top_level)
  UP(materials, materials) UP(textures, textures) UP(perlins, perlins) UP(images, images) UP(texels, texels)
  UP(top_box32, top_box32) UP(gravity_spheres, gravity_spheres) UP(gravity_y, gravity_y)
#ifndef RTX_F32_TU
  {
    // next-event estimation's light table (host/light_table.hpp): a few records and one int per slot, only when there are lights
    const LightTable lt = build_light_table(fs);
    if (!lt.lights.empty()) {
      if ((st = upload_array(ds, lt.lights, &ds->lights.lights)) != RTX_OK || (st = upload_array(ds, lt.slot_light, &ds->lights.slot_light)) != RTX_OK) {
        free_device_scene(ds);
        return st;
      }
      ds->lights.n_lights = (int32_t)lt.lights.size();
      ds->mesh.sphere_is_light.assign(fs.spheres.size(), 0);
      ds->mesh.rect_is_light.assign(fs.rects.size(), 0);
      for (const rt::FlatLight& L : lt.lights) {
        if (L.kind == rt::LIGHT_SPHERE) ds->mesh.sphere_is_light[(size_t)L.prim] = 1;
        else if (L.kind == rt::LIGHT_RECT) ds->mesh.rect_is_light[(size_t)L.prim] = 1;
      }
    }
  }
#endif
#undef UP
  v.n_top_level = (int32_t)fs.top_level.size();
  v.max_stack = fs.max_stack;
  v.features = fs.features;
  v.inst_entries = fs.view().inst_entries;
  // GravitySphere::get_center (hit.rs:369-391) leaves its stored trajectory for a brute-force loop of (time - time0) / 0.001
  // steps, per sphere test, per ray: a shutter far beyond the table is an effectively unbounded kernel.  Renders are limited to
  // RTX_GRAVITY_SLACK_S seconds past the shortest table (10 000 loop steps); rtx_render* return RTX_EINVAL beyond.
  for (const rt::FlatGravitySphere& g : fs.gravity_spheres)
    ds->gravity_time_limit = std::min(ds->gravity_time_limit, (double)g.table_len * 0.001 + 10.0);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, ds->device) == hipSuccess && prop.multiProcessorCount > 0) ds->n_cu = prop.multiProcessorCount;

  // one plan per kernel family; the order is their dependencies: wide tree <- vote, world <- wide, walk <- wide + lds
  ds->sw = read_switches();
  const LeafScan leaves = scan_leaves(fs);
  plan_vote(ds, fs);
  if ((st = plan_wide(ds, fs)) != RTX_OK || (st = plan_world(ds, fs)) != RTX_OK || (st = plan_lds(ds, fs, leaves)) != RTX_OK) {
    free_device_scene(ds);
    return st;
  }
  plan_walk(ds, leaves);
  if ((st = build_scene_update(ds, fs)) != RTX_OK) {
    free_device_scene(ds);
    return st;
  }
  build_scene_shading(ds, fs);
  *out = ds;
  return RTX_OK;
}

static rtx_status scene_trim_impl(DeviceScene* ds) {
  int cur = -1;
  HIP_TRY(hipGetDevice(&cur));
  if (cur != ds->device) { set_error("rtx_scene_trim: scene lives on a different device than the current one"); return RTX_EINVAL; }
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(ds->ws.samples.release());
  HIP_TRY(ds->ws.accum.release());
  return RTX_OK;
}

// This compilation's scene operations (f32_bridge.hpp), over the device scene as a void*.  The counting instantiation
// render_impl<true> is f64 only and stays outside the table.
static const RtxSceneOps scene_ops = {
    [](void* ds, const RtxCamera* cam, const RtxConfig* cfg, const RtxShard* shard, double* d_accum_rgb, uint8_t* d_rgb8,
       hipStream_t stream, RtxRenderStats* stats, const SampleRange* range) {
      return render_impl<false>((DeviceScene*)ds, cam, cfg, shard, d_accum_rgb, d_rgb8, stream, stats, range);
    },
    tonemap_impl,
    [](void* ds, const RtxCamera* cam, const RtxConfig* cfg, int32_t feature_spp, float4* d_albedo, float4* d_normal,
       hipStream_t stream) { return features_impl((DeviceScene*)ds, cam, cfg, feature_spp, d_albedo, d_normal, stream); },
    [](void* ds) { return scene_trim_impl((DeviceScene*)ds); },
    [](void* ds) { free_device_scene((DeviceScene*)ds); },
    [](void* ds, const RtxRayBatch* rays, const RtxRayHits* hits, hipStream_t stream) {
      return launch_cast_rays((DeviceScene*)ds, rays, hits, stream);
    },
    [](void* ds, const RtxRadianceRays* rays, double* d_sum_rgb, double* d_sumsq_rgb, hipStream_t stream, RtxRenderStats* stats) {
      return trace_rays_impl((DeviceScene*)ds, rays, d_sum_rgb, d_sumsq_rgb, stream, stats);
    },
    [](void* ds, const RtxSlotOps* resolved, int64_t n, hipStream_t stream) {
      return scene_set_transforms_impl((DeviceScene*)ds, resolved, n, stream);
    },
    [](void* ds, int32_t which, void* out, size_t bytes) { return scene_read_array_impl((DeviceScene*)ds, which, out, bytes); },
    [](void* ds, const int32_t* trees, int32_t n, hipStream_t stream, RtxRebuildStats* out) {
      return scene_rebuild_impl((DeviceScene*)ds, trees, n, stream, out);
    },
    [](void* ds, int32_t k, double* cost) { return scene_tree_cost_impl((DeviceScene*)ds, k, cost); },
    [](void* ds, const RtxShadingEdit* edits, int64_t n, hipStream_t stream) {
      return scene_set_shading_impl((DeviceScene*)ds, edits, n, stream);
    },
    [](void* ds, const RtxRayBatch* rays, double* d_tau, hipStream_t stream) {
      return launch_occlusion((DeviceScene*)ds, rays, d_tau, stream);
    },
    [](void* ds, const RtxGatherPoints* points, double* d_sum, double* d_sumsq, hipStream_t stream, RtxRenderStats* stats) {
      return gather_impl((DeviceScene*)ds, points, d_sum, d_sumsq, stream, stats);
    },
    [](void* ds, const RtxPointBatch* points, const RtxNearest* out, hipStream_t stream) {
      return launch_nearest((DeviceScene*)ds, points, out, stream);
    },
    [](void* ds) { size_t stack_lds = 0; return check_nearest_launch((DeviceScene*)ds, &stack_lds); },
};

}  // namespace rtx

using namespace rtx;

#ifdef RTX_F32_TU
#include "f32_entry.inc"   // the f32 compilation's side of f32_bridge.hpp
#else
#include "f32_convert.inc" // f64 flat arrays -> the f32 compilation's layouts

// Every render entry point but the counting one funnels through here: the scene handle carries the operations of the
// compilation that owns its device scene.
static rtx_status render_any(const rtx_scene* s, const RtxCamera* cam, const RtxConfig* cfg, const RtxShard* shard,
                             double* d_accum_rgb, uint8_t* d_rgb8, hipStream_t stream, RtxRenderStats* stats,
                             const SampleRange* range = nullptr) {
  if (!s) { set_error("render: NULL scene, camera or config"); return RTX_EINVAL; }
  return s->ops->render(s->device_scene, cam, cfg, shard, d_accum_rgb, d_rgb8, stream, stats, range);
}

extern "C" {

rtx_status rtx_scene_upload(const rtx_flat* f, rtx_scene** out) {
  if (!f || !out) { set_error("rtx_scene_upload: NULL argument"); return RTX_EINVAL; }
  *out = nullptr;
  DeviceScene* ds = nullptr;
  rtx_status st = scene_upload_impl(*flat_of(f), &ds);
  if (st != RTX_OK) return st;
  *out = make_scene_handle(ds, &scene_ops, 0);
  return RTX_OK;
}

rtx_status rtx_scene_upload_f32(const rtx_flat* f, rtx_scene** out) {
  if (!f || !out) { set_error("rtx_scene_upload_f32: NULL argument"); return RTX_EINVAL; }
  *out = nullptr;
  void* ds32 = nullptr;
  rtx_status st = upload_as_f32(*flat_of(f), &ds32);
  if (st != RTX_OK) return st;
  *out = make_scene_handle(ds32, rtx_f32_scene_ops(), 1);
  return RTX_OK;
}

int32_t rtx_scene_is_f32(const rtx_scene* s) { return s && s->f32 ? 1 : 0; }

rtx_status rtx_scene_trim(rtx_scene* s) {
  if (!s) { set_error("rtx_scene_trim: NULL scene"); return RTX_EINVAL; }
  return s->ops->trim(s->device_scene);
}

void rtx_scene_destroy(rtx_scene* s) {
  if (!s) return;
  s->ops->destroy(s->device_scene);
  free_scene_handle(s);
}

rtx_status rtx_render_device(const rtx_scene* s, const RtxCamera* cam, const RtxConfig* cfg,
                             const RtxShard* shard, double* d_accum_rgb, uint8_t* d_rgb8,
                             void* hip_stream, RtxRenderStats* stats) {
  return render_any(s, cam, cfg, shard, d_accum_rgb, d_rgb8, (hipStream_t)hip_stream, stats);
}

// ---- moving objects.  What needs no scene is checked first (abi.cpp: check_set_transforms), then the scene's own compilation
// checks the rest against its shadow of the upload and enqueues (scene_update.inc).
rtx_status rtx_scene_set_transforms(rtx_scene* s, const RtxSlotOps* updates, int64_t n, void* hip_stream) {
  std::vector<RtxSlotOps> resolved;
  const rtx_status st = check_set_transforms("rtx_scene_set_transforms", s, updates, n, &resolved);
  if (st != RTX_OK || n == 0) return st;
  return s->ops->set_transforms(s->device_scene, resolved.data(), n, (hipStream_t)hip_stream);
}

// ---- relighting (shading_update.inc).  What needs no scene is checked first -- the handle is not read before it has passed --
// then the scene's own compilation checks the edits against its shadow of the upload, plans and enqueues.
rtx_status rtx_scene_set_shading(rtx_scene* s, const RtxShadingEdit* edits, int64_t n, void* hip_stream) {
  std::string err;
  if (!check_shading_args("rtx_scene_set_shading", s, edits, n, &err)) { set_error(err); return RTX_EINVAL; }
  if (n == 0) return RTX_OK;
  return s->ops->set_shading(s->device_scene, edits, n, (hipStream_t)hip_stream);
}

// ---- deforming meshes and moving static spheres (mesh_update.inc): one ladder for the four entries.  What needs no scene
// comes first -- the handle is not read before it has passed -- then the checks shared with rtx_flat_set_triangles /
// _set_spheres (host/set_triangles.hpp) against the shadow the scene kept from its upload; nothing is enqueued before every
// check has passed.
static rtx_status scene_set_prims_any(const PrimKind& K, const char* who, rtx_scene* s, const int32_t* ids, int64_t n, const double* values,
                                      bool host_values, void* hip_stream) {
  std::string err;
  if (!check_prim_args(K, who, s, ids, n, values, &err)) { set_error(err); return RTX_EINVAL; }
  if (!host_values && ((uintptr_t)values & 7)) { set_error(std::string(who) + ": " + K.d_arg + " is not 8-byte aligned"); return RTX_EINVAL; }
  if (n == 0) return RTX_OK;
  const bool mov = K.type == rt::PRIM_MOVING_SPHERE;
  // (the movers' entries check every RTX_EINVAL that needs no shadow before the first RTX_EUNSUPPORTED; the ids need the shadow,
  // which only an f64 scene keeps)
  if (mov && host_values && !check_prims_finite(K, who, values, n, &err)) { set_error(err); return RTX_EINVAL; }
  if (s->f32) {
    set_error(std::string(who) + ": needs an f64 scene (rtx_scene_upload): an f32 scene does not hold the f64 " +
              (K.type == rt::PRIM_TRIANGLE
                   ? "vertices of the untouched triangles in touched leaves. Update the flat scene with rtx_flat_set_triangles"
                   : mov ? "records of the untouched primitives in touched leaves. Update the flat scene with rtx_flat_set_moving_spheres"
                   : K.type == rt::PRIM_RECT ? "records of the untouched primitives in touched leaves. Update the flat scene with rtx_flat_set_rects"
                         : "records of the untouched primitives in touched leaves. Update the flat scene with rtx_flat_set_spheres") +
              " and upload it again with rtx_scene_upload_f32");
    return RTX_EUNSUPPORTED;
  }
  if (!check_prim_ids(K, who, scene_device(s)->mesh.shadow, ids, n, &err)) { set_error(err); return RTX_EINVAL; }
  if (!mov && host_values && !check_prims_finite(K, who, values, n, &err)) { set_error(err); return RTX_EINVAL; }
  return scene_set_prims_impl(scene_device(s), K, who, ids, n, values, host_values, (hipStream_t)hip_stream);
}
rtx_status rtx_scene_set_triangles(rtx_scene* s, const int32_t* ids, int64_t n, const double* vertices, void* hip_stream) {
  return scene_set_prims_any(KIND_TRIANGLE, "rtx_scene_set_triangles", s, ids, n, vertices, true, hip_stream);
}
rtx_status rtx_scene_set_triangles_device(rtx_scene* s, const int32_t* ids, int64_t n, const double* d_vertices, void* hip_stream) {
  return scene_set_prims_any(KIND_TRIANGLE, "rtx_scene_set_triangles_device", s, ids, n, d_vertices, false, hip_stream);
}
rtx_status rtx_scene_set_spheres(rtx_scene* s, const int32_t* ids, int64_t n, const double* spheres, void* hip_stream) {
  return scene_set_prims_any(KIND_SPHERE, "rtx_scene_set_spheres", s, ids, n, spheres, true, hip_stream);
}
rtx_status rtx_scene_set_spheres_device(rtx_scene* s, const int32_t* ids, int64_t n, const double* d_spheres, void* hip_stream) {
  return scene_set_prims_any(KIND_SPHERE, "rtx_scene_set_spheres_device", s, ids, n, d_spheres, false, hip_stream);
}
rtx_status rtx_scene_set_moving_spheres(rtx_scene* s, const int32_t* ids, int64_t n, const double* movers, void* hip_stream) {
  return scene_set_prims_any(KIND_MOVING_SPHERE, "rtx_scene_set_moving_spheres", s, ids, n, movers, true, hip_stream);
}
rtx_status rtx_scene_set_moving_spheres_device(rtx_scene* s, const int32_t* ids, int64_t n, const double* d_movers, void* hip_stream) {
  return scene_set_prims_any(KIND_MOVING_SPHERE, "rtx_scene_set_moving_spheres_device", s, ids, n, d_movers, false, hip_stream);
}
rtx_status rtx_scene_set_rects(rtx_scene* s, const int32_t* ids, int64_t n, const double* rects, void* hip_stream) {
  return scene_set_prims_any(KIND_RECT, "rtx_scene_set_rects", s, ids, n, rects, true, hip_stream);
}
rtx_status rtx_scene_set_rects_device(rtx_scene* s, const int32_t* ids, int64_t n, const double* d_rects, void* hip_stream) {
  return scene_set_prims_any(KIND_RECT, "rtx_scene_set_rects_device", s, ids, n, d_rects, false, hip_stream);
}

// ---- instance trees of a resident scene: a new topology for the current pose, and the cost of a tree as it stands
// (scene_rebuild.inc).  What needs no device is checked here; the scene's own compilation checks the rest.
rtx_status rtx_scene_rebuild_instance_trees(rtx_scene* s, const int32_t* trees, int32_t n, void* hip_stream, RtxRebuildStats* out) {
  const char* who = "rtx_scene_rebuild_instance_trees";
  if (!s) { set_error(std::string(who) + ": the scene is NULL"); return RTX_EINVAL; }
  if (n < 0) { set_error(std::string(who) + ": n < 0"); return RTX_EINVAL; }
  if (out)
    for (int i = 0; i < 4; ++i)
      if (out->reserved[i] != 0) { set_error(std::string(who) + ": out->reserved[" + std::to_string(i) + "] is not 0"); return RTX_EINVAL; }
  return s->ops->rebuild_instance_trees(s->device_scene, trees, n, (hipStream_t)hip_stream, out);
}

rtx_status rtx_scene_instance_tree_cost(const rtx_scene* s, int32_t k, double* cost) {
  if (!s || !cost) { set_error("rtx_scene_instance_tree_cost: NULL argument"); return RTX_EINVAL; }
  return s->ops->instance_tree_cost(s->device_scene, k, cost);
}

rtx_status rtx_device_scene_array(const rtx_scene* s, int32_t which, void* out, size_t bytes) {
  if (!s) { set_error("rtx_device_scene_array: NULL scene"); return RTX_EINVAL; }
  return s->ops->read_array(s->device_scene, which, out, bytes);
}

rtx_status rtx_render_count(const rtx_scene* s, const RtxCamera* cam, const RtxConfig* cfg,
                            const RtxShard* shard, RtxRenderStats* stats) {
  if (!stats) { set_error("rtx_render_count: stats is NULL"); return RTX_EINVAL; }
  if (!s) { set_error("render: NULL scene, camera or config"); return RTX_EINVAL; }
  if (s->f32) { set_error("rtx_render_count: the work counters belong to the f64 path (upload the scene with rtx_scene_upload)"); return RTX_EUNSUPPORTED; }
  return render_impl<true>(scene_device(s), cam, cfg, shard, nullptr, nullptr, (hipStream_t) nullptr, stats);
}

rtx_status rtx_device_math(int32_t fn, const double* x, const double* y, int64_t n, double* out) {
  if (!x || !y || !out || n < 0) { set_error("rtx_device_math: bad argument"); return RTX_EINVAL; }
  if (n == 0) return RTX_OK;
  DeviceBuffer<double> dx, dy, dout;
  HIP_TRY(dx.upload(x, (size_t)n));
  HIP_TRY(dy.upload(y, (size_t)n));
  HIP_TRY(dout.alloc((size_t)n * sizeof(double)));
  if (fn >= 32) HIP_TRY(rtx_f32_device_math((int)fn, dx, dy, (long long)n, dout));  // the float entries: the f32 compilation's
  else hipLaunchKernelGGL(k_device_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (int)fn, dx, dy, (long long)n, dout);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, dout, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return RTX_OK;
}

rtx_status rtx_device_cull_verdicts(int32_t f32, int64_t n, const double* box, const double* ray, float* ray32, float* key, uint32_t* verdict) {
  if (f32 != 0 && f32 != 1) { set_error("rtx_device_cull_verdicts: f32 must be 0 or 1"); return RTX_EINVAL; }
  return f32 ? rtx_f32_cull_verdicts(n, box, ray, ray32, key, verdict) : cull_verdicts_impl(n, box, ray, ray32, key, verdict);
}

rtx_status rtx_device_walk_steps(int32_t f32, int32_t kind, int32_t bottom, const void* nodes, int64_t n_nodes, int32_t levels, int64_t n,
                                 const RtxWalkStepItem* items, int32_t* out) {
  if (f32 != 0 && f32 != 1) { set_error("rtx_device_walk_steps: f32 must be 0 or 1"); return RTX_EINVAL; }
  return f32 ? rtx_f32_walk_steps(kind, bottom, nodes, n_nodes, levels, n, items, out)
             : walk_steps_impl(kind, bottom, nodes, n_nodes, levels, n, items, out);
}

rtx_status rtx_device_stream(uint64_t seed, uint64_t pixel, uint32_t sample, int32_t n, double* out) {
  if (!out || n < 0) { set_error("rtx_device_stream: bad argument"); return RTX_EINVAL; }
  if (n == 0) return RTX_OK;
  DeviceBuffer<double> d;
  HIP_TRY(d.alloc((size_t)n * sizeof(double)));
  hipLaunchKernelGGL(k_device_stream, dim3(1), dim3(64), 0, 0, (unsigned long long)seed, (unsigned long long)pixel, (unsigned int)sample, (int)n, d);
  HIP_TRY(hipMemcpy(out, d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  return RTX_OK;
}

// One frame through host memory (rtx_render, rtx_render_ex; who: the entry point's name): allocates the device frame, renders
// it, waits for it and copies back what `out` asks for.
static rtx_status render_frame(const char* who, const rtx_scene* s, const RtxCamera* cam, const RtxConfig* cfg,
                               bool light_sampling, RtxFrame* out, RtxRenderStats* stats) {
  RtxShard sh;
  rtx_status st = validate(s, cam, cfg, nullptr, &sh);
  if (st != RTX_OK) return st;
  size_t npix = (size_t)cfg->image_width * (size_t)rtx_image_height(cfg);
  DeviceBuffer<double> d_accum;
  DeviceBuffer<uint8_t> d_rgb;
  if (d_accum.alloc(npix * 24) != hipSuccess || d_rgb.alloc(npix * 3) != hipSuccess) {
    set_error(std::string(who) + ": hipMalloc of the frame failed");
    return RTX_EHIP;
  }
  // light sampling: the whole frame as one sample range from sample 0 -- the passes, sums and tone map of a one-shot render
  const SampleRange range = {0u, (uint32_t)cfg->samples_per_pixel, 0, nullptr, nullptr, 0u, true};
  st = render_any(s, cam, cfg, nullptr, d_accum, d_rgb, (hipStream_t) nullptr, stats, light_sampling ? &range : nullptr);
  if (st != RTX_OK) return st;
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess && out->accum_rgb) e = hipMemcpy(out->accum_rgb, d_accum, npix * 24, hipMemcpyDeviceToHost);
  if (e == hipSuccess && out->rgb8) e = hipMemcpy(out->rgb8, d_rgb, npix * 3, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { set_error(std::string(who) + ": " + hipGetErrorString(e)); return RTX_EHIP; }
  return RTX_OK;
}

rtx_status rtx_render(const rtx_scene* s, const RtxCamera* cam, const RtxConfig* cfg, RtxFrame* out) {
  if (!out) { set_error("rtx_render: NULL frame"); return RTX_EINVAL; }
  return render_frame("rtx_render", s, cam, cfg, false, out, nullptr);
}

// Argument checks of the *_ex entry points, before any device call.
static rtx_status check_integrator_options(const rtx_scene* s, const RtxIntegratorOptions* opt, const char* who, bool* light_sampling) {
  *light_sampling = false;
  if (!opt) return RTX_OK;
  if (opt->light_sampling != 0 && opt->light_sampling != 1) {
    set_error(std::string(who) + ": light_sampling must be 0 or 1");
    return RTX_EINVAL;
  }
  if (opt->reserved[0] || opt->reserved[1] || opt->reserved[2]) {
    set_error(std::string(who) + ": RtxIntegratorOptions.reserved must be 0");
    return RTX_EINVAL;
  }
  if (opt->light_sampling && s && s->f32) {
    set_error(std::string(who) + ": light sampling is f64 only (upload the scene with rtx_scene_upload)");
    return RTX_EUNSUPPORTED;
  }
  *light_sampling = opt->light_sampling == 1;
  return RTX_OK;
}

rtx_status rtx_render_ex(const rtx_scene* s, const RtxCamera* cam, const RtxConfig* cfg, const RtxIntegratorOptions* opt,
                         RtxFrame* out, RtxRenderStats* stats) {
  if (!out) { set_error("rtx_render_ex: NULL frame"); return RTX_EINVAL; }
  bool nee = false;
  rtx_status st = check_integrator_options(s, opt, "rtx_render_ex", &nee);
  if (st != RTX_OK) return st;
  return render_frame("rtx_render_ex", s, cam, cfg, nee, out, stats);
}

}  // extern "C"

// render_scene_with_time (world.rs:1249-1330): one frame of the video experiment on a scene that stays resident.
extern "C" rtx_status rtx_render_scene_with_time(const rtx_scene* s, double t0, double t1, const char* path,
                                                 int32_t row_chunk_compat, const RtxConfig* overrides) {
  using namespace rtx;
  if (!s || !path) { set_error("rtx_render_scene_with_time: NULL argument"); return RTX_EINVAL; }
  // world.rs:1252-1275: everything about the frame is a constant there
  const double lookfrom[3] = {13, 2, 3}, lookat[3] = {0, 0, 0}, vup[3] = {0, 1, 0};
  RtxCamera cam;
  rtx_status st = rtx_camera_new(lookfrom, lookat, vup, 20.0, 1.0, 0.1, 10.0, t0, t1, &cam);
  if (st != RTX_OK) return st;  // t0 >= t1: gen_range(t0..t1) panics in the reference
  RtxConfig cfg;
  st = rtx_config_new(1.0, 500, 500, 50, 11, &cfg);  // THREADS = 11 (world.rs:18)
  if (st != RTX_OK) return st;
  cfg.background[0] = 0.7; cfg.background[1] = 0.8; cfg.background[2] = 1.0;
  cfg.row_chunk_compat = row_chunk_compat ? 1 : 0;
  if (overrides) {
    if (overrides->image_width > 0) cfg.image_width = overrides->image_width;
    if (overrides->samples_per_pixel > 0) cfg.samples_per_pixel = overrides->samples_per_pixel;
    if (overrides->max_depth > 0) cfg.max_depth = overrides->max_depth;
    cfg.seed = overrides->seed;
    cfg.sample_buffer_bytes = overrides->sample_buffer_bytes;
  }
  const size_t npix = (size_t)cfg.image_width * (size_t)rtx_image_height(&cfg);
  std::vector<uint8_t> rgb(npix * 3);
  RtxFrame frame = {nullptr, rgb.data()};
  st = rtx_render(s, &cam, &cfg, &frame);
  if (st != RTX_OK) return st;
  return rtx_write_ppm(path, cfg.image_width, rtx_image_height(&cfg), rgb.data());  // screen.write_to_ppm_file(path)
}

#include "query_entries.inc"  // rtx_scene_cast_rays*, rtx_scene_occlusion*, rtx_scene_trace_rays*: the entry points of the ray queries
#include "multi.inc"  // rtx_multi_*: one process, several GPUs, one RCCL gather
#include "progressive.inc"  // rtx_progressive_*: a frame accumulated over several calls, with its noise estimate
#endif  // !RTX_F32_TU
