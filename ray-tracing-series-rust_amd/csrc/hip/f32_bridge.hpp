// The seam between the two compilations of the device path.
//
// render.hip is compiled twice: as itself (arithmetic type rt::real = double: the bit-exact path every parity test
// checks) and through render_f32.hip (rt::real = float, namespaces renamed to rt32 / rtx32: the statistical fast mode of
// SURVEY.md 8f-4).  The f64 compilation owns the C ABI and its handle types; it hands the f32 compilation byte images of
// the flat arrays already converted to the f32 layouts (host/f32_layout.hpp) and gets back a device scene with the table of
// operations on it.  Each compilation fills one RtxSceneOps from the same lines of render.hip; a scene handle carries its
// table, so the entry points call s->ops->X(s->device_scene, ...) and never ask which precision a scene has.
// Nothing here mentions a type of either namespace, so both compilations see the same declarations.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "../../../include/rtx_abi.h"
#include "../host/f32_blobs.hpp"  // RtxF32Array, RtxF32Blobs: the converted flat arrays as they cross the seam

// A range of the samples of a render (render.hip knows it as SampleRange and says what the fields mean).
struct RtxSampleRange {
  uint32_t first, count;
  int cont;
  double* sumsq;
  const uint32_t* active;
  uint32_t n_active;
  bool light_sampling;
};

// What the entry points do with an uploaded scene, whichever compilation owns it.  Every call is asynchronous on stream.
struct RtxSceneOps {
  // render_impl<false>: the whole frame (range NULL: sums into d_accum_rgb, tone map into d_rgb8 unless NULL) or a sample range
  rtx_status (*render)(void* device_scene, const RtxCamera* cam, const RtxConfig* cfg, const RtxShard* shard, double* d_accum_rgb,
                       uint8_t* d_rgb8, hipStream_t stream, RtxRenderStats* stats, const RtxSampleRange* range);
  // tone map of an accumulator of spp samples per pixel, or (d_counts not NULL) of d_counts[lp] samples, spp where that is 0
  rtx_status (*tonemap)(const double* d_accum_rgb, uint8_t* d_rgb8, const int32_t* d_counts, uint32_t npix, uint32_t spp,
                        hipStream_t stream);
  // the feature pass (denoise.inc: k_features) of feature_spp first hits per pixel of the whole image
  rtx_status (*features)(void* device_scene, const RtxCamera* cam, const RtxConfig* cfg, int32_t feature_spp, float4* d_albedo,
                         float4* d_normal, hipStream_t stream);
  rtx_status (*trim)(void* device_scene);
  void (*destroy)(void* device_scene);
  // ray queries (cast_rays.inc: k_cast_rays): device pointers in both structs, arguments already checked
  rtx_status (*cast_rays)(void* device_scene, const RtxRayBatch* rays, const RtxRayHits* hits, hipStream_t stream);
  // radiance queries (trace_rays.inc: k_trace_rays): device pointers, arguments already checked; stats may be NULL, non-NULL
  // synchronises.  Uses the scene's render workspace.
  rtx_status (*trace_rays)(void* device_scene, const RtxRadianceRays* rays, double* d_sum_rgb, double* d_sumsq_rgb,
                           hipStream_t stream, RtxRenderStats* stats);
  // rtx_scene_set_transforms (scene_update.inc): n > 0 updates in host memory, already through the checks that need no scene
  // and RESOLVED (a rotate_y holds v[0] = sin, v[1] = cos); checks the rest against the scene, then enqueues
  rtx_status (*set_transforms)(void* device_scene, const RtxSlotOps* resolved, int64_t n, hipStream_t stream);
  // rtx_device_scene_array: one resident array copied to the host (blocking)
  rtx_status (*read_array)(void* device_scene, int32_t which, void* out, size_t bytes);
  // rtx_scene_rebuild_instance_trees (scene_rebuild.inc): the list already checked for NULL / n < 0 / reserved words; blocks once
  rtx_status (*rebuild_instance_trees)(void* device_scene, const int32_t* trees, int32_t n, hipStream_t stream, RtxRebuildStats* out);
  // rtx_scene_instance_tree_cost (blocking)
  rtx_status (*instance_tree_cost)(void* device_scene, int32_t k, double* cost);
  // rtx_scene_set_shading (shading_update.inc): n > 0 edits in host memory, already through the checks that need no scene; checks
  // the rest against the scene's shadow, then enqueues
  rtx_status (*set_shading)(void* device_scene, const RtxShadingEdit* edits, int64_t n, hipStream_t stream);
  // occlusion queries (occlusion.inc: k_occlusion): device pointers, arguments already checked
  rtx_status (*occlusion)(void* device_scene, const RtxRayBatch* rays, double* d_tau, hipStream_t stream);
  // gather queries (gather.inc: k_gather, k_reduce_samples_sh): device pointers, arguments already checked; stats may be NULL,
  // non-NULL synchronises.  Uses the scene's render workspace.
  rtx_status (*gather)(void* device_scene, const RtxGatherPoints* points, double* d_sum, double* d_sumsq, hipStream_t stream,
                       RtxRenderStats* stats);
  // nearest-point queries (nearest.inc: k_nearest): device pointers in both structs, arguments already checked
  rtx_status (*nearest)(void* device_scene, const RtxPointBatch* points, const RtxNearest* out, hipStream_t stream);
  // what nearest refuses whatever the batch (a scene with GravitySpheres, a BVH too deep for the LDS stack): asked by the host
  // entry before it stages anything
  rtx_status (*nearest_supported)(void* device_scene);
};

// A stable radix sort of (64-bit key, 32-bit value) pairs on `stream` (lbvh.hip, which already carries rocPRIM's sort: neither
// compilation of render.hip instantiates it).  temp == NULL: *temp_bytes = the temporary storage n pairs need.
hipError_t rtx_sort_pairs_u64_u32(void* temp, size_t* temp_bytes, const unsigned long long* keys_in, unsigned long long* keys_out,
                                  const uint32_t* vals_in, uint32_t* vals_out, int n, hipStream_t stream);
rtx_status rtx_f32_upload(const RtxF32Blobs* blobs, void** device_scene);
const RtxSceneOps* rtx_f32_scene_ops();  // the f32 compilation's table, for the scenes rtx_f32_upload makes
void rtx_f32_set_error(const char* msg);  // defined by the f64 compilation: both report through rtx_last_error
// rtx_device_math's float entries (fn >= 32): one arithmetic building block as the f32 compilation evaluates it
// (post_kernels.inc: k_device_math_f32); device pointers, asynchronous on the null stream.
hipError_t rtx_f32_device_math(int fn, const double* d_x, const double* d_y, long long n, double* d_out);
// rtx_gather_directions with f32 = 1 (gather.inc: gather_directions_impl as the f32 compilation has it); host only
void rtx_f32_gather_directions(const RtxGatherPoints* points, double* dir);
// rtx_device_cull_verdicts / rtx_device_walk_steps with f32 = 1 (cull_hooks.inc as the f32 compilation has it); host pointers
rtx_status rtx_f32_cull_verdicts(int64_t n, const double* box, const double* ray, float* ray32, float* key, uint32_t* verdict);
rtx_status rtx_f32_walk_steps(int32_t kind, int32_t bottom, const void* nodes, int64_t n_nodes, int32_t levels, int64_t n,
                              const RtxWalkStepItem* items, int32_t* out);
