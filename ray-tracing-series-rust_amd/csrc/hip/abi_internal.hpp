// Glue shared by abi.cpp (host-only entry points) and render.hip (device entry points).
#pragma once
#include <string>
#include <vector>
#include "../../../include/rtx_abi.h"
#include "../host/flat_scene.hpp"
#include "../host/scene_graph.hpp"

struct rtx_builder {
  rtx::SceneGraph graph;
  explicit rtx_builder(uint64_t seed) : graph(seed) {}
};
struct rtx_flat {
  rtx::FlatScene scene;
  rtx::BuildOptions options;  // what rtx_flatten built it with: RTX_REBUILD_SAH builds with the same
};
struct RtxSceneOps;  // f32_bridge.hpp
struct rtx_scene {
  void* device_scene;  // rtx::DeviceScene of render.hip, or (f32 != 0) the device scene of its f32 compilation render_f32.hip
  const RtxSceneOps* ops;  // what the compilation that owns device_scene does with it: every call on the scene goes through here
  int32_t f32;  // what rtx_scene_is_f32 answers and the argument checks that reject a precision test; never chooses a callee
};

namespace rtx {

struct DeviceScene;

void set_error(const std::string& msg);

inline const FlatScene* flat_of(const rtx_flat* f) { return &f->scene; }
inline DeviceScene* scene_device(const rtx_scene* s) { return (DeviceScene*)s->device_scene; }
inline rtx_scene* make_scene_handle(void* ds, const RtxSceneOps* ops, int32_t f32) {
  rtx_scene* s = new rtx_scene;
  s->device_scene = ds;
  s->ops = ops;
  s->f32 = f32;
  return s;
}
inline void free_scene_handle(rtx_scene* s) { delete s; }

// The argument checks of the ray queries' entry points (abi.cpp; no device call): RTX_EINVAL with a message that names the entry
// point `who` and the offending field.  rtx_scene_cast_rays* and rtx_scene_occlusion* (out, out_name: hits as "hits", tau as "tau"):
rtx_status check_ray_batch(const char* who, const rtx_scene* s, const RtxRayBatch* rays, const void* out, const char* out_name);
// rtx_scene_trace_rays*: the same first rungs, then the radiance batch's own fields.
rtx_status check_trace_rays(const char* who, const rtx_scene* s, const RtxRadianceRays* rays, const double* sum_rgb);
// rtx_scene_gather*: the gather batch's fields.
rtx_status check_gather(const char* who, const rtx_scene* s, const RtxGatherPoints* points, const double* sum);
// rtx_scene_nearest*: the point batch's fields.
rtx_status check_point_batch(const char* who, const rtx_scene* s, const RtxPointBatch* points, const RtxNearest* out);
// The checks of rtx_scene_set_transforms that need no scene (host/set_transforms.hpp: check_slot_ops_shape; s is compared with
// NULL and not read), then *resolved = the updates with every angle turned into sin / cos as the flat arrays hold them.
rtx_status check_set_transforms(const char* who, const rtx_scene* s, const RtxSlotOps* updates, int64_t n, std::vector<RtxSlotOps>* resolved);

}  // namespace rtx
