// The f32 compilation's side of f32_bridge.hpp (included by render.hip when RTX_F32_TU is defined).
namespace rtx {
void set_error(const std::string& msg) { rtx_f32_set_error(msg.c_str()); }

template <class T>
static bool take_blob(const RtxF32Blobs& b, int which, std::vector<T>* out) {
  if (b.bytes[which] == 0) { out->clear(); return true; }
  if (b.elem_bytes[which] != sizeof(T) || b.bytes[which] % sizeof(T) != 0) return false;
  out->resize(b.bytes[which] / sizeof(T));
  memcpy((void*)out->data(), b.data[which], b.bytes[which]);
  return true;
}
}  // namespace rtx

rtx_status rtx_f32_upload(const RtxF32Blobs* b, void** device_scene) {
  *device_scene = nullptr;
  FlatScene fs;
  bool ok = take_blob(*b, RTX32_SPHERES, &fs.spheres) && take_blob(*b, RTX32_MOVING_SPHERES, &fs.moving_spheres) &&
            take_blob(*b, RTX32_RECTS, &fs.rects) && take_blob(*b, RTX32_TRIANGLES, &fs.triangles) &&
            take_blob(*b, RTX32_NODES, &fs.nodes) && take_blob(*b, RTX32_NODES32, &fs.nodes32) &&
            take_blob(*b, RTX32_REFS, &fs.refs) && take_blob(*b, RTX32_ENTRIES, &fs.entries) &&
            take_blob(*b, RTX32_TOP_LEVEL, &fs.top_level) && take_blob(*b, RTX32_MATERIALS, &fs.materials) &&
            take_blob(*b, RTX32_TEXTURES, &fs.textures) && take_blob(*b, RTX32_PERLINS, &fs.perlins) &&
            take_blob(*b, RTX32_IMAGES, &fs.images) && take_blob(*b, RTX32_TEXELS, &fs.texels) &&
            take_blob(*b, RTX32_TOP_BOX32, &fs.top_box32) && take_blob(*b, RTX32_GRAVITY_SPHERES, &fs.gravity_spheres) &&
            take_blob(*b, RTX32_GRAVITY_Y, &fs.gravity_y) && take_blob(*b, RTX32_MOTION32, &fs.motion32) &&
            take_blob(*b, RTX32_MEMBER_LOCAL_BOX, &fs.member_local_box) && take_blob(*b, RTX32_SLOT_OPS64, &fs.slot_ops64);
  if (!ok) { set_error("rtx_scene_upload_f32: the f32 layout table of f32_layout.hpp disagrees with the compiled structs"); return RTX_EINVAL; }
  fs.max_stack = b->max_stack;
  fs.n_bvh = b->n_bvh;
  fs.features = b->features;
  DeviceScene* ds = nullptr;
  rtx_status st = scene_upload_impl(fs, &ds);
  if (st != RTX_OK) return st;
  *device_scene = ds;
  return RTX_OK;
}

const RtxSceneOps* rtx_f32_scene_ops() { return &scene_ops; }

hipError_t rtx_f32_device_math(int fn, const double* d_x, const double* d_y, long long n, double* d_out) {
  hipLaunchKernelGGL(k_device_math_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, d_x, d_y, n, d_out);
  return hipGetLastError();
}

void rtx_f32_gather_directions(const RtxGatherPoints* points, double* dir) { gather_directions_impl(points, dir); }

rtx_status rtx_f32_cull_verdicts(int64_t n, const double* box, const double* ray, float* ray32, float* key, uint32_t* verdict) {
  return cull_verdicts_impl(n, box, ray, ray32, key, verdict);
}

rtx_status rtx_f32_walk_steps(int32_t kind, int32_t bottom, const void* nodes, int64_t n_nodes, int32_t levels, int64_t n,
                              const RtxWalkStepItem* items, int32_t* out) {
  return walk_steps_impl(kind, bottom, nodes, n_nodes, levels, n, items, out);
}
