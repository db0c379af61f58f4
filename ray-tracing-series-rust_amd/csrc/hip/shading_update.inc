// rtx_scene_set_shading on a resident scene (included by render.hip, namespace rtx; compiled by both compilations).
//
// New shading parameters reach these device arrays and no other:
//   textures                  a SolidColor's colour, a Noise's scale
//   materials                 the copy of a SolidColor's colour in every Lambertian / DiffuseLight / Isotropic that names it; a
//                             Metal's albedo and fuzz; a Dielectric's ir and the three constants derived from it
//   entries / WorldDesc       a medium's -1 / density, and k_trace_world's copy of it
//   the light table (f64)     after a texture edit: every light's pick weight, cdf and pmf (mesh_update.inc: k_refresh_lights,
//                             unchanged -- the recomputation rtx_scene_set_spheres runs, by the function that built the table:
//                             host/light_table.hpp.  It reads the new colours from `textures`; when no light's colour changed
//                             it stores the bytes that were there)
// so that the arrays equal those of the host-edited flat scene uploaded afresh -- the judge of tests/test_gpu_set_shading.py.
// Nothing else caches a shading value: k_trace_lds reads materials from global memory, k_trace_vote and k_trace_world copy
// their tables into LDS at every launch, and features, needs_uv, the launch plans and sphere_is_light depend on kinds, which
// an edit never alters.  No trace kernel, no SceneView field and no launch plan changes.
//
// The values are computed on the host in f64 by core/shading_edit.hpp and a record is applied by that header's
// shading_write_apply, the function the flat scene's edit runs; an f32 scene narrows with the (float) cast in it.
// No index is derived from a value: every index comes from the plan (host/set_shading.hpp), which was checked against the
// shadow the scene kept from its upload.  No two threads write the same bytes: an edit's targets are unique and so are the
// copies derived from them (a material names one texture), so nothing beyond the kernel boundary needs stating.

// One thread per write record.
__global__ __launch_bounds__(256) void k_set_shading(const rt::ShadingWrite* __restrict__ rec, int n, rt::FlatMaterial* __restrict__ materials,
                                                    rt::FlatTexture* __restrict__ textures, rt::FlatEntry* __restrict__ entries,
                                                    WorldDesc* __restrict__ desc) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  rt::shading_write_apply(rec[i], materials, textures, entries, desc);
}

// ------------------------------------------------------------------ host side
// What an edit is checked against, built once at upload (scene_upload_impl).
static void build_scene_shading(DeviceScene* ds, const FlatScene& fs) { ds->upd.shading = build_shading_shadow(fs); }

// edits (host memory) have passed check_shading_args.  Every check comes first; then one copy, k_set_shading and, on an f64
// scene with a light table after a texture edit, k_refresh_lights, all on `stream`.
static rtx_status scene_set_shading_impl(DeviceScene* ds, const RtxShadingEdit* edits, int64_t n, hipStream_t stream) {
  SceneUpdate& u = ds->upd;
  std::string err;
  if (!check_shading_edits("rtx_scene_set_shading", u.shading, edits, n, &err)) { set_error(err); return RTX_EINVAL; }
  const rtx_status dst = check_scene_device(ds, "rtx_scene_set_shading", "was uploaded to");
  if (dst != RTX_OK) return dst;
  bool texture_edit = false;
  const std::vector<rt::ShadingWrite> writes = plan_shading(u.shading, edits, n, ds->world.desc != nullptr, &texture_edit);
#ifndef RTX_F32_TU
  const bool refresh = texture_edit && ds->lights.n_lights > 0;  // (an f32 scene holds no light table)
  if (refresh && !ds->mesh.d_light_weight) HIP_TRY(ds->mesh.d_light_weight.alloc((size_t)ds->lights.n_lights * sizeof(double)));
#endif
  const size_t bytes = writes.size() * sizeof(rt::ShadingWrite);
  void* h = nullptr;
  HIP_TRY(u.staging.reserve(bytes, stream, &h));
  memcpy(h, writes.data(), bytes);
  HIP_TRY(u.staging.copy(bytes, stream));
  hipLaunchKernelGGL(k_set_shading, dim3((unsigned)((writes.size() + 255) / 256)), dim3(256), 0, stream, (const rt::ShadingWrite*)u.staging.device(),
                     (int)writes.size(), (rt::FlatMaterial*)ds->view.materials, (rt::FlatTexture*)ds->view.textures, (rt::FlatEntry*)ds->view.entries,
                     (WorldDesc*)ds->world.desc);
  HIP_TRY(hipGetLastError());
#ifndef RTX_F32_TU
  if (refresh) {
    hipLaunchKernelGGL(k_refresh_lights, dim3(1), dim3(256), 0, stream, ds->view, (rt::FlatLight*)ds->lights.lights, ds->lights.n_lights,
                       (double*)ds->mesh.d_light_weight);
    HIP_TRY(hipGetLastError());
  }
#endif
  return RTX_OK;
}
