// The entry points of the ray queries and of the nearest-point query (included by render.hip's f64-only tail; the launchers: queries.inc).  A device entry
// takes the caller's device columns, asynchronous on the caller's stream; a host entry stages slices of RTX_*_HOST_SLICE rays
// (cut by host/ray_slices.hpp, as the launcher cuts a launch's) through device buffers, one after the other on the null stream.
// The arguments are checked first (abi.cpp: check_ray_batch, check_trace_rays, check_gather, check_point_batch), before any device call and before the handle is read.

// One column of a host entry, staged through a device buffer of its own: host pointer (NULL: the caller left the column out, its
// device pointer stays NULL), bytes per ray, copied in before the call?, copied out after it?
struct StagedColumn {
  const void* host; size_t bytes; bool in, out;
  DeviceBuffer<double> dev;
};
// Room for `rays` rays in every column that is not NULL.
template <size_t K>
static hipError_t stage_alloc(StagedColumn (&cols)[K], int64_t rays) {
  hipError_t e = hipSuccess;
  for (size_t i = 0; i < K && e == hipSuccess; ++i)
    if (cols[i].host) e = cols[i].dev.alloc((size_t)rays * cols[i].bytes);
  return e;
}
// Rays [first, first + count) of the "in" columns to the device, or (out) of the "out" columns back: blocking copies on the null
// stream, so a copy out waits for the launches before it.
template <size_t K>
static hipError_t stage_copy(StagedColumn (&cols)[K], int64_t first, int64_t count, bool out) {
  hipError_t e = hipSuccess;
  for (size_t i = 0; i < K && e == hipSuccess; ++i) {
    const StagedColumn& c = cols[i];
    if (!c.host || !(out ? c.out : c.in)) continue;
    const char* host = slice_of((const char*)c.host, (int64_t)c.bytes, first);
    e = out ? hipMemcpy((void*)host, c.dev, (size_t)count * c.bytes, hipMemcpyDeviceToHost)
            : hipMemcpy(c.dev, host, (size_t)count * c.bytes, hipMemcpyHostToDevice);
  }
  return e;
}

// What the kernels need of the device columns: RTX_EINVAL naming the first pointer with a bit of its mask set (7: stored as
// doubles, 15: stored 16 bytes at a time).
struct AlignedColumn { const void* p; uintptr_t mask; const char* name; };
static rtx_status check_aligned(const char* who, std::initializer_list<AlignedColumn> cols) {
  for (const AlignedColumn& c : cols)
    if ((uintptr_t)c.p & c.mask) {
      set_error(std::string(who) + ": " + c.name + " is not " + std::to_string(c.mask + 1) + "-byte aligned");
      return RTX_EINVAL;
    }
  return RTX_OK;
}

extern "C" {

// ---- ray queries
rtx_status rtx_scene_cast_rays_device(const rtx_scene* s, const RtxRayBatch* rays, const RtxRayHits* hits, void* hip_stream) {
  rtx_status st = check_ray_batch("rtx_scene_cast_rays_device", s, rays, hits, "hits");
  if (st != RTX_OK || rays->n == 0) return st;
  // the kernel stores uv as double2 and ids as int4, and every other column as doubles
  st = check_aligned("rtx_scene_cast_rays_device",
                     {{rays->origin, 7, "rays->origin"}, {rays->direction, 7, "rays->direction"}, {rays->time, 7, "rays->time"},
                      {rays->t_max, 7, "rays->t_max"},   {hits->t, 7, "hits->t"},                 {hits->p, 7, "hits->p"},
                      {hits->normal, 7, "hits->normal"}, {hits->uv, 15, "hits->uv"},              {hits->ids, 15, "hits->ids"}});
  if (st != RTX_OK) return st;
  return s->ops->cast_rays(s->device_scene, rays, hits, (hipStream_t)hip_stream);
}

// Host pointers: in 56 B a ray, out 88 B.
rtx_status rtx_scene_cast_rays(const rtx_scene* s, const RtxRayBatch* rays, const RtxRayHits* hits) {
  rtx_status st = check_ray_batch("rtx_scene_cast_rays", s, rays, hits, "hits");
  if (st != RTX_OK || rays->n == 0) return st;
  StagedColumn cols[] = {{rays->origin, 24, true, false}, {rays->direction, 24, true, false}, {rays->time, 8, true, false},
                         {rays->t_max, 8, true, false},   {hits->t, 8, false, true},          {hits->p, 24, false, true},
                         {hits->normal, 24, false, true}, {hits->uv, 16, false, true},        {hits->ids, 16, false, true}};
  HIP_TRY(stage_alloc(cols, std::min<int64_t>(rays->n, RTX_CAST_HOST_SLICE)));
  st = for_ray_slices(rays->n, RTX_CAST_HOST_SLICE, [&](int64_t first, int64_t count) -> rtx_status {
    HIP_TRY(stage_copy(cols, first, count, false));
    RtxRayBatch b = slice_of(*rays, first, count);
    b.origin = cols[0].dev; b.direction = cols[1].dev; b.time = cols[2].dev; b.t_max = cols[3].dev;
    const RtxRayHits h = {cols[4].dev, cols[5].dev, cols[6].dev, cols[7].dev, (int32_t*)(double*)cols[8].dev};
    const rtx_status lst = s->ops->cast_rays(s->device_scene, &b, &h, (hipStream_t) nullptr);
    if (lst != RTX_OK) return lst;
    HIP_TRY(stage_copy(cols, first, count, true));
    return RTX_OK;
  });
  if (st != RTX_OK) return st;
  HIP_TRY(hipDeviceSynchronize());  // an all-NULL RtxRayHits (a timing run) still returns after its launches
  return RTX_OK;
}

// ---- occlusion queries
rtx_status rtx_scene_occlusion_device(const rtx_scene* s, const RtxRayBatch* rays, double* d_tau, void* hip_stream) {
  rtx_status st = check_ray_batch("rtx_scene_occlusion_device", s, rays, d_tau, "tau");
  if (st != RTX_OK || rays->n == 0) return st;
  st = check_aligned("rtx_scene_occlusion_device", {{rays->origin, 7, "rays->origin"}, {rays->direction, 7, "rays->direction"},
                                                    {rays->time, 7, "rays->time"},     {rays->t_max, 7, "rays->t_max"},
                                                    {d_tau, 7, "d_tau"}});
  if (st != RTX_OK) return st;
  return s->ops->occlusion(s->device_scene, rays, d_tau, (hipStream_t)hip_stream);
}

// Host pointers: in 56 B a ray, out 8 B.
rtx_status rtx_scene_occlusion(const rtx_scene* s, const RtxRayBatch* rays, double* tau) {
  const rtx_status st = check_ray_batch("rtx_scene_occlusion", s, rays, tau, "tau");
  if (st != RTX_OK || rays->n == 0) return st;
  StagedColumn cols[] = {{rays->origin, 24, true, false}, {rays->direction, 24, true, false}, {rays->time, 8, true, false},
                         {rays->t_max, 8, true, false},   {tau, 8, false, true}};
  HIP_TRY(stage_alloc(cols, std::min<int64_t>(rays->n, RTX_CAST_HOST_SLICE)));
  return for_ray_slices(rays->n, RTX_CAST_HOST_SLICE, [&](int64_t first, int64_t count) -> rtx_status {
    HIP_TRY(stage_copy(cols, first, count, false));
    RtxRayBatch b = slice_of(*rays, first, count);
    b.origin = cols[0].dev; b.direction = cols[1].dev; b.time = cols[2].dev; b.t_max = cols[3].dev;
    const rtx_status lst = s->ops->occlusion(s->device_scene, &b, cols[4].dev, (hipStream_t) nullptr);
    if (lst != RTX_OK) return lst;
    HIP_TRY(stage_copy(cols, first, count, true));
    return RTX_OK;
  });
}

// ---- nearest-point queries
rtx_status rtx_scene_nearest_device(const rtx_scene* s, const RtxPointBatch* points, const RtxNearest* out, void* hip_stream) {
  rtx_status st = check_point_batch("rtx_scene_nearest_device", s, points, out);
  if (st != RTX_OK || points->n == 0) return st;
  // the kernel stores ids as int4 and every other column as doubles
  st = check_aligned("rtx_scene_nearest_device", {{points->points, 7, "points->points"}, {points->time, 7, "points->time"},
                                                  {points->r_max, 7, "points->r_max"},   {out->d, 7, "out->d"},
                                                  {out->q, 7, "out->q"},                 {out->ids, 15, "out->ids"}});
  if (st != RTX_OK) return st;
  return s->ops->nearest(s->device_scene, points, out, (hipStream_t)hip_stream);
}

// Host pointers: in 40 B a point, out 48 B.
rtx_status rtx_scene_nearest(const rtx_scene* s, const RtxPointBatch* points, const RtxNearest* out) {
  rtx_status st = check_point_batch("rtx_scene_nearest", s, points, out);
  if (st != RTX_OK || points->n == 0) return st;
  if ((st = s->ops->nearest_supported(s->device_scene)) != RTX_OK) return st;  // refused before a byte is staged
  StagedColumn cols[] = {{points->points, 24, true, false}, {points->time, 8, true, false}, {points->r_max, 8, true, false},
                         {out->d, 8, false, true},          {out->q, 24, false, true},      {out->ids, 16, false, true}};
  HIP_TRY(stage_alloc(cols, std::min<int64_t>(points->n, RTX_CAST_HOST_SLICE)));
  st = for_ray_slices(points->n, RTX_CAST_HOST_SLICE, [&](int64_t first, int64_t count) -> rtx_status {
    HIP_TRY(stage_copy(cols, first, count, false));
    RtxPointBatch b = slice_of(*points, first, count);
    b.points = cols[0].dev; b.time = cols[1].dev; b.r_max = cols[2].dev;
    const RtxNearest o = {cols[3].dev, cols[4].dev, (int32_t*)(double*)cols[5].dev};
    const rtx_status lst = s->ops->nearest(s->device_scene, &b, &o, (hipStream_t) nullptr);
    if (lst != RTX_OK) return lst;
    HIP_TRY(stage_copy(cols, first, count, true));
    return RTX_OK;
  });
  if (st != RTX_OK) return st;
  HIP_TRY(hipDeviceSynchronize());  // an all-NULL RtxNearest (a timing run) still returns after its launches
  return RTX_OK;
}

// ---- radiance queries
rtx_status rtx_scene_trace_rays_device(const rtx_scene* s, const RtxRadianceRays* rays, double* d_sum_rgb, double* d_sumsq_rgb,
                                       void* hip_stream, RtxRenderStats* stats) {
  rtx_status st = check_trace_rays("rtx_scene_trace_rays_device", s, rays, d_sum_rgb);
  if (st != RTX_OK) return st;
  st = check_aligned("rtx_scene_trace_rays_device", {{rays->origin, 7, "rays->origin"}, {rays->direction, 7, "rays->direction"},
                                                     {rays->time, 7, "rays->time"},     {d_sum_rgb, 7, "sum_rgb"},
                                                     {d_sumsq_rgb, 7, "sumsq_rgb"}});
  if (st != RTX_OK) return st;
  if (stats && rays->n == 0) memset(stats, 0, sizeof(*stats));
  if (rays->n == 0) return RTX_OK;
  if (rays->light_sampling && s->f32) {
    set_error("rtx_scene_trace_rays_device: light sampling needs an f64 scene (rtx_scene_upload)");
    return RTX_EUNSUPPORTED;
  }
  return s->ops->trace_rays(s->device_scene, rays, d_sum_rgb, d_sumsq_rgb, (hipStream_t)hip_stream, stats);
}

// Host pointers: in 56 B a ray, sums 48 B (copied in as well when the call continues them).
rtx_status rtx_scene_trace_rays(const rtx_scene* s, const RtxRadianceRays* rays, double* sum_rgb, double* sumsq_rgb,
                                RtxRenderStats* stats) {
  const rtx_status st = check_trace_rays("rtx_scene_trace_rays", s, rays, sum_rgb);
  if (st != RTX_OK) return st;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (rays->n == 0) return RTX_OK;
  if (rays->light_sampling && s->f32) {
    set_error("rtx_scene_trace_rays: light sampling needs an f64 scene (rtx_scene_upload)");
    return RTX_EUNSUPPORTED;
  }
  const bool cont = rays->accumulate != 0;
  StagedColumn cols[] = {{rays->origin, 24, true, false}, {rays->direction, 24, true, false}, {rays->time, 8, true, false},
                         {sum_rgb, 24, cont, true},       {sumsq_rgb, 24, cont, true}};
  HIP_TRY(stage_alloc(cols, std::min<int64_t>(rays->n, RTX_TRACE_HOST_SLICE)));
  return for_ray_slices(rays->n, RTX_TRACE_HOST_SLICE, [&](int64_t first, int64_t count) -> rtx_status {
    HIP_TRY(stage_copy(cols, first, count, false));
    RtxRadianceRays b = slice_of(*rays, first, count);
    b.origin = cols[0].dev; b.direction = cols[1].dev; b.time = cols[2].dev;
    RtxRenderStats one;
    const rtx_status lst = s->ops->trace_rays(s->device_scene, &b, cols[3].dev, cols[4].dev, (hipStream_t) nullptr, stats ? &one : nullptr);
    if (lst != RTX_OK) return lst;
    HIP_TRY(stage_copy(cols, first, count, true));  // (the odd passes were joined to the null stream)
    if (stats) {
      stats->samples += one.samples; stats->trace_ms += one.trace_ms; stats->trace_launches += one.trace_launches;
      stats->passes += one.passes; stats->trace_kernel = one.trace_kernel;
      stats->sample_buffer_bytes = std::max(stats->sample_buffer_bytes, one.sample_buffer_bytes);
    }
    return RTX_OK;
  });
}

// ---- gather queries
static rtx_status check_gather_precision(const char* who, const rtx_scene* s, const RtxGatherPoints* points) {
  if (points->light_sampling && s->f32) {
    set_error(std::string(who) + ": light sampling needs an f64 scene (rtx_scene_upload)");
    return RTX_EUNSUPPORTED;
  }
  return RTX_OK;
}

rtx_status rtx_scene_gather_device(const rtx_scene* s, const RtxGatherPoints* points, double* d_sum, double* d_sumsq, void* hip_stream,
                                   RtxRenderStats* stats) {
  rtx_status st = check_gather("rtx_scene_gather_device", s, points, d_sum);
  if (st != RTX_OK) return st;
  st = check_aligned("rtx_scene_gather_device", {{points->position, 7, "points->position"}, {points->normal, 7, "points->normal"},
                                                 {points->time, 7, "points->time"},         {d_sum, 7, "sum"},
                                                 {d_sumsq, 7, "sumsq"}});
  if (st != RTX_OK) return st;
  if (stats && points->n == 0) memset(stats, 0, sizeof(*stats));
  if (points->n == 0) return RTX_OK;
  if ((st = check_gather_precision("rtx_scene_gather_device", s, points)) != RTX_OK) return st;
  return s->ops->gather(s->device_scene, points, d_sum, d_sumsq, (hipStream_t)hip_stream, stats);
}

// Host pointers: in 56 B a point, sums 48 B a point and coefficient (copied in as well when the call continues them).
rtx_status rtx_scene_gather(const rtx_scene* s, const RtxGatherPoints* points, double* sum, double* sumsq, RtxRenderStats* stats) {
  rtx_status st = check_gather("rtx_scene_gather", s, points, sum);
  if (st != RTX_OK) return st;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (points->n == 0) return RTX_OK;
  if ((st = check_gather_precision("rtx_scene_gather", s, points)) != RTX_OK) return st;
  const bool cont = points->accumulate != 0;
  const size_t sum_bytes = 24 * (size_t)sh_coeffs(points->sh_order);
  StagedColumn cols[] = {{points->position, 24, true, false}, {points->normal, 24, true, false}, {points->time, 8, true, false},
                         {sum, sum_bytes, cont, true},        {sumsq, sum_bytes, cont, true}};
  HIP_TRY(stage_alloc(cols, std::min<int64_t>(points->n, RTX_TRACE_HOST_SLICE)));
  return for_ray_slices(points->n, RTX_TRACE_HOST_SLICE, [&](int64_t first, int64_t count) -> rtx_status {
    HIP_TRY(stage_copy(cols, first, count, false));
    RtxGatherPoints b = slice_of(*points, first, count);
    b.position = cols[0].dev; b.normal = cols[1].dev; b.time = cols[2].dev;
    RtxRenderStats one;
    const rtx_status lst = s->ops->gather(s->device_scene, &b, cols[3].dev, cols[4].dev, (hipStream_t) nullptr, stats ? &one : nullptr);
    if (lst != RTX_OK) return lst;
    HIP_TRY(stage_copy(cols, first, count, true));  // (the odd passes were joined to the null stream)
    if (stats) {
      stats->samples += one.samples; stats->trace_ms += one.trace_ms; stats->trace_launches += one.trace_launches;
      stats->passes += one.passes; stats->trace_kernel = one.trace_kernel;
      stats->sample_buffer_bytes = std::max(stats->sample_buffer_bytes, one.sample_buffer_bytes);
    }
    return RTX_OK;
  });
}

// Host only: the start directions the kernels draw, by the core function they run, in either compilation's arithmetic.
rtx_status rtx_gather_directions(const RtxGatherPoints* points, int32_t f32, double* dir) {
  const char* bad = nullptr;
  if (!points) bad = "points is NULL";
  else if (!dir) bad = "dir is NULL";
  else if (points->n < 0) bad = "points->n < 0";
  else if (points->samples < 1) bad = "points->samples < 1";
  else if ((uint64_t)points->first_sample + (uint64_t)points->samples > (1ull << 32)) bad = "points->first_sample + points->samples is past 2^32";
  else if (f32 != 0 && f32 != 1) bad = "f32 is neither 0 nor 1";
  if (bad) { set_error(std::string("rtx_gather_directions: ") + bad); return RTX_EINVAL; }
  if (f32) rtx_f32_gather_directions(points, dir);
  else gather_directions_impl(points, dir);
  return RTX_OK;
}

}  // extern "C"
