// The launchers of the ray queries, the gather and the nearest-point query (included by render.hip, namespace rtx, so compiled for both precisions).  Device
// pointers, asynchronous on the caller's stream; the arguments were checked by the entry point (query_entries.inc, abi.cpp).
// Each is a check (check_walk_launch), the launch slices of the batch (host/ray_slices.hpp), the kernel's argument struct, the
// launch of the scene's preset (with_query_preset).

// What a launcher of a kernel that walks with LdsStack checks first: the scene lives on the current device, and its deepest
// walk fits the LDS stack (*stack_lds: the launch's dynamic LDS bytes).  who: the prefix of the message.
static rtx_status check_walk_launch(const DeviceScene* ds, const char* who, size_t* stack_lds) {
  int cur = -1;
  HIP_TRY(hipGetDevice(&cur));
  if (cur != ds->device) { set_error(std::string(who) + ": scene was uploaded to a different device than the current one"); return RTX_EINVAL; }
  *stack_lds = stack_bytes((uint32_t)ds->view.max_stack + 1u);
  if (*stack_lds > 64 * 1024) { set_error(std::string(who) + ": BVH too deep for the LDS traversal stack"); return RTX_EUNSUPPORTED; }
  return RTX_OK;
}

// launch(std::integral_constant<uint32_t, preset>) with the feature preset a query kernel is instantiated for: instance trees,
// everything (GravitySpheres), any other world.
template <class Launch>
static void with_query_preset(uint32_t features, Launch launch) {
  if (features & rt::F_INSTANCE) launch(std::integral_constant<uint32_t, P_INST>());
  else if (features & rt::F_GRAVITY_SPHERE) launch(std::integral_constant<uint32_t, P_ALL>());
  else launch(std::integral_constant<uint32_t, P_ANY>());
}

// Scenes with GravitySpheres: a ray later than this is not walked (the reference's brute-force loop is unbounded there).
static double query_time_limit(const DeviceScene* ds) { return (ds->view.features & rt::F_GRAVITY_SPHERE) ? ds->gravity_time_limit : 1e300; }

// A launch indexes rays with 32 bits, so a batch goes out in launch slices of CAST_LAUNCH_RAYS.
static const int64_t CAST_LAUNCH_RAYS = (int64_t)1 << 30;

// The launches of a cast or an occlusion batch: one ray per lane, launch(preset, the slice's batch, its first ray, grid, LDS bytes).
template <class Launch>
static rtx_status launch_ray_batch(DeviceScene* ds, const char* who, const RtxRayBatch* b, Launch launch) {
  size_t stack_lds = 0;
  const rtx_status st = check_walk_launch(ds, who, &stack_lds);
  if (st != RTX_OK) return st;
  return for_ray_slices(b->n, CAST_LAUNCH_RAYS, [&](int64_t first, int64_t count) -> rtx_status {
    const dim3 grid(grid_size((uint32_t)count, TRACE_BLOCK, (uint64_t)ds->n_cu * 8));
    with_query_preset(ds->view.features, [&](auto preset) { launch(preset, slice_of(*b, first, count), first, grid, stack_lds); });
    HIP_TRY(hipGetLastError());
    return RTX_OK;
  });
}

// Ray queries (cast_rays.inc: k_cast_rays): the batch's rays against the scene, the requested columns written.
static rtx_status launch_cast_rays(DeviceScene* ds, const RtxRayBatch* b, const RtxRayHits* h, hipStream_t stream) {
  return launch_ray_batch(ds, "cast_rays", b, [&](auto preset, const RtxRayBatch& s, int64_t first, dim3 grid, size_t stack_lds) {
    const RtxRayHits o = slice_of(*h, first);
    const CastArgs a = {{s.origin, s.direction, s.time}, s.t_max, s.t_min, s.t_max_all, query_time_limit(ds), s.seed, s.stream_step,
                        o.t, o.p, o.normal, o.uv, o.ids};
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cast_rays<decltype(preset)::value>), grid, dim3(TRACE_BLOCK), stack_lds, stream, ds->view, a,
                       (uint32_t)s.n);
  });
}

// Occlusion queries (occlusion.inc: k_occlusion): tau of the batch's rays.
static rtx_status launch_occlusion(DeviceScene* ds, const RtxRayBatch* b, double* d_tau, hipStream_t stream) {
  return launch_ray_batch(ds, "occlusion", b, [&](auto preset, const RtxRayBatch& s, int64_t first, dim3 grid, size_t stack_lds) {
    const OcclusionArgs a = {{s.origin, s.direction, s.time}, s.t_max, s.t_min, s.t_max_all, query_time_limit(ds), slice_of(d_tau, 1, first)};
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_occlusion<decltype(preset)::value>), grid, dim3(TRACE_BLOCK), stack_lds, stream, ds->view, a,
                       (uint32_t)s.n);
  });
}

// Nearest-point queries (nearest.inc: k_nearest): the requested columns of the batch's points.  Scenes with GravitySpheres are
// refused (include/rtx_abi.h says why), so of with_query_preset's three only P_INST and P_ANY are instantiated.
// check_nearest_launch is what refuses, for the launcher and -- before anything is staged -- for the host entry.
static rtx_status check_nearest_launch(const DeviceScene* ds, size_t* stack_lds) {
  if (ds->view.features & rt::F_GRAVITY_SPHERE) {
    set_error("nearest: scenes with GravitySpheres are not supported (their boxes do not bound the trajectory)");
    return RTX_EUNSUPPORTED;
  }
  return check_walk_launch(ds, "nearest", stack_lds);
}
static rtx_status launch_nearest(DeviceScene* ds, const RtxPointBatch* b, const RtxNearest* out, hipStream_t stream) {
  size_t stack_lds = 0;
  const rtx_status st = check_nearest_launch(ds, &stack_lds);
  if (st != RTX_OK) return st;
  return for_ray_slices(b->n, CAST_LAUNCH_RAYS, [&](int64_t first, int64_t count) -> rtx_status {
    const dim3 grid(grid_size((uint32_t)count, TRACE_BLOCK, (uint64_t)ds->n_cu * 8));
    const RtxPointBatch s = slice_of(*b, first, count);
    const RtxNearest o = slice_of(*out, first);
    const NearestArgs a = {s.points, s.time, s.r_max, s.r_max_all, s.media, o.d, o.q, o.ids};
    if (ds->view.features & rt::F_INSTANCE)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nearest<P_INST>), grid, dim3(TRACE_BLOCK), stack_lds, stream, ds->view, a, (uint32_t)s.n);
    else
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nearest<P_ANY>), grid, dim3(TRACE_BLOCK), stack_lds, stream, ds->view, a, (uint32_t)s.n);
    HIP_TRY(hipGetLastError());
    return RTX_OK;
  });
}

// One pass of a radiance query (trace_rays.inc: k_trace_rays) on `stream`: its work counter zeroed, then the persistent launch --
// as many blocks as are resident, at most one wave per TRACE_CHUNK items (launch_nee's rule).
template <bool NEE>
static rtx_status launch_trace_rays_pass(const DeviceScene* ds, const rt::RenderParams& rp, const RadianceArgs& ra, uint32_t s_begin,
                                         uint32_t total, uint32_t n, double* samples, unsigned int* work_counter, size_t stack_lds,
                                         hipStream_t stream) {
  HIP_TRY(hipMemsetAsync(work_counter, 0, sizeof(unsigned int), stream));
  with_query_preset(ds->view.features, [&](auto preset) {
    constexpr uint32_t F = decltype(preset)::value;
    const int nb = occupancy(k_trace_rays<F, NEE>, stack_lds);
    const uint32_t grid = grid_size(total, TRACE_CHUNK, (uint64_t)ds->n_cu * (uint64_t)(nb > 0 ? nb : 1) * (TRACE_BLOCK / 64));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_trace_rays<F, NEE>), dim3((grid + TRACE_BLOCK / 64 - 1) / (TRACE_BLOCK / 64)),
                       dim3(TRACE_BLOCK), stack_lds, stream, ds->view, ds->lights, rp, ra, s_begin, total, n, samples, work_counter);
  });
  HIP_TRY(hipGetLastError());
  return RTX_OK;
}

// Radiance queries (trace_rays.inc: k_trace_rays): q->samples samples of the estimator along every ray of the batch, summed in
// sample order onto d_sum (and their squares onto d_sumsq unless NULL).  Asynchronous on stream unless stats is asked for.
// Passes are planned by prepare_workspace and run as a render's do: two deep when the sample buffer does not hold the call, even
// passes on the caller's stream, odd ones on ws.aux_stream, reductions in pass order.
static rtx_status trace_rays_impl(DeviceScene* ds, const RtxRadianceRays* q, double* d_sum, double* d_sumsq, hipStream_t stream,
                                  RtxRenderStats* stats) {
  size_t stack_lds = 0;
  rtx_status st = check_walk_launch(ds, "trace_rays", &stack_lds);
  if (st != RTX_OK) return st;
#ifdef RTX_F32_TU
  if (q->light_sampling) { set_error("trace_rays: light sampling is f64 only"); return RTX_EUNSUPPORTED; }  // (the entry points reject it first)
  const auto launch_pass = launch_trace_rays_pass<false>;
#else
  const auto launch_pass = q->light_sampling ? launch_trace_rays_pass<true> : launch_trace_rays_pass<false>;
#endif
  rt::RenderParams rp;
  memset(&rp, 0, sizeof(rp));  // no camera, no image: path_begin_ray reads neither
  rp.background = rt::v3(q->background[0], q->background[1], q->background[2]);
  rp.samples_per_pixel = q->samples;
  rp.max_depth = q->max_depth;
  rp.seed = q->seed;
  const uint32_t spp = (uint32_t)q->samples;
  if (stats) memset(stats, 0, sizeof(*stats));
  Workspace& ws = ds->ws;
  float trace_ms = 0.f;
  int passes = 0;
  size_t sample_bytes = 0;
  st = for_ray_slices(q->n, CAST_LAUNCH_RAYS, [&](int64_t first, int64_t count) -> rtx_status {
    const RtxRadianceRays s = slice_of(*q, first, count);
    const uint32_t n = (uint32_t)count;
    double* sum = slice_of(d_sum, 3, first);
    double* sumsq = slice_of(d_sumsq, 3, first);
    PassPlan pp;
    const rtx_status pst = prepare_workspace(ds, q->sample_buffer_bytes, n, n, spp, stats != nullptr, stream, &sum, &pp);
    if (pst != RTX_OK) return pst;
    sample_bytes = std::max(sample_bytes, pp.sample_bytes);
    const RadianceArgs ra = {{s.origin, s.direction, s.time}, query_time_limit(ds), s.first_ray};
    if (pp.pipeline) {
      HIP_TRY(hipEventRecord(ws.ev_pass[2], stream));
      HIP_TRY(hipStreamWaitEvent(ws.aux_stream, ws.ev_pass[2], 0));
    }
    int k = 0;  // passes of this launch slice
    for (uint32_t s_off = 0; s_off < spp; s_off += pp.spp_pass, ++k, ++passes) {
      const int half = pp.pipeline ? (k & 1) : 0;
      const uint32_t s_count = spp - s_off < pp.spp_pass ? spp - s_off : pp.spp_pass;
      const uint32_t total = (uint32_t)((uint64_t)s_count * n);
      const hipStream_t ps = half ? ws.aux_stream : stream;
      double* samples = ws.samples + (size_t)half * (size_t)pp.spp_pass * (size_t)n * 3u;
      if (stats) HIP_TRY(hipEventRecord(ws.ev[0], ps));
      const rtx_status lst = launch_pass(ds, rp, ra, s.first_sample + s_off, total, n, samples, ws.work_counter + half, stack_lds, ps);
      if (lst != RTX_OK) return lst;
      if (stats) {
        HIP_TRY(hipEventRecord(ws.ev[1], ps));
        HIP_TRY(hipEventSynchronize(ws.ev[1]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]));
        trace_ms += ms;
      }
      const uint32_t pgrid = (n + 255u) / 256u;
      if (pp.pipeline && k > 0) HIP_TRY(hipStreamWaitEvent(ps, ws.ev_pass[1 - half], 0));  // the previous pass's sums are in
      const int first_pass = s_off == 0 && !q->accumulate ? 1 : 0;
      if (sumsq) hipLaunchKernelGGL(k_reduce_samples_moments, dim3(pgrid), dim3(256), 0, ps, samples, sum, sumsq, n, s_count, first_pass);
      else hipLaunchKernelGGL(k_reduce_samples, dim3(pgrid), dim3(256), 0, ps, samples, sum, n, s_count, first_pass);
      HIP_TRY(hipGetLastError());
      if (pp.pipeline) HIP_TRY(hipEventRecord(ws.ev_pass[half], ps));
    }
    if (pp.pipeline && k > 0 && ((k - 1) & 1)) HIP_TRY(hipStreamWaitEvent(stream, ws.ev_pass[1], 0));
    return RTX_OK;
  });
  if (st != RTX_OK) return st;
  if (stats) {
    HIP_TRY(hipStreamSynchronize(stream));
    stats->trace_ms = trace_ms;
    stats->trace_launches = passes;
    stats->passes = passes;
    stats->trace_kernel = RTX_KERNEL_RAYS;
    stats->sample_buffer_bytes = sample_bytes;
    stats->samples = (uint64_t)spp * (uint64_t)q->n;
  }
  return RTX_OK;
}

// Points per group of a gather pass's item order (core/item_order.hpp): a wave holds many samples of few points, as k_trace_world's
// does.  One group (item g = s_local * n + r, a wave's 64 consecutive items 64 consecutive points of one sample) reads the
// columns contiguously but measured 1 to 18 % slower on every workload of scripts/bench_gather.py; groups of 1 and of 4 points
// measured alike (DESIGN.md section 7.6).  With one sample a pass every group size is the same order.
static const uint32_t GATHER_ITEM_GROUP = 4;

// One pass of a gather query (gather.inc: k_gather) on `stream`: launch_trace_rays_pass' rule.
template <bool NEE, bool SURFACE>
static rtx_status launch_gather_pass(const DeviceScene* ds, const rt::RenderParams& rp, const GatherArgs& ga, uint32_t s_begin,
                                     uint32_t total, uint32_t n, double* samples, unsigned int* work_counter, size_t stack_lds,
                                     hipStream_t stream) {
  HIP_TRY(hipMemsetAsync(work_counter, 0, sizeof(unsigned int), stream));
  // the pass's item order (core/item_order.hpp): total = s_count * n items in groups of GATHER_ITEM_GROUP points (RTX_ITEM_GROUP overrides)
  const rt::ItemOrder order = rt::make_item_order(n, total / n, ds->sw.item_group ? ds->sw.item_group : GATHER_ITEM_GROUP);
  with_query_preset(ds->view.features, [&](auto preset) {
    constexpr uint32_t F = decltype(preset)::value;
    const int nb = occupancy(k_gather<F, NEE, SURFACE>, stack_lds);
    const uint32_t grid = grid_size(total, TRACE_CHUNK, (uint64_t)ds->n_cu * (uint64_t)(nb > 0 ? nb : 1) * (TRACE_BLOCK / 64));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gather<F, NEE, SURFACE>), dim3((grid + TRACE_BLOCK / 64 - 1) / (TRACE_BLOCK / 64)),
                       dim3(TRACE_BLOCK), stack_lds, stream, ds->view, ds->lights, rp, ga, order, s_begin, total, samples, work_counter);
  });
  HIP_TRY(hipGetLastError());
  return RTX_OK;
}

// Gather queries (gather.inc: k_gather): q->samples samples of the estimator from every point of the batch, summed in sample order
// onto d_sum (and their squares onto d_sumsq unless NULL) -- plain sums [n][3], or with q->sh_order > 0 the spherical-harmonic
// sums [n][K][3] of k_reduce_samples_sh.  Passes, streams and reductions as in trace_rays_impl.
static rtx_status gather_impl(DeviceScene* ds, const RtxGatherPoints* q, double* d_sum, double* d_sumsq, hipStream_t stream,
                              RtxRenderStats* stats) {
  size_t stack_lds = 0;
  rtx_status st = check_walk_launch(ds, "gather", &stack_lds);
  if (st != RTX_OK) return st;
  const bool surface = q->normal != nullptr;
#ifdef RTX_F32_TU
  if (q->light_sampling) { set_error("gather: light sampling is f64 only"); return RTX_EUNSUPPORTED; }  // (the entry points reject it first)
  const auto launch_pass = surface ? launch_gather_pass<false, true> : launch_gather_pass<false, false>;
#else
  const auto launch_pass = q->light_sampling ? (surface ? launch_gather_pass<true, true> : launch_gather_pass<true, false>)
                                             : (surface ? launch_gather_pass<false, true> : launch_gather_pass<false, false>);
#endif
  rt::RenderParams rp;
  memset(&rp, 0, sizeof(rp));  // no camera, no image: path_begin_gather reads neither
  rp.background = rt::v3(q->background[0], q->background[1], q->background[2]);
  rp.samples_per_pixel = q->samples;
  rp.max_depth = q->max_depth;
  rp.seed = q->seed;
  const uint32_t spp = (uint32_t)q->samples;
  const int64_t width = 3 * (int64_t)sh_coeffs(q->sh_order);  // doubles of sums a point
  if (stats) memset(stats, 0, sizeof(*stats));
  Workspace& ws = ds->ws;
  float trace_ms = 0.f;
  int passes = 0;
  size_t sample_bytes = 0;
  st = for_ray_slices(q->n, CAST_LAUNCH_RAYS, [&](int64_t first, int64_t count) -> rtx_status {
    const RtxGatherPoints s = slice_of(*q, first, count);
    const uint32_t n = (uint32_t)count;
    double* sum = slice_of(d_sum, width, first);
    double* sumsq = slice_of(d_sumsq, width, first);
    PassPlan pp;
    const rtx_status pst = prepare_workspace(ds, q->sample_buffer_bytes, n, n, spp, stats != nullptr, stream, &sum, &pp);
    if (pst != RTX_OK) return pst;
    sample_bytes = std::max(sample_bytes, pp.sample_bytes);
    const GatherArgs ga = {s.position, s.normal, s.time, query_time_limit(ds), s.first_point};
    if (pp.pipeline) {
      HIP_TRY(hipEventRecord(ws.ev_pass[2], stream));
      HIP_TRY(hipStreamWaitEvent(ws.aux_stream, ws.ev_pass[2], 0));
    }
    int k = 0;  // passes of this launch slice
    for (uint32_t s_off = 0; s_off < spp; s_off += pp.spp_pass, ++k, ++passes) {
      const int half = pp.pipeline ? (k & 1) : 0;
      const uint32_t s_count = spp - s_off < pp.spp_pass ? spp - s_off : pp.spp_pass;
      const uint32_t total = (uint32_t)((uint64_t)s_count * n);
      const hipStream_t ps = half ? ws.aux_stream : stream;
      double* samples = ws.samples + (size_t)half * (size_t)pp.spp_pass * (size_t)n * 3u;
      if (stats) HIP_TRY(hipEventRecord(ws.ev[0], ps));
      const rtx_status lst = launch_pass(ds, rp, ga, s.first_sample + s_off, total, n, samples, ws.work_counter + half, stack_lds, ps);
      if (lst != RTX_OK) return lst;
      if (stats) {
        HIP_TRY(hipEventRecord(ws.ev[1], ps));
        HIP_TRY(hipEventSynchronize(ws.ev[1]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]));
        trace_ms += ms;
      }
      const uint32_t pgrid = (n + 255u) / 256u;
      if (pp.pipeline && k > 0) HIP_TRY(hipStreamWaitEvent(ps, ws.ev_pass[1 - half], 0));  // the previous pass's sums are in
      const int first_pass = s_off == 0 && !q->accumulate ? 1 : 0;
      if (q->sh_order == 2)
        hipLaunchKernelGGL(k_reduce_samples_sh<2>, dim3(pgrid), dim3(256), 0, ps, samples, sum, sumsq, n, s_count, first_pass, q->seed,
                           s.first_point, s.first_sample + s_off);
      else if (q->sh_order == 1)
        hipLaunchKernelGGL(k_reduce_samples_sh<1>, dim3(pgrid), dim3(256), 0, ps, samples, sum, sumsq, n, s_count, first_pass, q->seed,
                           s.first_point, s.first_sample + s_off);
      else if (sumsq) hipLaunchKernelGGL(k_reduce_samples_moments, dim3(pgrid), dim3(256), 0, ps, samples, sum, sumsq, n, s_count, first_pass);
      else hipLaunchKernelGGL(k_reduce_samples, dim3(pgrid), dim3(256), 0, ps, samples, sum, n, s_count, first_pass);
      HIP_TRY(hipGetLastError());
      if (pp.pipeline) HIP_TRY(hipEventRecord(ws.ev_pass[half], ps));
    }
    if (pp.pipeline && k > 0 && ((k - 1) & 1)) HIP_TRY(hipStreamWaitEvent(stream, ws.ev_pass[1], 0));
    return RTX_OK;
  });
  if (st != RTX_OK) return st;
  if (stats) {
    HIP_TRY(hipStreamSynchronize(stream));
    stats->trace_ms = trace_ms;
    stats->trace_launches = passes;
    stats->passes = passes;
    stats->trace_kernel = RTX_KERNEL_RAYS;
    stats->sample_buffer_bytes = sample_bytes;
    stats->samples = (uint64_t)spp * (uint64_t)q->n;
  }
  return RTX_OK;
}
