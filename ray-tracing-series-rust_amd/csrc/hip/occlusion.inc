// k_occlusion -- any-hit segment casts of a caller's ray batch on a resident scene (rtx_scene_occlusion*; included by render.hip,
// namespace rtx, so compiled for both precisions).
//
// Ray r of a launch is ONE call world_occlusion<F, LdsStack>(scene, Ray(origin_r, direction_r, time_r), t_min, t_max_r) of the
// shared core (core/occlusion.hpp): +inf when a surface blocks the segment, else the summed optical depth of the media on it.
// No stream, no HitRecord, no draw.  Rays are k_cast_rays' f64 columns and the f32 compilation narrows them with the same
// casts; tau is widened to f64 whichever precision the scene has.
//
// Scheduling is k_cast_rays': one ray per lane, a grid-stride loop whose trip count is wave-uniform (a wave takes 64 consecutive
// rays per trip), no work counter, no atomics; a wave's 64 results are one contiguous 512-byte store.  A ray later than the
// GravitySpheres' time limit is not tested and answers NaN (k_trace_rays' rule): a ray that was not tested must not read as clear.

struct OcclusionArgs {
  QueryRays rays;           // cast_rays.inc
  const double* t_max;      // [n] or NULL: t_max_all
  double t_min, t_max_all;
  double time_limit;        // scenes with GravitySpheres: a ray later than this is not tested (DeviceScene::gravity_time_limit)
  double* tau;              // [n]
};

template <uint32_t F>
__global__ __launch_bounds__(TRACE_BLOCK) void k_occlusion(rt::SceneView sv, OcclusionArgs a, uint32_t n) {
  extern __shared__ int32_t lds_stack[];
  LdsStack stack;
  stack.base = lds_stack + threadIdx.x;
  stack.n = 0;
  const uint32_t lane = threadIdx.x & 63u;
  // `first` is the wave's first ray of this trip: the same in every lane, so the trip count is wave-uniform
  for (uint32_t first = blockIdx.x * TRACE_BLOCK + (threadIdx.x & ~63u); first < n; first += gridDim.x * TRACE_BLOCK) {
    const uint32_t r = first + lane;
    if (r < n) {
      double o[3], d[3];
      for (int c = 0; c < 3; ++c) { o[c] = a.rays.origin[3 * (size_t)r + c]; d[c] = a.rays.direction[3 * (size_t)r + c]; }
      const double time = a.rays.time ? a.rays.time[r] : 0.0;
      const double t_max = a.t_max ? a.t_max[r] : a.t_max_all;
      double tau = __builtin_nan("");
      if (!(time > a.time_limit)) {
        const rt::Ray ray = rt::make_ray(rt::v3((rt::real)o[0], (rt::real)o[1], (rt::real)o[2]),
                                         rt::v3((rt::real)d[0], (rt::real)d[1], (rt::real)d[2]), (rt::real)time);
        stack.reset();
        tau = (double)rt::world_occlusion<F, LdsStack>(sv, ray, (rt::real)a.t_min, (rt::real)t_max, stack);
      }
      a.tau[r] = tau;
    }
  }
}
