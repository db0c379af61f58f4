// k_nearest -- nearest-point queries of a caller's point batch on a resident scene (rtx_scene_nearest*; included by render.hip,
// namespace rtx, so compiled for both precisions).
//
// Point r of a launch is ONE call world_nearest<F, false, LdsStack>(scene, p_r, time_r, r_max_r, media) of the shared core
// (core/nearest.hpp): the closest surface point of the world list, its distance and what it belongs to.  No stream, no draw.
// Points are f64 COLUMNS whichever precision the scene has: the f32 compilation narrows p, time and r_max with the casts
// k_cast_rays uses and widens what it writes.
//
// Scheduling is k_occlusion's: one point per lane, a grid-stride loop whose trip count is wave-uniform (a wave takes 64
// consecutive points per trip), no work counter, no atomics, LdsStack in dynamic LDS.  A wave's 64 distances are one contiguous
// 512-byte store, ids one 16-byte store per lane, q three strided stores as the cast writes its p column.  media is a kernel
// argument: every test on it is wave-uniform.

struct NearestArgs {
  const double* points;  // [n][3]
  const double* time;    // [n] or NULL: 0
  const double* r_max;   // [n] or NULL: r_max_all
  double r_max_all;
  int32_t media;
  double* d;             // [n]
  double* q;             // [n][3]
  int32_t* ids;          // [n][4]
};

template <uint32_t F>
__global__ __launch_bounds__(TRACE_BLOCK) void k_nearest(rt::SceneView sv, NearestArgs a, uint32_t n) {
  extern __shared__ int32_t lds_stack[];
  LdsStack stack;
  stack.base = lds_stack + threadIdx.x;
  stack.n = 0;
  const uint32_t lane = threadIdx.x & 63u;
  const bool media = a.media != 0;
  // `first` is the wave's first point of this trip: the same in every lane, so the trip count is wave-uniform
  for (uint32_t first = blockIdx.x * TRACE_BLOCK + (threadIdx.x & ~63u); first < n; first += gridDim.x * TRACE_BLOCK) {
    const uint32_t r = first + lane;
    if (r < n) {
      double p[3];
      for (int c = 0; c < 3; ++c) p[c] = a.points[3 * (size_t)r + c];
      const double time = a.time ? a.time[r] : 0.0;
      const double r_max = a.r_max ? a.r_max[r] : a.r_max_all;
      rt::NearestBest best;
      stack.reset();
      rt::world_nearest<F, false, LdsStack>(sv, rt::v3((rt::real)p[0], (rt::real)p[1], (rt::real)p[2]), (rt::real)time, (rt::real)r_max,
                                            media, &best, stack, nullptr);
      if (a.d) a.d[r] = best.found ? (double)rt::rt_sqrt(best.d2) : (double)INFINITY;
      if (a.q) {
        const double qv[3] = {best.found ? (double)best.q.x : 0.0, best.found ? (double)best.q.y : 0.0, best.found ? (double)best.q.z : 0.0};
        for (int c = 0; c < 3; ++c) a.q[3 * (size_t)r + c] = qv[c];
      }
      if (a.ids)
        ((int4*)a.ids)[r] = best.found ? make_int4(rt::nearest_material(sv, best), best.slot, (int)rt::primref_type(best.ref),
                                                   (int)rt::primref_index(best.ref))
                                       : make_int4(-1, -1, -1, -1);
    }
  }
}
