// k_cast_rays -- closest-hit casts of a caller's ray batch on a resident scene (rtx_scene_cast_rays*; included by render.hip,
// namespace rtx, so compiled for both precisions).
//
// Ray r of a launch is ONE call world_hit<F, false, LdsStack, SLOT = true>(scene, Ray(origin_r, direction_r, time_r), t_min,
// t_max_r, rng_r) of the shared core -- the call a path's bounce makes -- on the stream rng_for_sample(seed + r * stream_step,
// 0, 0), so a ConstantMedium answers with its random hit drawn from that stream.  No second traversal lives here.  Rays and
// results are f64 COLUMNS whichever precision the scene has: the f32 compilation narrows a ray with the casts its camera rays
// go through ((real) of each component, of t_min and of t_max) and widens what it writes, as the accumulators are.
//
// Scheduling: one ray per lane, a grid-stride loop whose trip count is wave-uniform (a wave takes 64 consecutive rays per trip,
// so every column access of a wave is one contiguous block).  The work counter of pass_items.inc (queue_claim) is NOT used: a
// cast leaves the scene untouched and may be enqueued on any number of streams at once, and a counter is per-call mutable device
// state that someone has to own and zero in stream order; what the counter buys the trace kernels -- a lane that takes the next
// item when its path ends early -- has nothing to bite on, every ray being a single walk.
//
// A [n][3] f64 column is a 24-byte stride per lane, read and written as three strided accesses (the compiler merges them
// where it can): a wave's three accesses touch the same twelve 128-byte lines, so HBM sees every line once and the cost is
// address traffic in the vector cache.  No LDS beyond the walk stack, no barrier.

// The ray columns every query kernel takes (device pointers): the first member of CastArgs, OcclusionArgs and RadianceArgs.
// Each kernel reads and narrows a ray with its own lines: a shared loader reordered the code of 15 of the 18 instantiations.
struct QueryRays {
  const double* origin;     // [n][3]
  const double* direction;  // [n][3]
  const double* time;       // [n] or NULL: 0
};

// A launch's rays and result columns (device pointers; a NULL column is not read / not written) -- a kernel argument, so every
// test on it is wave-uniform.
struct CastArgs {
  QueryRays rays;
  const double* t_max;      // [n] or NULL: t_max_all
  double t_min, t_max_all;
  double time_limit;        // scenes with GravitySpheres: a ray later than this is not cast (DeviceScene::gravity_time_limit)
  uint64_t seed, stream_step;
  double* t;        // [n]
  double* p;        // [n][3]
  double* normal;   // [n][3]
  double* uv;       // [n][2]
  int32_t* ids;     // [n][4]
};

template <uint32_t F>
__global__ __launch_bounds__(TRACE_BLOCK) void k_cast_rays(rt::SceneView sv, CastArgs a, uint32_t n) {
  extern __shared__ int32_t lds_stack[];
  LdsStack stack;
  stack.base = lds_stack + threadIdx.x;
  stack.n = 0;
  const uint32_t lane = threadIdx.x & 63u;
  // `first` is the wave's first ray of this trip: the same in every lane, so the trip count is wave-uniform
  for (uint32_t first = blockIdx.x * TRACE_BLOCK + (threadIdx.x & ~63u); first < n; first += gridDim.x * TRACE_BLOCK) {
    const uint32_t r = first + lane;
    const bool live = r < n;
    double o[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0};
    if (live) {
      for (int c = 0; c < 3; ++c) { o[c] = a.rays.origin[3 * (size_t)r + c]; d[c] = a.rays.direction[3 * (size_t)r + c]; }
    }
    rt::HitRecord rec;
    int32_t slot = -1;
    bool hit = false;
    if (live) {
      const double time = a.rays.time ? a.rays.time[r] : 0.0;
      const double t_max = a.t_max ? a.t_max[r] : a.t_max_all;
      const rt::Ray ray = rt::make_ray(rt::v3((rt::real)o[0], (rt::real)o[1], (rt::real)o[2]),
                                       rt::v3((rt::real)d[0], (rt::real)d[1], (rt::real)d[2]), (rt::real)time);
      rt::Rng rng = rt::rng_for_sample(a.seed + (uint64_t)r * a.stream_step, 0, 0);
      if (!(time > a.time_limit)) {
        stack.reset();
        hit = rt::world_hit<F, false, LdsStack, true>(sv, ray, (rt::real)a.t_min, (rt::real)t_max, &rec, rng, stack, nullptr, &slot);
      }
    }
    double pv[3] = {0.0, 0.0, 0.0}, nv[3] = {0.0, 0.0, 0.0};
    if (hit) {
      pv[0] = (double)rec.p.x; pv[1] = (double)rec.p.y; pv[2] = (double)rec.p.z;
      nv[0] = (double)rec.normal.x; nv[1] = (double)rec.normal.y; nv[2] = (double)rec.normal.z;
    }
    if (a.t && live) a.t[r] = hit ? (double)rec.t : (double)INFINITY;
    if (a.p && live) { for (int c = 0; c < 3; ++c) a.p[3 * (size_t)r + c] = pv[c]; }
    if (a.normal && live) { for (int c = 0; c < 3; ++c) a.normal[3 * (size_t)r + c] = nv[c]; }
    if (a.uv && live) ((double2*)a.uv)[r] = hit ? make_double2((double)rec.u, (double)rec.v) : make_double2(0.0, 0.0);
    if (a.ids && live) ((int4*)a.ids)[r] = hit ? make_int4(1, rec.mat, slot, rec.front_face ? 1 : 0) : make_int4(0, -1, -1, 0);
  }
}
