// k_trace_rays -- the estimator's radiance along a caller's rays on a resident scene (rtx_scene_trace_rays*; included by
// render.hip, namespace rtx, so compiled for both precisions; DESIGN.md section 7.4).
//
// A pass is the index space of pass_items.inc with the batch's rays in the place of a shard's pixels: item g = s_local * n + r
// is sample s_begin + s_local of ray r, so 64 consecutive items are 64 consecutive rays of one sample.  The path of an item is
// core/integrator.hpp's path_begin_ray -- the ray as given, the stream of (seed, first_ray + r, sample), no draw before the
// first bounce -- followed by path_step (NEE: path_step_nee), the source the tests' host checker runs.  Scheduling is
// k_trace_nee's: persistent waves claim TRACE_CHUNK items through the pass's work counter, a lane whose path has ended takes the
// next item of the chunk at once (items lane, lane + 64, ...), walk stacks live in LDS.  Every item owns its slot of the pass's
// sample buffer (store_sample); k_reduce_samples / k_reduce_samples_moments add the pass onto the caller's sums in sample order.
//
// Rays come in as k_cast_rays takes them: [n][3] f64 columns read as three strided accesses per lane (cast_rays.inc says what
// that costs and why no LDS staging), an optional [n] time column; the f32 compilation narrows each component with a (real)
// cast.  A ray whose time is past time_limit (scenes with GravitySpheres) is not traced: its sample is stored as NaN, so its
// sums are NaN -- never mistaken for a dark ray.

// A launch's rays (device pointers) -- a kernel argument, so every test on it is wave-uniform.
struct RadianceArgs {
  QueryRays rays;           // cast_rays.inc
  double time_limit;        // scenes with GravitySpheres: a ray later than this is not traced (DeviceScene::gravity_time_limit)
  uint64_t first_ray;       // index of the launch's ray 0 in the caller's whole batch: the stream key's pixel word
};

// Starts item g's path.  false: the ray is not traced and its sample is already stored (NaN).
__device__ __forceinline__ bool start_ray_path(const rt::RenderParams& rp, const RadianceArgs& a, uint32_t n, uint32_t s_begin,
                                               uint32_t g, double* samples, rt::PathState* ps) {
  const uint32_t s_local = g / n;
  const uint32_t r = g - s_local * n;
  double o[3], d[3];
  for (int c = 0; c < 3; ++c) { o[c] = a.rays.origin[3 * (size_t)r + c]; d[c] = a.rays.direction[3 * (size_t)r + c]; }
  const double time = a.rays.time ? a.rays.time[r] : 0.0;
  if (time > a.time_limit) {
    const double nan = __builtin_nan("");
    double* out = samples + 3 * (size_t)g;
    out[0] = nan; out[1] = nan; out[2] = nan;
    return false;
  }
  const rt::Ray ray = rt::make_ray(rt::v3((rt::real)o[0], (rt::real)o[1], (rt::real)o[2]),
                                   rt::v3((rt::real)d[0], (rt::real)d[1], (rt::real)d[2]), (rt::real)time);
  rt::path_begin_ray(rp, ray, a.first_ray + (uint64_t)r, s_begin + s_local, ps);
  return true;
}

template <uint32_t F, bool NEE>
__global__ __launch_bounds__(TRACE_BLOCK) void k_trace_rays(rt::SceneView sv, rt::LightView lv, rt::RenderParams rp, RadianceArgs ra,
                                                             uint32_t s_begin, uint32_t total, uint32_t n,
                                                             double* __restrict__ samples, unsigned int* __restrict__ work_counter) {
  extern __shared__ int32_t lds_stack[];
  LdsStack stack;
  stack.base = lds_stack + threadIdx.x;
  stack.n = 0;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t next = 0, end = 0;  // this lane's next item of the wave's chunk; the chunk's end (wave-uniform)
  uint32_t item = 0;
  bool live = false;
  rt::PathState ps;
  rt::real last_pdf = rt::real(-1.0);
  for (;;) {
    // (a loop: an untraced ray ends at once, and a lane without a path must have used up its share of the chunk)
    while (!live && next < end) {
      live = start_ray_path(rp, ra, n, s_begin, next, samples, &ps);
      item = next;
      next += 64u;
      last_pdf = rt::real(-1.0);
    }
    if (wave_ballot(live) == 0ull) {  // the chunk is done: claim the next one
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(work_counter, TRACE_CHUNK);
      base = __shfl(base, 0, 64);
      if (base >= total) break;
      end = total - base < TRACE_CHUNK ? total : base + TRACE_CHUNK;
      next = base + lane;
      continue;
    }
    if (live) {
      bool done;
      if constexpr (NEE) done = rt::path_step_nee<F, false>(sv, lv, rp, &ps, &last_pdf, stack, (rt::TraceCounters*)nullptr);
      else done = rt::path_step<F, false>(sv, rp, &ps, stack, (rt::TraceCounters*)nullptr);
      if (done) {
        store_sample(samples, item, ps.output);
        live = false;
      }
    }
  }
}
