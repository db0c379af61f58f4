// k_trace_nee -- the trace kernel of next-event estimation (rtx_render_ex / rtx_progressive_create_ex with light_sampling = 1;
// included by render.hip, namespace rtx).
//
// The estimator is core/integrator.hpp's (path_step_nee: extension walk, scatter, light connection with its shadow walk, MIS),
// the same source the tests' host checker runs.  Scheduling follows the resident kernels: persistent waves claim TRACE_CHUNK
// items of the pass at a time through the pass's work counter; inside a chunk a lane whose path has ended takes the next item of
// the chunk at once (in-lane regeneration: items lane, lane + 64, ... of the chunk), so short paths do not wait for the wave's
// longest one until the chunk runs dry.  Walk stacks live in LDS (LdsStack, one column per thread).  Each lane alternates between
// the extension walk and the shadow walk of its own path.  Every item owns its slot of the pass's sample buffer (store_sample):
// k_reduce_samples, the noise statistics, adaptive retirement (ActiveMap), sharding and the denoiser see what any other trace
// kernel writes.
template <uint32_t F, class SM = ShardMap>
__global__ __launch_bounds__(TRACE_BLOCK) void k_trace_nee(rt::SceneView sv, rt::LightView lv, rt::RenderParams rp, SM sm,
                                                            uint32_t s_begin, uint32_t total,
                                                            double* __restrict__ samples, unsigned int* __restrict__ work_counter) {
  extern __shared__ int32_t lds_stack[];
  LdsStack stack;
  stack.base = lds_stack + threadIdx.x;
  stack.n = 0;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t next = 0, end = 0;  // this lane's next item of the wave's chunk; the chunk's end (wave-uniform)
  uint32_t item = 0;  // the live path's slot of the sample buffer
  bool live = false;
  rt::PathState ps;
  rt::real last_pdf = rt::real(-1.0);
  for (;;) {
    if (!live && next < end) {
      item = start_path(rp, sm, s_begin, next, &ps);
      next += 64u;
      last_pdf = rt::real(-1.0);
      live = true;
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
    if (live && rt::path_step_nee<F, false>(sv, lv, rp, &ps, &last_pdf, stack, (rt::TraceCounters*)nullptr)) {
      store_sample(samples, item, ps.output);
      live = false;
    }
  }
}
