// k_gather, k_reduce_samples_sh -- light arriving at a caller's points on a resident scene (rtx_scene_gather*; included by
// render.hip, namespace rtx, so compiled for both precisions; DESIGN.md section 7.6).
//
// A pass is k_trace_rays' index space with the batch's points in the place of its rays, in the order of core/item_order.hpp
// (the launcher's GATHER_ITEM_GROUP points a group, sample-major inside a group: a wave's 64 consecutive items are many samples
// of few points); item g is sample s_begin + s_local of point r and owns the slot s_local * n + r.  The path of an item is
// core/integrator.hpp's path_begin_gather -- the stream of (seed, first_point + r, sample), whose first draws give the start
// direction: normal + unit vector (SURFACE, Lambertian::scatter's rule) or the unit vector itself (the probe form) -- followed by
// path_step (NEE: path_step_nee; NEE and SURFACE: the start vertex' light connection first, path_begin_gather_nee), the source
// the tests' host checker runs.  Scheduling is k_trace_rays': persistent waves claim TRACE_CHUNK items through the pass's work
// counter, a lane whose path has ended takes the next item of the chunk at once, walk stacks live in LDS.  Every item owns its
// slot of the pass's sample buffer (store_sample: 3 doubles an item, whatever the output), and k_reduce_samples /
// k_reduce_samples_moments add the pass onto the caller's plain sums in sample order.
//
// Points come in as k_cast_rays takes its rays: [n][3] f64 columns read as three strided accesses per lane (cast_rays.inc says
// what that costs and why no LDS staging), an optional [n] time column; the f32 compilation narrows each component with a (real)
// cast.  A point whose time is past time_limit (scenes with GravitySpheres) is not traced: its sample is stored as NaN.
//
// Spherical-harmonic output does not widen the sample buffer: k_reduce_samples_sh draws dir_s again -- the first draws of the
// sample's stream, in this compilation's precision, exactly what the path drew -- and adds Y_i(dir_s) * L_s[c] for s ascending,
// i = 0 .. K-1, c = 0 .. 2 (core/sh_basis.hpp; double arithmetic, every operation separately rounded).
#include "../core/sh_basis.hpp"

// A launch's points (device pointers) -- a kernel argument, so every test on it is wave-uniform.
struct GatherArgs {
  const double* position;   // [n][3]
  const double* normal;     // [n][3]; NULL in the probe form (never read there)
  const double* time;       // [n] or NULL
  double time_limit;        // scenes with GravitySpheres: a point later than this is not traced (DeviceScene::gravity_time_limit)
  uint64_t first_point;     // index of the launch's point 0 in the caller's whole batch: the stream key's pixel word
};

// Starts item g's path and returns its slot of the sample buffer through *slot.  false: the point is not traced and its sample is
// already stored (NaN).
template <uint32_t F, bool NEE, bool SURFACE>
__device__ __forceinline__ bool start_gather_path(const rt::SceneView& sv, const rt::LightView& lv, const rt::RenderParams& rp,
                                                  const GatherArgs& a, const rt::ItemOrder& order, uint32_t s_begin, uint32_t g,
                                                  double* samples, rt::PathState* ps, rt::real* last_pdf, LdsStack& stack,
                                                  uint32_t* slot) {
  uint32_t r, s_local;
  *slot = rt::item_order_map(order, g, &r, &s_local);
  double p[3], nn[3] = {0.0, 0.0, 0.0};
  for (int c = 0; c < 3; ++c) p[c] = a.position[3 * (size_t)r + c];
  if constexpr (SURFACE) {
    for (int c = 0; c < 3; ++c) nn[c] = a.normal[3 * (size_t)r + c];
  }
  const double time = a.time ? a.time[r] : 0.0;
  if (time > a.time_limit) {
    const double nan = __builtin_nan("");
    double* out = samples + 3 * (size_t)*slot;
    out[0] = nan; out[1] = nan; out[2] = nan;
    return false;
  }
  const rt::Point3 pos = rt::v3((rt::real)p[0], (rt::real)p[1], (rt::real)p[2]);
  const rt::Vec3 normal = rt::v3((rt::real)nn[0], (rt::real)nn[1], (rt::real)nn[2]);
  *last_pdf = rt::real(-1.0);
  if constexpr (NEE && SURFACE)
    rt::path_begin_gather_nee<F, false>(sv, lv, rp, pos, normal, (rt::real)time, a.first_point + (uint64_t)r, s_begin + s_local, ps,
                                        last_pdf, stack, (rt::TraceCounters*)nullptr);
  else
    rt::path_begin_gather(rp, pos, normal, SURFACE, (rt::real)time, a.first_point + (uint64_t)r, s_begin + s_local, ps);
  return true;
}

template <uint32_t F, bool NEE, bool SURFACE>
__global__ __launch_bounds__(TRACE_BLOCK) void k_gather(rt::SceneView sv, rt::LightView lv, rt::RenderParams rp, GatherArgs ga,
                                                         rt::ItemOrder order, uint32_t s_begin, uint32_t total,
                                                         double* __restrict__ samples, unsigned int* __restrict__ work_counter) {
  extern __shared__ int32_t lds_stack[];
  LdsStack stack;
  stack.base = lds_stack + threadIdx.x;
  stack.n = 0;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t next = 0, end = 0;  // this lane's next item of the wave's chunk; the chunk's end (wave-uniform)
  uint32_t slot = 0;  // of the live path's sample
  bool live = false;
  rt::PathState ps;
  rt::real last_pdf = rt::real(-1.0);
  for (;;) {
    // (a loop: an untraced point ends at once, and a lane without a path must have used up its share of the chunk)
    while (!live && next < end) {
      live = start_gather_path<F, NEE, SURFACE>(sv, lv, rp, ga, order, s_begin, next, samples, &ps, &last_pdf, stack, &slot);
      next += 64u;
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
        store_sample(samples, slot, ps.output);
        live = false;
      }
    }
  }
}

// One lane per point: the pass's samples projected onto the K = (ORDER + 1)^2 basis functions and added in ascending sample
// order onto sum[n][K][3] (and their squares onto sumsq unless NULL).  dir_s is drawn again from the sample's stream.
template <int ORDER>
__global__ __launch_bounds__(256) void k_reduce_samples_sh(const double* __restrict__ samples, double* __restrict__ sum,
                                                           double* __restrict__ sumsq, uint32_t n, uint32_t s_count, int first_pass,
                                                           uint64_t seed, uint64_t first_point, uint32_t s_begin) {
#pragma clang fp contract(off)
  constexpr int K = (ORDER + 1) * (ORDER + 1);
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  double S[3 * K], Q[3 * K];
  double* gs = sum + (size_t)(3 * K) * r;
  double* gq = sumsq ? sumsq + (size_t)(3 * K) * r : nullptr;
  for (int k = 0; k < 3 * K; ++k) {
    S[k] = first_pass ? 0.0 : gs[k];
    Q[k] = (first_pass || !gq) ? 0.0 : gq[k];
  }
  for (uint32_t s = 0; s < s_count; ++s) {
    const double* x = samples + 3 * ((size_t)s * n + r);
    const double L[3] = {x[0], x[1], x[2]};
    const rt::Vec3 d = rt::gather_sample_direction(seed, first_point + (uint64_t)r, s_begin + s, false, rt::v3(0, 0, 0));
    double Y[K];
    sh_basis_eval(ORDER, (double)d.x, (double)d.y, (double)d.z, Y);
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double v = __dmul_rn(Y[i], L[c]);
        S[3 * i + c] = __dadd_rn(S[3 * i + c], v);
        Q[3 * i + c] = __dadd_rn(Q[3 * i + c], __dmul_rn(v, v));
      }
  }
  for (int k = 0; k < 3 * K; ++k) {
    gs[k] = S[k];
    if (gq) gq[k] = Q[k];
  }
}

// rtx_gather_directions in this compilation's arithmetic (host only): dir [n][samples][3], widened.
static void gather_directions_impl(const RtxGatherPoints* g, double* dir) {
  for (int64_t r = 0; r < g->n; ++r) {
    rt::Vec3 normal = rt::v3(0, 0, 0);
    if (g->normal) normal = rt::v3((rt::real)g->normal[3 * r], (rt::real)g->normal[3 * r + 1], (rt::real)g->normal[3 * r + 2]);
    for (int32_t s = 0; s < g->samples; ++s) {
      const rt::Vec3 d = rt::gather_sample_direction(g->seed, g->first_point + (uint64_t)r, g->first_sample + (uint32_t)s,
                                                     g->normal != nullptr, normal);
      double* o = dir + 3 * ((size_t)r * (size_t)g->samples + (size_t)s);
      o[0] = (double)d.x; o[1] = (double)d.y; o[2] = (double)d.z;
    }
  }
}
