// Grid-stride and persistent trace kernels (included by render.hip, namespace rtx).

// ------------------------------------------------------------------ kernels
// Feature presets the trace kernels are compiled for (see core/flat_types.hpp Feature).
constexpr uint32_t P_SPHERES = rt::F_SPHERE | rt::F_MOVING_SPHERE | rt::F_BVH | rt::F_LAMBERTIAN |
                               rt::F_METAL | rt::F_DIELECTRIC | rt::F_CHECKER;
// P_SPHERES without moving spheres and checker textures: the Book-1 final scene exactly.  Code a scene cannot reach
// costs registers even when it never runs (measured: C2 +5 % from shrinking the unreachable checker code).
constexpr uint32_t P_STATIC_SPHERES = rt::F_SPHERE | rt::F_BVH | rt::F_LAMBERTIAN | rt::F_METAL | rt::F_DIELECTRIC;
constexpr uint32_t P_MESH = rt::F_SPHERE | rt::F_RECT | rt::F_TRIANGLE | rt::F_PRIM_ENTRY | rt::F_GROUP |
                            rt::F_BVH | rt::F_LAMBERTIAN | rt::F_METAL | rt::F_DIELECTRIC | rt::F_LIGHT;
// P_MESH without spheres, ordered groups and dielectrics: the dragon room exactly.
constexpr uint32_t P_MESH_ROOM = rt::F_RECT | rt::F_TRIANGLE | rt::F_PRIM_ENTRY | rt::F_BVH | rt::F_LAMBERTIAN | rt::F_METAL | rt::F_LIGHT;
constexpr uint32_t P_ALL = rt::F_ALL;                            // everything, GravitySphere included (k_trace_simple, scene 8)
constexpr uint32_t P_ANY = rt::F_ALL & ~rt::F_GRAVITY_SPHERE;    // any world of the catalogue's BASELINE scenes

// Straightforward form: grid-stride over the pass's (sample, pixel) index space (pass_items.inc), one whole
// path per loop iteration.
// Kept as the A/B partner of k_trace_persistent (RTX_TRACE_KERNEL=simple) and as the
// instrumented (COUNT) build.
template <uint32_t F, bool COUNT>
__global__ __launch_bounds__(TRACE_BLOCK) void k_trace_simple(rt::SceneView sv, rt::RenderParams rp,
                                                               ShardMap sm, uint32_t s_begin,
                                                               uint32_t total, uint32_t npix,
                                                               double* __restrict__ samples,
                                                               rt::TraceCounters* counters) {
  extern __shared__ int32_t lds_stack[];
  LdsStack stack;
  stack.base = lds_stack + threadIdx.x;
  stack.n = 0;
  rt::TraceCounters cnt;
  if (COUNT) memset(&cnt, 0, sizeof(cnt));
  for (uint64_t g64 = (uint64_t)blockIdx.x * TRACE_BLOCK + threadIdx.x; g64 < total;
       g64 += (uint64_t)gridDim.x * TRACE_BLOCK) {
    const uint32_t g = (uint32_t)g64;
    uint32_t i, j;
    const uint32_t s_local = item_pixel(sm, npix, g, &i, &j);
    store_sample(samples, g, rt::trace_sample<F, COUNT>(sv, rp, i, j, s_begin + s_local, stack, &cnt));
  }
  if (COUNT) flush_counters(cnt, counters);
}

template <bool WIDE> struct VoteWalkT;  // wave-cooperative BVH walker, defined with the voting walk below

// Persistent waves with path regeneration.  Waves pull TRACE_CHUNK-item chunks of the pass's
// index space (pass_items.inc) from a global counter and hand items to their lanes as lanes
// finish paths: every loop iteration the lanes without a path are compacted with a 64-bit
// __ballot and ranked with mbcnt (the wavefront prefix sum), take consecutive items
// (= consecutive pixels of one sample: coherent camera rays) and start a new path, then ALL
// lanes advance their path by one bounce.  A lane therefore never idles while the queue has
// work, whatever the length of its neighbours' paths.
// WIDE: sv_in.nodes carries the 4-wide culling tree (FlatNode4, see below) instead of the f64 binary tree, which
// this kernel never reads.
template <uint32_t F, bool WIDE>
__global__ __launch_bounds__(TRACE_BLOCK, (F == P_ANY ? 3 : 1)) void k_trace_persistent(rt::SceneView sv_in, rt::RenderParams rp,
                                                                   ShardMap sm, uint32_t s_begin,
                                                                   uint32_t total, uint32_t npix,
                                                                   double* __restrict__ samples,
                                                                   unsigned int* __restrict__ work_counter,
                                                                   const rt::FlatEntry* __restrict__ entries_ro,
                                                                   const int32_t* __restrict__ top_level_ro,
                                                                   const rt::FlatSphere* __restrict__ spheres_ro,
                                                                   const rt::FlatMovingSphere* __restrict__ msph_ro,
                                                                   const rt::FlatRect* __restrict__ rects_ro,
                                                                   const rt::FlatTriangle* __restrict__ tris_ro,
                                                                   const rt::FlatMaterial* __restrict__ mats_ro,
                                                                   const rt::FlatTexture* __restrict__ tex_ro,
                                                                   const rt::PrimRef* __restrict__ refs_ro) {
  // The world table is read through `const __restrict__` kernel parameters: that is what lets the
  // compiler prove the kernel's own stores cannot clobber it and fetch the (wave-uniform) entries with
  // scalar loads -- one s_load per wave instead of 64 identical vector loads per lane.
  rt::SceneView sv = sv_in;
  sv.entries = entries_ro;
  sv.top_level = top_level_ro;
  sv.spheres = spheres_ro; sv.moving_spheres = msph_ro; sv.rects = rects_ro; sv.triangles = tris_ro;
  sv.materials = mats_ro; sv.textures = tex_ro; sv.refs = refs_ro;
  extern __shared__ int32_t lds_stack[];
  LdsStack stack;
  stack.base = lds_stack + threadIdx.x;
  stack.n = 0;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t chunk_pos = 0, chunk_end = 0;  // wave-uniform
  bool queue_empty = false;               // wave-uniform
  bool active = false;
  uint32_t g = 0;
  rt::PathState ps;
  for (;;) {
    unsigned long long need_mask = wave_ballot(!active);
    if (need_mask != 0ull) {
      if (chunk_pos >= chunk_end && !queue_empty) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(work_counter, TRACE_CHUNK);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= total) {
          queue_empty = true;
        } else {
          chunk_pos = base;
          chunk_end = (total - base < TRACE_CHUNK) ? total : base + TRACE_CHUNK;
        }
      }
      if (chunk_pos < chunk_end) {
        uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need_mask >> 32),
                                                  __builtin_amdgcn_mbcnt_lo((uint32_t)need_mask, 0u));
        uint32_t n_need = (uint32_t)__popcll(need_mask);
        uint32_t avail = chunk_end - chunk_pos;
        if (!active && rank < avail) {
          g = chunk_pos + rank;
          start_path(rp, sm, npix, s_begin, g, &ps);
          active = true;
        }
        chunk_pos += (n_need < avail) ? n_need : avail;
      }
    }
    if (wave_ballot(active) == 0ull) break;  // queue drained and every lane's path has ended
    if (active) {
      if (rt::path_step<F, false, LdsStack, VoteWalkT<WIDE>>(sv, rp, &ps, stack, nullptr)) {
        store_sample(samples, g, ps.output);
        active = false;
      }
    }
  }
}
