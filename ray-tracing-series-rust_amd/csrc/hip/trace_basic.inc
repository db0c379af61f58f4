// Kernel feature presets and the grid-stride trace kernel (included by render.hip, namespace rtx).

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
constexpr uint32_t P_ALL = rt::F_ALL & ~rt::F_INSTANCE;          // everything, GravitySphere included (k_trace_simple, scene 8)
constexpr uint32_t P_ANY = P_ALL & ~rt::F_GRAVITY_SPHERE;        // any world of the catalogue's BASELINE scenes
// P_ALL plus the walk of instance trees: the preset of every world that holds one (a preset without F_INSTANCE scans the
// members as plain slots -- the same frame, O(members) per ray).  Its own preset so that no P_ALL kernel carries the walk.
constexpr uint32_t P_INST = rt::F_ALL;
static_assert(P_ALL == (1u << 20) - 1u, "the presets of worlds without instance trees are what they were before F_INSTANCE");

// Straightforward form: grid-stride over the pass's (sample, pixel) index space (pass_items.inc), one whole
// path per loop iteration.
// Kept as the instrumented (COUNT) build and as the plainest kernel to force (RTX_TRACE_KERNEL=simple).
template <uint32_t F, bool COUNT, class SM = ShardMap>
__global__ __launch_bounds__(TRACE_BLOCK) void k_trace_simple(rt::SceneView sv, rt::RenderParams rp,
                                                               SM sm, uint32_t s_begin,
                                                               uint32_t total,
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
    uint32_t i, j, s_local;
    const uint32_t slot = item_pixel(sm, g, &i, &j, &s_local);
    store_sample(samples, slot, rt::trace_sample<F, COUNT>(sv, rp, i, j, s_begin + s_local, stack, &cnt));
  }
  if (COUNT) flush_counters(cnt, counters);
}
