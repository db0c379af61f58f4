// The wavefront (split-kernel) integrator: path state in HBM, one kernel per stage (included by render.hip, namespace rtx).
//
// SURVEY 8f-4's second half.  The resident kernels (k_trace_vote / k_trace_world) keep a whole path in registers and lose
// lanes wherever paths disagree about what to do next: on the dragon room the shading code runs with 41 of 64 lanes, node
// steps with 23, regeneration with 8, and the 128 registers that the path + walk + shading state need cap the kernel at
// 4 waves per SIMD while 51 % of its wave cycles wait for a dependent node fetch.  Here a pool of P path slots lives in
// HBM as structure-of-arrays and every bounce of every path is three launches:
//
//   k_wf_generate  free slots (a dense list) get the next samples of the pass: path_begin + the depth test of the
//                  first bounce, all lanes busy (world.rs:1211-1214, world.rs:64-67)
//   k_wf_trace     persistent waves pull slots, each lane walks ONE ray through the BVH with the voting walk of
//                  trace_vote.inc and writes (t, primitive); a lane whose walk is over takes the next slot as soon as
//                  `refill_min` lanes are free -- nothing but walk state is live, so more waves fit (bvh.rs:97-112)
//   k_wf_shade     one lane per slot: plain top-level primitives (the room's rectangles) in list order with
//                  HittableList's tie rule, HitRecord, scatter, emitted, the next bounce's depth test; an ended path
//                  writes its sample and puts its slot on the free list (hit.rs:660-690, world.rs:68-90)
//
// A path's stream, its draws and their order are those of every other kernel (the stream is keyed by (pixel, sample), the
// state just waits in HBM between stages), every sample owns its slot of the sample buffer, and the arithmetic is the same
// core code: the image is bit-identical (tests/test_gpu_wavefront.py).  What it costs is traffic: ~270 B per ray-bounce
// read + written (ray 48 + 56 + 48, hit 12 + 12, stream 16 + 16, product 24 + 24, depth / sample index 12).  `output` is
// only touched when a path that goes on has gathered light (never, with the reference's materials: the only emitter does
// not scatter), flagged in the depth word.
//
// No stage takes a contended atomic.  (The first version did -- one device-scope atomicAdd per wave for a global free list
// and one per 256 slots for the trace kernel's work counter, 85 000 per iteration on two addresses; removing them was worth
// 10 %: 93 -> 103 Msamples/s at 4 Mi slots.)  The pool is cut into segments of 1024 slots = one workgroup of the generate
// and shade kernels: a segment compacts its own ended slots (wave ballots + one LDS atomic per wave), refills them itself,
// and draws its samples from its own interleaved share of the pass (64-sample chunks dealt round-robin over the segments,
// so every segment sees the whole frame and they run dry together).  The trace kernel's waves take the pool's 64-slot
// chunks round-robin as well.
//
// Measured on the dragon room (profiles/r02/wavefront/): shading 4 Mi paths takes 0.26 ms and generation 0.11 ms -- both
// far cheaper than inside the resident kernel -- but every launch of k_wf_trace ends with its longest walk, ONE lane
// paying a full memory latency per node step (0.5 ms for the coherent first bounce, 0.9 - 7.7 ms for every later one),
// which the resident kernel hides behind the other paths of the wave.  Bigger pools amortise it (4 / 16 / 64 Mi slots:
// 103 / 200 / 323 Msamples/s) without reaching k_trace_vote's 829: the integrator stays an A/B alternative.
//
// Applies to the worlds k_trace_vote serves (one BVH + plain primitives).  RTX_TRACE_KERNEL=wavefront forces it where it
// applies, RTX_WF_PATHS sets P, RTX_WF_REFILL the refill threshold, RTX_WF_CHECK how often the host looks for the end.


constexpr uint32_t WF_FREE = 0xffffffffu;    // g[]: the slot holds no path
constexpr uint32_t WF_NOHIT = 0xffffffffu;   // hit_ref[]: the walk found nothing (PrimRef types end at 4: no clash)
constexpr uint32_t WF_ENDED = 0xfffffffeu;   // hit_ref[]: the path ended before its first query (shade only finalises it)
constexpr int32_t WF_HAS_OUTPUT = 1 << 30;   // depth[]: output[] holds something other than (0, 0, 0)
constexpr uint32_t WF_SEG = 1024u;           // slots per segment = threads per workgroup of k_wf_generate / k_wf_shade
constexpr uint32_t WF_DEAL = 64u;            // samples (and, in the trace kernel, slots) per round-robin chunk

// Pool traffic is streamed once per stage: non-temporal, so that it does not push the culling tree out of L2 / MALL.
template <class T> __device__ __forceinline__ T wf_ld(const T* p) { return __builtin_nontemporal_load(p); }
template <class T> __device__ __forceinline__ void wf_st(T* p, T v) { __builtin_nontemporal_store(v, p); }

struct WavePool {
  rt::real* ray;             // [7][P] origin xyz, direction xyz, time
  unsigned long long* rng;   // [2][P]
  rt::real* product;         // [3][P]
  rt::real* output;          // [3][P]
  int32_t* depth;            // [P] bounces left | WF_HAS_OUTPUT
  uint32_t* g;               // [P] the path's slot of the pass's sample buffer, WF_FREE
  rt::real* hit_t;           // [P]
  uint32_t* hit_ref;         // [P]
  uint32_t* free_list;       // [P]: segment b lists its free slots at [b * WF_SEG, b * WF_SEG + n_free[b])
  uint32_t* n_free;          // [P / WF_SEG]
  uint32_t* cursor;          // [P / WF_SEG] samples segment b has drawn from its share of the pass
  uint32_t* ctrl;            // [0] live paths (k_wf_count)
  uint32_t P;
};

__global__ void k_wf_init(WavePool pool) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < pool.P) { pool.g[s] = WF_FREE; pool.free_list[s] = s; }
  if (s < pool.P / WF_SEG) { pool.n_free[s] = WF_SEG; pool.cursor[s] = 0u; }
}

// Live paths of the pool (the host looks at this every few iterations to find the end of the pass).
__global__ __launch_bounds__(256) void k_wf_count(WavePool pool) {
  uint32_t n = 0;
  for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < pool.P; s += gridDim.x * blockDim.x) n += pool.g[s] != WF_FREE ? 1u : 0u;
  __shared__ uint32_t acc;
  if (threadIdx.x == 0) acc = 0u;
  __syncthreads();
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
  if ((threadIdx.x & 63u) == 0u) atomicAdd(&acc, n);
  __syncthreads();
  if (threadIdx.x == 0 && acc != 0u) atomicAdd(&pool.ctrl[0], acc);
}

// Segment b refills its free slots: its m-th sample is sample ((m / 64) * n_seg + b) * 64 + m % 64 of the pass.
template <class SM>
__global__ __launch_bounds__(WF_SEG) void k_wf_generate(WavePool pool, rt::RenderParams rp, SM sm, uint32_t s_begin, uint32_t total) {
  const uint32_t b = blockIdx.x, k = threadIdx.x, n_seg = gridDim.x;
  const uint32_t n_free = pool.n_free[b], cur = pool.cursor[b];
  if (n_free == 0u) return;
  __syncthreads();  // everyone has read the two words
  if (k == 0) { pool.cursor[b] = cur + n_free; pool.n_free[b] = 0u; }  // samples past the end of the pass are drawn, and dropped, too
  if (k >= n_free) return;
  const uint32_t m = cur + k;
  const unsigned long long g64 = ((unsigned long long)(m / WF_DEAL) * n_seg + b) * WF_DEAL + (m % WF_DEAL);
  if (g64 >= (unsigned long long)total) return;  // the segment's share is used up: the slot stays free (and off the list)
  const uint32_t g = (uint32_t)g64;
  const uint32_t P = pool.P;
  const uint32_t slot = pool.free_list[b * WF_SEG + k];
  rt::PathState ps;
  const uint32_t sample_slot = start_path(rp, sm, s_begin, g, &ps);
  const bool ended = rt::path_bounce_begin(&ps);  // world.rs:64-67 (max_depth >= 1: never at birth in f64)
  pool.ray[0 * (size_t)P + slot] = ps.ray.origin.x; pool.ray[1 * (size_t)P + slot] = ps.ray.origin.y; pool.ray[2 * (size_t)P + slot] = ps.ray.origin.z;
  pool.ray[3 * (size_t)P + slot] = ps.ray.direction.x; pool.ray[4 * (size_t)P + slot] = ps.ray.direction.y; pool.ray[5 * (size_t)P + slot] = ps.ray.direction.z;
  pool.ray[6 * (size_t)P + slot] = ps.ray.time;
  pool.rng[slot] = ps.rng.s0; pool.rng[(size_t)P + slot] = ps.rng.s1;
  pool.product[slot] = ps.product.x; pool.product[(size_t)P + slot] = ps.product.y; pool.product[2 * (size_t)P + slot] = ps.product.z;
  pool.depth[slot] = ps.depth < 0 ? 0 : ps.depth;
  pool.hit_ref[slot] = ended ? WF_ENDED : WF_NOHIT;
  pool.g[slot] = sample_slot;
}

// The BVH query of every live slot.
template <uint32_t F, bool WIDE, int MIN_BLOCKS>
__global__ __launch_bounds__(TRACE_BLOCK, MIN_BLOCKS) void k_wf_trace(rt::SceneView sv, WavePool pool, uint32_t leaf_weight, uint32_t refill_min,
                                                                     uint32_t bvh_pos, const FlatNode4* __restrict__ nodes4, int32_t tri_base) {
  extern __shared__ int32_t lds_stack[];
  LdsStack stack;
  stack.base = lds_stack + threadIdx.x;
  stack.n = 0;
  const uint32_t P = pool.P;
  const rt::FlatEntry& bvh = sv.entries[sv.top_level[bvh_pos]];
  const int32_t root = bvh.a;
  const uint32_t first_ref = (uint32_t)bvh.b;
  // this wave's share of the pool: the 64-slot chunks c with c % n_waves == wave (wave-uniform bookkeeping)
  const uint32_t n_waves = gridDim.x * (TRACE_BLOCK / 64u), n_chunks = P / WF_DEAL;
  uint32_t chunk = blockIdx.x * (TRACE_BLOCK / 64u) + (threadIdx.x >> 6);
  uint32_t chunk_pos = 0;   // slots of `chunk` already handed out
  bool queue_empty = chunk >= n_chunks;
  uint32_t slot = WF_FREE;  // the slot whose ray this lane walks
  rt::Ray ray = rt::make_ray(rt::v3(0, 0, 0), rt::v3(0, 0, 0), 0);
  rt::Ray32 q = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  uint32_t dir_neg = 0;
  float t_max32 = 0.f;
  int32_t cur = WALK_DONE;
  rt::Closest best;
  best.t = 0.0; best.ref = 0; best.order = 0; best.hit = false;
  for (;;) {
    // ---- lanes without a ray take the next slots once enough of them wait
    const unsigned long long need_mask = wave_ballot(slot == WF_FREE);
    const uint32_t n_need = (uint32_t)__popcll(need_mask);
    if (!queue_empty && n_need >= refill_min) {
      const uint32_t rank = lane_rank(need_mask);
      const uint32_t avail = WF_DEAL - chunk_pos;
      if (slot == WF_FREE && rank < avail) {
        const uint32_t s = chunk * WF_DEAL + chunk_pos + rank;
        // all loads of the refill in flight together (the ray of a free slot is stale data that is never used)
        const uint32_t gs = wf_ld(&pool.g[s]), hr = wf_ld(&pool.hit_ref[s]);
        const rt::real ox = wf_ld(&pool.ray[s]), oy = wf_ld(&pool.ray[(size_t)P + s]), oz = wf_ld(&pool.ray[2 * (size_t)P + s]);
        const rt::real dx = wf_ld(&pool.ray[3 * (size_t)P + s]), dy = wf_ld(&pool.ray[4 * (size_t)P + s]), dz = wf_ld(&pool.ray[5 * (size_t)P + s]);
        const rt::real tm = (F & (rt::F_MOVING_SPHERE | rt::F_GRAVITY_SPHERE)) ? wf_ld(&pool.ray[6 * (size_t)P + s]) : rt::real(0);
        if (gs != WF_FREE && hr != WF_ENDED) {
          slot = s;
          ray = rt::make_ray(rt::v3(ox, oy, oz), rt::v3(dx, dy, dz), tm);
          q = rt::make_ray32(ray, rt::ray_t_min(ray));
          dir_neg = WIDE ? wide_sign_pack(ray) : rt::ray_dir_neg(ray);
          t_max32 = __builtin_huge_valf();
          best.t = RT_INFINITY; best.hit = false; best.ref = 0; best.order = 0;
          stack.reset();
          cur = root;
        }
      }
      chunk_pos += (n_need < avail) ? n_need : avail;
      if (chunk_pos >= WF_DEAL) {
        chunk += n_waves; chunk_pos = 0;
        queue_empty = chunk >= n_chunks;
      }
    }
    if (wave_ballot(slot != WF_FREE) == 0ull) {
      if (queue_empty) break;
      continue;  // every slot handed out was free: take the next ones (n_need is 64 >= refill_min)
    }
    // ---- walk: cost-weighted node / leaf vote, until `refill_min` lanes are free again (or, with nothing left to take, to the end)
    const uint32_t threshold = queue_empty ? 1u : 65u - refill_min;
    for (;;) {
      const bool is_leaf = cur < 0;
      const bool is_node = (uint32_t)cur < (uint32_t)WALK_DONE;
      const unsigned long long m_node = wave_ballot(is_node), m_leaf = wave_ballot(is_leaf);
      if ((uint32_t)__popcll(m_node | m_leaf) < threshold) break;
      if ((uint32_t)__popcll(m_node) * leaf_weight >= (uint32_t)__popcll(m_leaf)) {
        if (is_node) {
          if (WIDE) walk_node_step4(nodes4, q, dir_neg, t_max32, &cur, stack);
          else walk_node_step32(sv.nodes32[cur], q, dir_neg, t_max32, &cur, stack);
        }
      } else if (is_leaf) {
        walk_leaf_step<F>(sv, first_ref, ray, rt::ray_t_min(ray), &best, &cur, stack, tri_base);
        t_max32 = rt::cull_round_up(best.t);
      }
    }
    // ---- finished walks hand their answer to the shading stage
    if (slot != WF_FREE && cur == WALK_DONE) {
      wf_st(&pool.hit_t[slot], best.t);
      wf_st(&pool.hit_ref[slot], best.hit ? (uint32_t)best.ref : WF_NOHIT);
      slot = WF_FREE;
    }
  }
}

// The rest of HittableList::hit and of ray_color's loop body for every live slot of segment blockIdx.x.
template <uint32_t F>
__global__ __launch_bounds__(WF_SEG) void k_wf_shade(rt::SceneView sv, WavePool pool, rt::RenderParams rp, double* __restrict__ samples,
                                                     uint32_t bvh_pos) {
  __shared__ uint32_t seg_free;
  if (threadIdx.x == 0) seg_free = 0u;
  __syncthreads();
  const uint32_t s = blockIdx.x * WF_SEG + threadIdx.x;
  const uint32_t P = pool.P;
  const uint32_t g = wf_ld(&pool.g[s]);
  bool ended = false;
  if (g != WF_FREE) {
    rt::PathState ps;
    const uint32_t href = wf_ld(&pool.hit_ref[s]);
    const int32_t dword = wf_ld(&pool.depth[s]);
    ps.depth = dword & ~WF_HAS_OUTPUT;
    ps.output = rt::v3(0, 0, 0);
    if (dword & WF_HAS_OUTPUT) ps.output = rt::v3(pool.output[s], pool.output[(size_t)P + s], pool.output[2 * (size_t)P + s]);
    if (href == WF_ENDED) {
      ended = true;
    } else {
      ps.ray = rt::make_ray(rt::v3(wf_ld(&pool.ray[s]), wf_ld(&pool.ray[(size_t)P + s]), wf_ld(&pool.ray[2 * (size_t)P + s])),
                            rt::v3(wf_ld(&pool.ray[3 * (size_t)P + s]), wf_ld(&pool.ray[4 * (size_t)P + s]), wf_ld(&pool.ray[5 * (size_t)P + s])),
                            wf_ld(&pool.ray[6 * (size_t)P + s]));
      ps.rng.s0 = wf_ld(&pool.rng[s]); ps.rng.s1 = wf_ld(&pool.rng[(size_t)P + s]);
      ps.product = rt::v3(wf_ld(&pool.product[s]), wf_ld(&pool.product[(size_t)P + s]), wf_ld(&pool.product[2 * (size_t)P + s]));
      rt::Closest best;
      best.hit = href != WF_NOHIT;
      best.t = best.hit ? wf_ld(&pool.hit_t[s]) : RT_INFINITY;
      best.ref = best.hit ? (rt::PrimRef)href : 0;
      best.order = 0;
      if (F & rt::F_PRIM_ENTRY) {
        // Plain primitives beside the BVH in the top-level list, in list order; the LATER entry wins an exact tie
        // (hit.rs:660-690), wherever the BVH sits in the list -- the block k_trace_vote runs after its walk.
        int32_t win_entry = best.hit ? (int32_t)bvh_pos : -1;
        for (int32_t k = 0; k < sv.n_top_level; ++k) {
          if (k == (int32_t)bvh_pos) continue;
          const rt::FlatEntry* e = &sv.entries[dev_load_uniform(&sv.top_level[k])];
          const rt::PrimRef ref = (rt::PrimRef)dev_load_uniform(&e->a);
          rt::real t;
          if (rt::prim_t<F, false>(sv, ref, ps.ray, rt::ray_t_min(ps.ray), best.t, &t, nullptr)) {
            if (t < best.t || win_entry < k) { best.t = t; best.ref = ref; best.hit = true; win_entry = k; }
          }
        }
      }
      rt::HitRecord rec;
      if (best.hit) rt::prim_finalize<F>(sv, best.ref, ps.ray, best.t, &rec);
      ended = rt::path_bounce_end<F, false>(sv, rp, &ps, best.hit, rec, nullptr);
      if (!ended) ended = rt::path_bounce_begin(&ps);  // the next bounce's depth test (world.rs:64-67)
      if (!ended) {
        wf_st(&pool.ray[s], ps.ray.origin.x); wf_st(&pool.ray[(size_t)P + s], ps.ray.origin.y); wf_st(&pool.ray[2 * (size_t)P + s], ps.ray.origin.z);
        wf_st(&pool.ray[3 * (size_t)P + s], ps.ray.direction.x); wf_st(&pool.ray[4 * (size_t)P + s], ps.ray.direction.y); wf_st(&pool.ray[5 * (size_t)P + s], ps.ray.direction.z);
        wf_st(&pool.rng[s], (unsigned long long)ps.rng.s0); wf_st(&pool.rng[(size_t)P + s], (unsigned long long)ps.rng.s1);
        wf_st(&pool.product[s], ps.product.x); wf_st(&pool.product[(size_t)P + s], ps.product.y); wf_st(&pool.product[2 * (size_t)P + s], ps.product.z);
        // x + (+-0) == x and a sum of zeros that starts at +0 stays +0: an all-zero output need not be stored
        const bool has_out = !(ps.output.x == rt::real(0) && ps.output.y == rt::real(0) && ps.output.z == rt::real(0));
        if (has_out) { pool.output[s] = ps.output.x; pool.output[(size_t)P + s] = ps.output.y; pool.output[2 * (size_t)P + s] = ps.output.z; }
        wf_st(&pool.depth[s], ps.depth | (has_out ? WF_HAS_OUTPUT : 0));
      }
    }
    if (ended) {
      store_sample(samples, g, ps.output);
      pool.g[s] = WF_FREE;
    }
  }
  // ---- ended paths put their slots on the segment's list (one LDS atomic per wave)
  const unsigned long long m = wave_ballot(ended);
  if (m != 0ull) {
    const uint32_t lane = threadIdx.x & 63u;
    const int leader = (int)__builtin_ctzll(m);
    uint32_t base = 0;
    if (lane == (uint32_t)leader) base = atomicAdd(&seg_free, (uint32_t)__popcll(m));
    base = __builtin_amdgcn_readlane(base, leader);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (ended) pool.free_list[blockIdx.x * WF_SEG + base + rank] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) pool.n_free[blockIdx.x] = seg_free;
}
