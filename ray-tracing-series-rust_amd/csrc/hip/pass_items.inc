// A pass's index space as the trace kernels see it (included by render.hip, namespace rtx): item -> pixel and path, the
// sample store, the persistent kernels' work counter (chunk size, claim), a lane's rank in a wave mask and the size of the
// per-wave primary-ray ring.
//
// A pass of `total` items is one index space [0, total).  Which (pixel, sample) pair item g is -- the ORDER of the pass -- is
// core/item_order.hpp's: groups of P consecutive local pixels, sample-major inside a group (PassMap::order, prepared per pass
// by the launcher, in device memory).  With P >= npix item g = s_local * npix + lp is sample s_begin + s_local of the shard's local pixel lp, so
// 64 consecutive items are 64 consecutive pixels of one sample; with a small P they are many samples of few pixels.  The
// sample's SLOT in the sample buffer is s_local * npix + lp whatever the order.  Which lane traces an item cannot matter:
// streams are keyed by (pixel, sample) and every item owns its output slot.  A lane carries the slot, not the item.
//
// An adaptive pass (progressive.inc) traces only the shard's still-active pixels: its map is an ActiveMap, whose list holds
// their local pixels in ascending order, and npix is then the length of that list -- slot s_local * npix + k is sample
// s_begin + s_local of local pixel active[k], and the order's groups are runs of P list entries.  The list is ascending, so
// neighbouring entries are still mostly neighbouring pixels.  The map's type is a template parameter of every trace kernel (SM, default ShardMap): a uniform
// pass's instantiation has neither the list nor a test for it -- a runtime test on a kernel argument cost 0.4 - 1.6 % on the
// k_trace_lds and k_trace_world legs of bench.py, through the kernels' register assignment.

// What turns an item of a pass into a pixel and a sample: the pass's item order, and the shard's map from a local pixel lp to
// the image (column i, row j).  Rows of a shard are the rows j with (j / block_rows) % shard_count == shard_index, compacted in
// ascending j.  One record per pass in device memory, written by k_pass_begin; the divisions by width and block_rows are
// prepared like the order's (rt::Div32).
struct PassMap {
  rt::ItemOrder order;
  rt::Div32 width, block_rows;
  uint32_t shard_index, shard_count;
};
constexpr uint32_t PASS_MAP_DWORDS = rt::ITEM_ORDER_DWORDS + 10u;
static_assert(sizeof(PassMap) == PASS_MAP_DWORDS * 4u, "item_pixel reads it dword by dword");
// The map as a trace kernel's argument.
struct ShardMap {
  const PassMap* pass;
};
struct ActiveMap : ShardMap {
  const uint32_t* active;  // the pass's active local pixels, ascending
};
__device__ __forceinline__ uint32_t map_pixel(const ShardMap&, uint32_t k) { return k; }
__device__ __forceinline__ uint32_t map_pixel(const ActiveMap& m, uint32_t k) { return m.active[k]; }
__device__ __forceinline__ void shard_pixel(const PassMap& m, uint32_t lp, uint32_t* i, uint32_t* j) {
  const uint32_t lr = rt::div32(lp, m.width.m, m.width.sh1, m.width.sh2);
  *i = lp - lr * m.width.d;
  const uint32_t k = rt::div32(lr, m.block_rows.m, m.block_rows.sh1, m.block_rows.sh2);
  const uint32_t within = lr - k * m.block_rows.d;
  *j = (k * m.shard_count + m.shard_index) * m.block_rows.d + within;
}

// Item g of the pass -> image pixel (i, j) and the item's sample index within the pass; returns the sample's slot.
// The pass's constants are read HERE, into VECTOR registers (every lane loads the same words), through a pointer the compiler
// takes for a lane's own.  k_trace_lds has no scalar registers to spare: as kernel arguments the order's constants sat in
// them for the whole kernel and pushed 27 other values into lanes of a spill register, and as scalar loads where a path starts
// they still pushed out 10, read back once per bounce.  Vector registers are free where a path starts.  What the trace kernels
// keep for the whole pass is the pointer's register pair; the shard's four numbers and the pixel count no longer need any.
// SCALAR (wide k_trace_vote, which starts paths in the lane with as few as 8 lanes waiting and is bound by latency): the same
// words through the scalar cache, each moved to a vector register at once -- a scalar load that hits returns several times
// sooner than a vector load that has to go to L2, and the scalar registers are given back before the path begins.
template <bool SCALAR = false, class SM>
__device__ __forceinline__ uint32_t item_pixel(const SM& sm, uint32_t g, uint32_t* i, uint32_t* j, uint32_t* s_local) {
  typedef const __attribute__((address_space(1))) uint32_t GlobalU32;
  typedef const __attribute__((address_space(4))) uint32_t ConstU32;
  const PassMap* pp = sm.pass;
  uint32_t dw[PASS_MAP_DWORDS];
  if (SCALAR) {
    asm volatile("" : "+s"(pp));
    ConstU32* w = (ConstU32*)pp;
    for (uint32_t k = 0; k < PASS_MAP_DWORDS; ++k) { uint32_t v = w[k]; asm volatile("" : "+v"(v)); dw[k] = v; }
  } else {
    asm volatile("" : "+v"(pp));
    GlobalU32* w = (GlobalU32*)pp;
    for (uint32_t k = 0; k < PASS_MAP_DWORDS; ++k) dw[k] = w[k];
  }
  PassMap pm;
  __builtin_memcpy(&pm, dw, sizeof(pm));
  uint32_t lp;
  const uint32_t slot = rt::item_order_map(pm.order, g, &lp, s_local);
  shard_pixel(pm, map_pixel(sm, lp), i, j);
  return slot;
}

// The camera ray and RNG stream of item g (path_begin, core/integrator.hpp); returns the sample's slot.
template <bool SCALAR = false, class SM>
__device__ __forceinline__ uint32_t start_path(const rt::RenderParams& rp, const SM& sm, uint32_t s_begin, uint32_t g,
                                               rt::PathState* ps) {
  uint32_t i, j, s_local;
  const uint32_t slot = item_pixel<SCALAR>(sm, g, &i, &j, &s_local);
  rt::path_begin(rp, i, j, s_begin + s_local, ps);
  return slot;
}

// A sample's radiance into its slot of the pass's sample buffer (k_reduce_samples adds it onto the accumulator in sample order).
__device__ __forceinline__ void store_sample(double* samples, uint32_t slot, const rt::Color& c) {
  double* o = samples + 3 * (size_t)slot;
  o[0] = c.x; o[1] = c.y; o[2] = c.z;
}

// Opens a pass on its stream: the work counter back to 0, the pass's map where the trace kernels read it.
__global__ void k_pass_begin(unsigned int* work_counter, PassMap* map, PassMap m) {
  if (threadIdx.x == 0) { *work_counter = 0u; *map = m; }
}

// Items a wave claims from the pass's work counter per grab (k_trace_lds: RTX_CHUNK, this by default).
#define TRACE_CHUNK 512u

// A lane's rank among the set lanes of a wave mask: the number of set bits below its own lane.  (k_wf_shade spells the pair out:
// through this function its instructions come out in another order.)
__device__ __forceinline__ uint32_t lane_rank(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// The wave claims the next `chunk` items of the pass: lane 0 bumps the work counter, every lane gets the first item.  At or past
// the pass's total the queue is empty; the caller clamps the chunk's end to the total.  Used where the kernel's code comes out
// the same as with the lines written in place (k_trace_vote, trace_ring.inc); k_trace_lds without a ring, k_trace_world and
// k_trace_nee keep them written out, and a form that also does the test and the clamp changed every kernel.
__device__ __forceinline__ uint32_t queue_claim(unsigned int* work_counter, uint32_t chunk) {
  uint32_t base = 0;
  if ((threadIdx.x & 63u) == 0u) base = atomicAdd(work_counter, chunk);
  return __builtin_amdgcn_readfirstlane(base);
}

// (A wave's ring of ready primary rays in LDS -- RING_F64, ring_bytes -- is laid out in lds_layout.inc.)
