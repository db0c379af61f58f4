// A pass's index space as the trace kernels see it (included by render.hip, namespace rtx): item -> pixel and path, the
// sample store, the persistent kernels' work counter (chunk size, claim), a lane's rank in a wave mask and the size of the
// per-wave primary-ray ring.
//
// A pass of `total` items is one index space [0, total): item g = s_local * npix + lp is sample s_begin + s_local of the
// shard's local pixel lp, so 64 consecutive items are 64 consecutive pixels of one sample: coherent primary rays, coalesced
// sample-buffer stores.  Which lane traces an item cannot matter: streams are keyed by (pixel, sample) and every item owns its
// output slot.
//
// An adaptive pass (progressive.inc) traces only the shard's still-active pixels: its map is an ActiveMap, whose list holds
// their local pixels in ascending order, and npix is then the length of that list -- item g = s_local * npix + k is sample
// s_begin + s_local of local pixel active[k].  The list is ascending, so 64 consecutive items are still mostly neighbouring
// pixels of one sample.  The map's type is a template parameter of every trace kernel (SM, default ShardMap): a uniform
// pass's instantiation has neither the list nor a test for it -- a runtime test on a kernel argument cost 0.4 - 1.6 % on the
// k_trace_lds and k_trace_world legs of bench.py, through the kernels' register assignment.

// Local pixel lp of a shard -> image (column i, row j).  Rows of a shard are the rows j with
// (j / block_rows) % shard_count == shard_index, compacted in ascending j.
struct ShardMap {
  int32_t width, block_rows, shard_index, shard_count;
};
struct ActiveMap : ShardMap {
  const uint32_t* active;  // the pass's active local pixels, ascending
};
__device__ __forceinline__ uint32_t map_pixel(const ShardMap&, uint32_t k) { return k; }
__device__ __forceinline__ uint32_t map_pixel(const ActiveMap& m, uint32_t k) { return m.active[k]; }
__device__ __forceinline__ void shard_pixel(const ShardMap& m, uint32_t lp, uint32_t* i, uint32_t* j) {
  uint32_t lr = lp / (uint32_t)m.width;
  *i = lp - lr * (uint32_t)m.width;
  uint32_t k = lr / (uint32_t)m.block_rows;
  uint32_t within = lr - k * (uint32_t)m.block_rows;
  *j = (k * (uint32_t)m.shard_count + (uint32_t)m.shard_index) * (uint32_t)m.block_rows + within;
}

// Item g of the pass -> image pixel (i, j); returns the item's sample index within the pass.
template <class SM>
__device__ __forceinline__ uint32_t item_pixel(const SM& sm, uint32_t npix, uint32_t g, uint32_t* i, uint32_t* j) {
  const uint32_t s_local = g / npix;
  shard_pixel(sm, map_pixel(sm, g - s_local * npix), i, j);
  return s_local;
}

// The camera ray and RNG stream of item g (path_begin, core/integrator.hpp).
template <class SM>
__device__ __forceinline__ void start_path(const rt::RenderParams& rp, const SM& sm, uint32_t npix, uint32_t s_begin,
                                           uint32_t g, rt::PathState* ps) {
  uint32_t i, j;
  const uint32_t s_local = item_pixel(sm, npix, g, &i, &j);
  rt::path_begin(rp, i, j, s_begin + s_local, ps);
}

// Item g's radiance into the pass's sample buffer (k_reduce_samples adds it onto the accumulator in sample order).
__device__ __forceinline__ void store_sample(double* samples, uint32_t g, const rt::Color& c) {
  double* o = samples + 3 * (size_t)g;
  o[0] = c.x; o[1] = c.y; o[2] = c.z;
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
