// The primary-ray ring's top-up and take, as text: included inside the regeneration step of k_trace_vote and k_trace_lds, with
//   RING_CAP         entries of a wave's ring (a constant or a kernel argument)
//   RING_DIAG(mask)  the kernel's diagnostics line for the lanes that start a path (may be empty)
// defined before the include and undefined after it.  It is text and not a function because every function form tried (around
// the whole block, or only around the row stores and loads) changed these kernels' instructions; as text the compiler sees what
// it saw when each kernel spelled the block out.  Uses the kernel's locals: n_need and rank (count of the lanes without a path,
// and each one's rank among them), ring_f, ring_g, ring_n, chunk_pos, chunk_end, queue_empty, chunk, lane, active, ps, g and
// the pass's arguments.  The row order (origin, direction, time, RNG state; then the sample's slot) and path_begin's constants
// (core/integrator.hpp) live here and nowhere else.
//
// Regeneration (Philox seeding, pixel jitter, lens rejection loop, camera ray: ~600 VALU) runs for the whole wave at once and
// only when the ring cannot serve the lanes that wait; a lane whose path has ended pops a ready ray (10 LDS reads).  The ring
// is a stack.  Top up at most twice: a chunk boundary can cut the first batch short.
for (int rep = 0; rep < 2 && ring_n < n_need && !queue_empty; ++rep) {
  if (chunk_pos >= chunk_end) {
    const uint32_t base = queue_claim(work_counter, chunk);
    if (base >= total) { queue_empty = true; break; }
    chunk_pos = base;
    chunk_end = (total - base < chunk) ? total : base + chunk;
  }
  const uint32_t room = RING_CAP - ring_n, avail = chunk_end - chunk_pos;
  const uint32_t m = room < avail ? room : avail;
  RING_DIAG(wave_ballot(lane < m));
  if (lane < m) {
    // start_path in two halves, the sample's slot stored in between: nothing of the item's map stays in a register across
    // path_begin, where this kernel's register count peaks
    const uint32_t slot = ring_n + lane;
    uint32_t pi, pj, s_local;
    ring_g[slot] = item_pixel(sm, chunk_pos + lane, &pi, &pj, &s_local);
    rt::PathState fresh;
    rt::path_begin(rp, pi, pj, s_begin + s_local, &fresh);
    ring_f[0 * RING_CAP + slot] = fresh.ray.origin.x; ring_f[1 * RING_CAP + slot] = fresh.ray.origin.y;
    ring_f[2 * RING_CAP + slot] = fresh.ray.origin.z; ring_f[3 * RING_CAP + slot] = fresh.ray.direction.x;
    ring_f[4 * RING_CAP + slot] = fresh.ray.direction.y; ring_f[5 * RING_CAP + slot] = fresh.ray.direction.z;
    ring_f[6 * RING_CAP + slot] = fresh.ray.time;
    ring_f[7 * RING_CAP + slot] = rt::bits_f64(fresh.rng.s0); ring_f[8 * RING_CAP + slot] = rt::bits_f64(fresh.rng.s1);
  }
  chunk_pos += m;
  ring_n += m;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // LDS executes a wave's accesses in order
}
const uint32_t take = n_need < ring_n ? n_need : ring_n;
if (!active && rank < take) {
  const uint32_t slot = ring_n - 1u - rank;
  ps.ray = rt::make_ray(rt::v3(ring_f[0 * RING_CAP + slot], ring_f[1 * RING_CAP + slot], ring_f[2 * RING_CAP + slot]),
                        rt::v3(ring_f[3 * RING_CAP + slot], ring_f[4 * RING_CAP + slot], ring_f[5 * RING_CAP + slot]),
                        ring_f[6 * RING_CAP + slot]);
  ps.rng.s0 = rt::f64_bits(ring_f[7 * RING_CAP + slot]); ps.rng.s1 = rt::f64_bits(ring_f[8 * RING_CAP + slot]);
  ps.product = rt::v3(1, 1, 1);   // path_begin's constants (core/integrator.hpp)
  ps.output = rt::v3(0, 0, 0);
  ps.depth = rp.max_depth;
  g = ring_g[slot];
  active = true;
}
ring_n -= take;
__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
