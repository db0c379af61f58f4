// k_trace_world -- the trace kernel for ANY world (included by render.hip, namespace rtx).
//
// HittableList::hit (hit.rs:660-690) scans the world's entries in order; in the reference's big scenes two of those
// entries are BVHs (Book-2: 400 boxes, and the 1000-sphere cube under Translate(RotateY(..))) and the rest are plain
// primitives and media.  world_hit (core/geometry.hpp) runs that scan wave-synchronously: every lane of the wave is at
// the same entry, so each BVH walk lasts as long as the wave's slowest ray -- twice per bounce (measured on Book-2 in the
// since-removed k_trace_persistent: 30 % of the VALU lanes busy).  Here the scan is a per-lane state machine, so that walks can be carried over exactly as
// k_trace_vote carries them over within one BVH:
//
//   ENTRY(e)  the lane must process world entry e next        WALK(e)  its ray is inside the BVH of entry e
//   SHADE     all entries done: finalize + scatter            NEED     no path: wants a sample index
//
//   loop:  ONE kind of work per iteration, the kind most lanes wait for: walk step (node / leaf vote) | sweep | shade | regenerate
//
// A sweep visits the entry indices 0..n-1 ONCE, wave-uniformly (entry records are scalar loads, the kind switch is a
// scalar branch); at index e the lanes whose own position is e take part: a lane leaving the BVH of entry 0 finishes it,
// runs through the plain entries 1..10 and enters the BVH of entry 11 in one sweep, while its neighbours may be
// anywhere else in their own scans.  Walk steps serve lanes of different entries together (one node array holds every
// BVH; the ray each lane walks with -- transformed for Translate/RotateY entries -- and its t_min sit in a per-lane LDS
// slot).  The running hit is kept as (entry, primitive, t) and the HitRecord is built once, for the winner.
//
// Semantics are world_hit's (core/geometry.hpp), per lane: entries in list order, later entry wins an exact tie,
// a medium draws its uniform at its place in the list (hit.rs:969) from the lane's own stream, media over any boundary.
// Results are bit-identical to every other kernel (tests/test_gpu_parity.py).

constexpr uint32_t P_BOOK2 = P_ANY & ~(rt::F_TRIANGLE | rt::F_GROUP | rt::F_CHECKER | rt::F_MEDIUM_GENERAL);
constexpr uint32_t P_NO_SPHERE_MEDIA = P_ANY & ~rt::F_MEDIUM_SPHERE;  // the Cornell family and the other list worlds: no fused sphere-medium code  // the Book-2 final scene exactly

enum : uint32_t { WS_NEED = 0u, WS_ENTRY = 1u, WS_WALK = 2u, WS_SHADE = 3u };

// One record per slot of the world list with everything a sweep needs about the entry, so that the sweep reaches it
// with ONE scalar fetch (walking FlatEntry -> boundary entry -> transformed entry -> geometry entry costs up to four
// dependent scalar loads per slot).  Built at upload from the flattened scene.
enum : int32_t {
  WD_MEDIUM = 1, WD_XFORM = 2, WD_BVH = 4,
  WD_BOXED_PRIM = 8,    // `box` holds the f32 box of the entry's geometry: a plain static primitive, or the boundary sphere of a medium
  WD_SPHERE = 16,       // the geometry is one static sphere, untransformed: g_a is its PrimRef (plain entry or medium boundary)
  WD_TIME_BOX = 64,     // a plain moving sphere: `box` covers it for ray times inside [neg_inv_density, aux] = its own (time0, time1);
                        // the launcher's shutter interval decides per render whether the box may be used
  WD_PAIR = 32,         // a plain WD_SPHERE entry whose NEXT entry is a medium bounded by the very same sphere (Book-2's glass balls
                        // around their smoke / fog): the sweep solves the quadratic once for both entries
};
struct WorldDesc {  // 192 B
  int32_t flags, n_ops;
  int32_t g_kind, g_a, g_b;    // the geometry: PRIM (a = ref) / GROUP (a = first ref, b = count) / BVH (a = root, b = first ref)
  int32_t medium_mat;          // phase-function material of a medium
  float box[6];                // WD_BOXED_PRIM: f32 box of the plain static primitive (lo xyz, hi xyz; rounded outward)
  rt::real neg_inv_density;      // FlatEntry.f[0] of a medium
  rt::FlatXformOp ops[RT_MAX_XFORM_OPS];  // outermost first
  rt::real aux;                  // WD_TIME_BOX: the moving sphere's time1 (its time0 sits in neg_inv_density)
};
static_assert(sizeof(WorldDesc) == (sizeof(rt::real) == 8 ? 192 : 136), "WorldDesc layout");

static std::vector<WorldDesc> build_world_desc(const FlatScene& fs) {
  std::vector<WorldDesc> out(fs.top_level.size());
  for (size_t k = 0; k < fs.top_level.size(); ++k) {
    WorldDesc& d = out[k];
    memset(&d, 0, sizeof(d));
    const rt::FlatEntry* E = &fs.entries[fs.top_level[k]];
    const rt::FlatEntry* S = E;
    if (E->kind == rt::ENTRY_MEDIUM) { d.flags |= WD_MEDIUM; d.medium_mat = E->b; d.neg_inv_density = E->f[0]; S = &fs.entries[E->a]; }
    const rt::FlatEntry* G = S;
    if (S->kind == rt::ENTRY_XFORM) { d.flags |= WD_XFORM; d.n_ops = S->b; for (int k = 0; k < RT_MAX_XFORM_OPS; ++k) d.ops[k] = S->ops[k]; G = &fs.entries[S->a]; }
    d.g_kind = G->kind; d.g_a = G->a; d.g_b = G->b;
    if (G->kind == rt::ENTRY_BVH) d.flags |= WD_BVH;
    if (E->kind == rt::ENTRY_PRIM && fs.top_box32.size() >= 6 * (k + 1)) {
      bool finite = true;
      for (int a = 0; a < 6; ++a) { d.box[a] = fs.top_box32[6 * k + a]; finite = finite && std::isfinite(d.box[a]); }
      if (finite) d.flags |= WD_BOXED_PRIM;
    }
    if (E->kind == rt::ENTRY_PRIM && rt::primref_type((rt::PrimRef)E->a) == rt::PRIM_MOVING_SPHERE) {
      // (core/mover_box.hpp: mover_slot_box32, the rule rtx_scene_set_moving_spheres shares)
      const rt::FlatMovingSphere& ms = fs.moving_spheres[rt::primref_index((rt::PrimRef)E->a)];
      if (rt::mover_slot_box32(ms, d.box)) { d.flags |= WD_TIME_BOX; d.neg_inv_density = ms.time0; d.aux = ms.time1; }
    }
    if (!(d.flags & WD_XFORM) && G->kind == rt::ENTRY_PRIM && rt::primref_type((rt::PrimRef)G->a) == rt::PRIM_SPHERE) {
      d.flags |= WD_SPHERE;
      if (d.flags & WD_MEDIUM) {
        // A medium only acts where the ray is inside its boundary within (t_min, closest) (hit.rs:969-975: t1 >= t2 returns
        // before the uniform is drawn), i.e. inside the boundary's box: the same conservative f32 test applies.
        // (core/prim_box.hpp: medium_sphere_box32, the rule rtx_scene_set_spheres shares)
        const bool finite = rt::medium_sphere_box32(fs.spheres[rt::primref_index((rt::PrimRef)G->a)], d.box);
        if (finite) d.flags |= WD_BOXED_PRIM;
      }
    }
  }
  for (size_t k = 0; k + 1 < out.size(); ++k) {
    const WorldDesc& a = out[k];
    const WorldDesc& b = out[k + 1];
    if ((a.flags & WD_SPHERE) && !(a.flags & WD_MEDIUM) && (b.flags & WD_SPHERE) && (b.flags & WD_MEDIUM)) {
      const rt::FlatSphere& sa = fs.spheres[rt::primref_index((rt::PrimRef)a.g_a)];
      const rt::FlatSphere& sb = fs.spheres[rt::primref_index((rt::PrimRef)b.g_a)];
      if (memcmp(&sa.cx, &sb.cx, 4 * sizeof(rt::real)) == 0) out[k].flags |= WD_PAIR;  // centre and radius, bit for bit
    }
  }
  // The instance trees, BEHIND the slots' records: record n_top + k has g_a = first slot, g_b = number of slots, medium_mat =
  // root node of tree k, in ascending order of first slot; one more with g_a = INT32_MAX closes the table (it is what
  // core/flat_types.hpp's ENTRY_INSTANCE records say).  Only the P_INST instantiation reads past the slots.
  if (fs.features & rt::F_INSTANCE)
    for (const rt::FlatEntry& e : fs.entries)
      if (e.kind == rt::ENTRY_INSTANCE) {
        WorldDesc d;
        memset(&d, 0, sizeof(d));
        d.g_a = e.b; d.g_b = e.c; d.medium_mat = e.a;
        out.push_back(d);
      }
  return out;
}
// waves per SIMD k_trace_world is compiled for: 3 (168 VGPRs) measured best in f64 (2: 423, 4: 344 against 573 Msamples/s on
// Book-2); the f32 compilation's state is half the registers
#if defined(RT_F32)
#define WORLD_WPS 4
#else
#define WORLD_WPS 3
#endif
#define WORLD_SLOT_F64 7  // per-lane LDS slot: walk ray origin(3) direction(3), exact t_min of the query

// A transform op at a wave-uniform address (scalar loads, field by field: the constant address space has no class copy).
__device__ __forceinline__ rt::FlatXformOp load_op_uniform(const rt::FlatXformOp* p) {
  rt::FlatXformOp o;
  o.op = dev_load_uniform(&p->op); o.pad = 0;
  o.v[0] = dev_load_uniform(&p->v[0]); o.v[1] = dev_load_uniform(&p->v[1]); o.v[2] = dev_load_uniform(&p->v[2]);
  return o;
}

// UNIFORM: G is the same for every lane (the sweep); false: each lane has its own (a member of an instance tree).
template <uint32_t F, bool UNIFORM = true>
__device__ __forceinline__ bool direct_closest(const rt::SceneView& sv, const rt::FlatEntry& G, const rt::Ray& r, rt::real t_min,
                                               rt::real t_max, rt::real* t_out, rt::PrimRef* ref_out) {
  if ((F & rt::F_PRIM_ENTRY) && (G.kind == rt::ENTRY_PRIM || !(F & rt::F_GROUP))) {
    *ref_out = (rt::PrimRef)G.a;
    return rt::prim_t<F, false>(sv, (rt::PrimRef)G.a, r, t_min, t_max, t_out, nullptr);
  }
  bool hit = false;
  if (F & rt::F_GROUP) {  // HittableList::hit: in order, shrinking closest_so_far, later wins ties
    rt::real best = t_max;
    for (int32_t i = 0; i < G.b; ++i) {
      const rt::PrimRef ref = UNIFORM ? dev_load_uniform(&sv.refs[G.a + i]) : sv.refs[G.a + i];
      rt::real t;
      if (rt::prim_t<F, false>(sv, ref, r, t_min, best, &t, nullptr)) { best = t; hit = true; *ref_out = ref; }
    }
    *t_out = best;
  }
  return hit;
}

// DIAG: per-region counters (executions by the wave, lanes taking part) -- diagnostic build only (RTX_TRACE_KERNEL=world_diag).
template <uint32_t F, bool WIDE, int WAVES_PER_SIMD, bool DIAG = false, class SM = ShardMap>
__global__ __launch_bounds__(TRACE_BLOCK, WAVES_PER_SIMD) void k_trace_world(
    rt::SceneView sv_in, rt::RenderParams rp, SM sm, uint32_t s_begin, uint32_t total,
    double* __restrict__ samples, unsigned int* __restrict__ work_counter, const rt::FlatEntry* __restrict__ entries_ro,
    const int32_t* __restrict__ top_level_ro, const rt::FlatSphere* __restrict__ spheres_ro,
    const rt::FlatMovingSphere* __restrict__ msph_ro, const rt::FlatRect* __restrict__ rects_ro,
    const rt::FlatTriangle* __restrict__ tris_ro, const rt::FlatMaterial* __restrict__ mats_ro,
    const rt::FlatTexture* __restrict__ tex_ro, const rt::PrimRef* __restrict__ refs_ro,
    const FlatNode4* __restrict__ nodes4, const WorldDesc* __restrict__ wdesc, uint32_t leaf_weight, uint32_t walk_threshold,
    uint32_t stack_levels, uint32_t n_perlin_lds, uint32_t n_mat_lds, uint32_t n_tex_lds, unsigned long long* diag = nullptr) {
  unsigned long long dg[16];
  if (DIAG) for (int k = 0; k < 16; ++k) dg[k] = 0;
  rt::SceneView sv = sv_in;  // read-only tables through const __restrict__ parameters: scalar loads where uniform
  sv.entries = entries_ro; sv.top_level = top_level_ro;
  sv.spheres = spheres_ro; sv.moving_spheres = msph_ro; sv.rects = rects_ro; sv.triangles = tris_ro;
  sv.materials = mats_ro; sv.textures = tex_ro; sv.refs = refs_ro;
  extern __shared__ int32_t lds_stack[];
  LdsStackB stack;
  stack.base = lds_stack + threadIdx.x;
  stack.init();
  rt::real* const slot = (rt::real*)(lds_stack + stack_levels * TRACE_BLOCK) + threadIdx.x;  // field k at slot[k * TRACE_BLOCK]
  // The Perlin tables (9 KB each) ride in LDS when they fit: a marble hit is rare per ray but present in most shading rounds
  // of a wave, and turbulence is 7 octaves of dependent table look-ups (perm -> gradient) that otherwise each wait on L1 / L2.
  if (n_perlin_lds > 0u) {
    uint32_t* const dst = (uint32_t*)((rt::real*)(lds_stack + stack_levels * TRACE_BLOCK) + WORLD_SLOT_F64 * TRACE_BLOCK);
    const uint32_t* const src = (const uint32_t*)sv.perlins;
    const uint32_t words = n_perlin_lds * (uint32_t)(sizeof(rt::FlatPerlin) / 4u);
    for (uint32_t k = threadIdx.x; k < words; k += TRACE_BLOCK) dst[k] = src[k];
    __syncthreads();
    sv.perlins = (const rt::FlatPerlin*)dst;
  }
  // ... and so do the material and texture tables of worlds that have few of them: every shading fetches material -> texture,
  // two dependent per-lane loads
  if (n_mat_lds > 0u) {
    uint32_t* const dst = (uint32_t*)((rt::real*)(lds_stack + stack_levels * TRACE_BLOCK) + WORLD_SLOT_F64 * TRACE_BLOCK) +
                          n_perlin_lds * (uint32_t)(sizeof(rt::FlatPerlin) / 4u);
    const uint32_t mw = n_mat_lds * (uint32_t)(sizeof(rt::FlatMaterial) / 4u), tw = n_tex_lds * (uint32_t)(sizeof(rt::FlatTexture) / 4u);
    const uint32_t* const ms = (const uint32_t*)mats_ro;
    const uint32_t* const ts = (const uint32_t*)tex_ro;
    for (uint32_t k = threadIdx.x; k < mw; k += TRACE_BLOCK) dst[k] = ms[k];
    for (uint32_t k = threadIdx.x; k < tw; k += TRACE_BLOCK) dst[mw + k] = ts[k];
    __syncthreads();
    sv.materials = (const rt::FlatMaterial*)dst;
    sv.textures = (const rt::FlatTexture*)(dst + mw);
  }
  const uint32_t lane = threadIdx.x & 63u;
  const int32_t n_top = sv.n_top_level;
  uint32_t chunk_pos = 0, chunk_end = 0;  // wave-uniform
  bool queue_empty = false;               // wave-uniform
  uint32_t stage = WS_NEED;
  uint32_t g = 0;  // the path's slot of the sample buffer (start_path)
  rt::PathState ps;
  // the lane's scan of the world list
  int32_t ei = 0;              // entry being processed
  uint32_t ph = 0;             // 0 / 1: first / second boundary query of a medium whose boundary is a BVH
  rt::real closest = RT_INFINITY, aux_t = 0.0;
  bool hit_any = false;
  int32_t win_e = 0;
  rt::PrimRef win_ref = 0;
  // walk state
  rt::Ray32 q = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  uint32_t dir_neg = 0;
  float t_max32 = 0.f;
  int32_t cur = WALK_DONE, walk_root = 0;
  bool walk_plain = false;     // the walk belongs to a non-medium BVH entry: its result needs no entry record to be taken
  uint32_t first_ref = 0;
  rt::Closest best;
  best.t = 0.0; best.ref = WALK_NO_REF; best.order = 0; best.hit = false;  // (.hit is not maintained in this kernel: WALK_NO_REF, trace_vote.inc)
  // Instance trees (P_INST only; DESIGN.md 8.1).  A lane whose scan reaches the first slot of a tree walks the SLOT tree with
  // the same node steps as any BVH (im = 1: its culling ray is the path's own, `closest` its t_max); a leaf of that tree is one
  // member slot, which the lane visits on its own: record by a per-lane load, ray transformed per lane, a primitive or group
  // tested in place, a BVH member walked ABOVE the slot walk on the same stack (im = 2: one WALK_DONE marker between the two, so
  // the member walk ends like any walk and the lane then pops the slot walk's next item).  Members are met in tree order, so the
  // list's tie rule is spelled out: on t == closest the higher slot wins (core/geometry.hpp: instance_offer_slot).
  constexpr bool INST = (F & rt::F_INSTANCE) != 0;
  static_assert(!(INST && WIDE), "worlds with instance trees walk the binary tree");
  [[maybe_unused]] uint32_t im = 0u;  // 0: no instance walk, 1: in the slot tree, 2: in a member's BVH (walk_root holds the member's slot)

  auto slot_ray = [&]() {
    return rt::make_ray(rt::v3(slot[0 * TRACE_BLOCK], slot[1 * TRACE_BLOCK], slot[2 * TRACE_BLOCK]),
                        rt::v3(slot[3 * TRACE_BLOCK], slot[4 * TRACE_BLOCK], slot[5 * TRACE_BLOCK]), ps.ray.time);
  };
  auto begin_walk = [&](const rt::Ray& rq, rt::real q_min, rt::real q_max, int32_t root, uint32_t fref) {
    slot[0 * TRACE_BLOCK] = rq.origin.x; slot[1 * TRACE_BLOCK] = rq.origin.y; slot[2 * TRACE_BLOCK] = rq.origin.z;
    slot[3 * TRACE_BLOCK] = rq.direction.x; slot[4 * TRACE_BLOCK] = rq.direction.y; slot[5 * TRACE_BLOCK] = rq.direction.z;
    slot[6 * TRACE_BLOCK] = q_min;
    q = rt::make_ray32(rq, q_min);
    dir_neg = WIDE ? wide_sign_pack(rq) : rt::ray_dir_neg(rq);  // wide walks keep their plane offsets in this register
    t_max32 = rt::cull_round_up(q_max);
    best.t = q_max; best.ref = WALK_NO_REF; best.order = 0;
    stack.reset();
    cur = root;
    walk_root = root;
    first_ref = fref;
  };
  auto write_sample = [&]() { store_sample(samples, g, ps.output); };
  // a new ray starts its scan (world.rs:64-68: depth first)
  auto begin_bounce = [&]() {
    if (rt::path_bounce_begin(&ps)) { write_sample(); stage = WS_NEED; }
    else { closest = RT_INFINITY; hit_any = false; ei = 0; ph = 0; stage = WS_ENTRY; }
  };

  // a member's BVH walk has ended: take its hit by the list's rule, go on with the slot walk
  auto close_member = [&]() {
    if constexpr (INST) if (im == 2u && cur == WALK_DONE) {
      if (best.ref != WALK_NO_REF && !(hit_any && best.t == closest && walk_root < win_e)) { closest = best.t; win_e = walk_root; win_ref = best.ref; hit_any = true; }
      q = rt::make_ray32(ps.ray, rt::ray_t_min(ps.ray));
      dir_neg = rt::ray_dir_neg(ps.ray);
      t_max32 = rt::cull_round_up(closest);
      cur = stack.pop();
      im = 1u;
    }
  };
  // a leaf of the slot tree: one member, visited by this lane alone
  auto visit_member = [&]() {
    if constexpr (INST) {
    const int32_t ms = (int32_t)rt::leaf_first(cur);
    const WorldDesc* W = &wdesc[ms];  // per-lane
    const int32_t wflags = W->flags;
    const rt::real t_min = rt::ray_t_min(ps.ray);
    rt::Ray rq = ps.ray;
    if ((F & rt::F_XFORM) && (wflags & WD_XFORM)) {
      const int n_ops = W->n_ops;
      for (int k = 0; k < n_ops; ++k) rq = rt::xform_ray(W->ops[k], rq);
    }
    rt::FlatEntry G;
    G.kind = W->g_kind; G.a = W->g_a; G.b = W->g_b;
    if ((F & rt::F_BVH) && (wflags & WD_BVH)) {
      slot[0 * TRACE_BLOCK] = rq.origin.x; slot[1 * TRACE_BLOCK] = rq.origin.y; slot[2 * TRACE_BLOCK] = rq.origin.z;
      slot[3 * TRACE_BLOCK] = rq.direction.x; slot[4 * TRACE_BLOCK] = rq.direction.y; slot[5 * TRACE_BLOCK] = rq.direction.z;
      slot[6 * TRACE_BLOCK] = t_min;
      q = rt::make_ray32(rq, t_min);
      dir_neg = rt::ray_dir_neg(rq);
      t_max32 = rt::cull_round_up(closest);
      best.t = closest; best.ref = WALK_NO_REF; best.order = 0;
      stack.push(WALK_DONE);
      cur = G.a;
      first_ref = (uint32_t)G.b;
      walk_root = ms;
      im = 2u;
    } else {
      rt::real t;
      rt::PrimRef ref = 0;
      if (direct_closest<F, false>(sv, G, rq, t_min, closest, &t, &ref) && !(hit_any && t == closest && ms < win_e)) {
        closest = t; win_e = ms; win_ref = ref; hit_any = true;
        t_max32 = rt::cull_round_up(closest);
      }
      cur = stack.pop();
    }
    }
  };

  // entry 0 a plain BVH (Book-2, the dragon room, every catalogue scene that has a BVH): a new ray enters it at once
  bool e0_plain_bvh = false;
  int32_t e0_root = 0;
  uint32_t e0_first_ref = 0;
  if (n_top > 0) {
    e0_plain_bvh = (F & rt::F_BVH) && dev_load_uniform(&wdesc[0].flags) == WD_BVH;
    e0_root = dev_load_uniform(&wdesc[0].g_a);
    e0_first_ref = (uint32_t)dev_load_uniform(&wdesc[0].g_b);
    if constexpr (INST) if (dev_load_uniform(&wdesc[n_top].g_a) == 0) e0_plain_bvh = false;  // slot 0 is a member: reached through its tree
  }
  auto begin_bounce_fast = [&]() {
    begin_bounce();
    if (stage == WS_ENTRY && e0_plain_bvh) {
      begin_walk(ps.ray, rt::ray_t_min(ps.ray), closest, e0_root, e0_first_ref);
      walk_plain = true;
      stage = WS_WALK;
    }
  };

  // One kind of work per iteration, chosen by vote: the kind most lanes are waiting for runs (walk step, sweep of the
  // world list, shading, regeneration), so each of the long code paths executes with a well filled wave; lanes of the
  // other kinds keep their state and wait.  Every lane passes through every kind again and again, so none starves.
  for (;;) {
    // a finished walk of a plain (non-medium) BVH entry needs nothing from the entry record: close it here
    if (stage == WS_WALK && cur == WALK_DONE && walk_plain) {
      if (best.ref != WALK_NO_REF) { closest = best.t; win_e = ei; win_ref = best.ref; hit_any = true; }
      ei += 1;
      stage = ei >= n_top ? WS_SHADE : WS_ENTRY;
    }
    close_member();
    const bool is_leaf = cur < 0;
    const bool is_node = (uint32_t)cur < (uint32_t)WALK_DONE;
    const unsigned long long m_node = wave_ballot(is_node), m_leaf = wave_ballot(is_leaf);
    const unsigned long long m_sweep = wave_ballot(stage == WS_ENTRY || (stage == WS_WALK && cur == WALK_DONE));
    const unsigned long long m_shade = wave_ballot(stage == WS_SHADE);
    const unsigned long long m_need = wave_ballot(stage == WS_NEED);
    const uint32_t n_walk = (uint32_t)__popcll(m_node | m_leaf), n_sweep = (uint32_t)__popcll(m_sweep);
    const uint32_t n_shade = (uint32_t)__popcll(m_shade);
    const uint32_t n_need = queue_empty ? 0u : (uint32_t)__popcll(m_need);
    if ((n_walk | n_sweep | n_shade | n_need) == 0u) break;  // queue drained and every path has ended
    // walk steps are short, the sweep and shading are long: walking goes on while at least `walk_threshold` lanes walk, so
    // that the long paths run seldom and with many lanes; below that the largest waiting class runs
    uint32_t n_other = n_sweep > n_shade ? n_sweep : n_shade;
    n_other = n_other > n_need ? n_other : n_need;
    if (n_walk > 0u && (walk_threshold == 0u ? n_walk >= n_other : (n_walk >= walk_threshold || n_other == 0u))) {
      // ------------------------------------------------------------------ walk steps: node / leaf vote
      // Steps repeat without the full vote while walking must still be the largest class even if every lane that has
      // finished since belongs to the largest other class (a lane's class after its walk is not known until it is closed).
      const uint32_t others = n_other;
      unsigned long long mn = m_node, ml = m_leaf;
      for (;;) {
        if ((uint32_t)__popcll(mn) * leaf_weight >= (uint32_t)__popcll(ml)) {
          DIAG_ADD(0, mn);
          if ((uint32_t)cur < (uint32_t)WALK_DONE) {
            if (WIDE) walk_node_step4(nodes4, q, dir_neg, t_max32, &cur, stack);
            else walk_node_step32(sv.nodes32[cur], q, dir_neg, t_max32, &cur, stack);
          }
        } else if (cur < 0) {
          DIAG_ADD(1, ml);
          bool at_member = false;
          if constexpr (INST) at_member = im == 1u;
          if (at_member) {
            visit_member();
          } else {
            const rt::Ray rl = slot_ray();
            walk_leaf_step<F>(sv, first_ref, rl, slot[6 * TRACE_BLOCK], &best, &cur, stack);
            t_max32 = rt::cull_round_up(best.t);
          }
        }
        close_member();
        mn = wave_ballot((uint32_t)cur < (uint32_t)WALK_DONE);
        ml = wave_ballot(cur < 0);
        const uint32_t still = (uint32_t)__popcll(mn | ml);
        if (still == 0u || (walk_threshold == 0u ? still < others + (n_walk - still) : (still < walk_threshold && others + (n_walk - still) > 0u))) break;
      }
    } else if (n_shade >= n_sweep && n_shade >= n_need) {
      // ------------------------------------------------------------------ shade the lanes whose scan is complete
      // (A split into a lean Lambertian-only class and a "rare materials" class was measured on Book-2 and dropped: 72 % of
      // its hits are on glass, fog or lights -- the r = 5000 glass shell alone catches every escaping ray -- and a fifth
      // class thins every other one out: 631 -> 493 Msamples/s.)
      DIAG_ADD(3, m_shade);
      if (stage == WS_SHADE) {
        rt::HitRecord rec;
        if (hit_any) {
          const WorldDesc* W = &wdesc[win_e];  // per-lane: lanes won at different entries
          const int32_t wflags = W->flags;
          if ((F & rt::F_MEDIUM) && (wflags & WD_MEDIUM)) {
            rec.t = closest;
            rec.p = rt::ray_at(ps.ray, closest);
            rec.normal = rt::v3(0, 0, 0);
            rec.front_face = true;
            rec.u = 0.0; rec.v = 0.0;
            rec.mat = W->medium_mat;
          } else if ((F & rt::F_XFORM) && (wflags & WD_XFORM)) {
            const int nops = W->n_ops;
            const rt::FlatXformOp op0 = W->ops[0];
            rt::Ray rq = rt::xform_ray(op0, ps.ray);
            if (nops == 1) {  // one or two wrappers (every catalogue scene): straight-line code, the records in registers
              rt::prim_finalize<F>(sv, win_ref, rq, closest, &rec);
              rt::xform_record(op0, rq, &rec);
            } else if (nops == 2) {
              const rt::FlatXformOp op1 = W->ops[1];
              rq = rt::xform_ray(op1, rq);
              rt::prim_finalize<F>(sv, win_ref, rq, closest, &rec);
              rt::xform_record(op1, rq, &rec);
              rt::xform_record(op0, rt::xform_ray(op0, ps.ray), &rec);
            } else {          // three or four: the general chain
              for (int k = 1; k < nops; ++k) rq = rt::xform_ray(W->ops[k], rq);
              rt::prim_finalize<F>(sv, win_ref, rq, closest, &rec);
              rt::xform_record_chain(W->ops, nops, ps.ray, rq, &rec);
            }
          } else {
            rt::prim_finalize<F>(sv, win_ref, ps.ray, closest, &rec);
          }
        }
        if (rt::path_bounce_end<F, false>(sv, rp, &ps, hit_any, rec, nullptr)) { write_sample(); stage = WS_NEED; }
        else begin_bounce_fast();
      }
    } else if (n_sweep >= n_need) {
      // ------------------------------------------------------------------ sweep over the world list
      DIAG_ADD(2, m_sweep);
      // the sweep steps OVER the slots of an instance tree: its members are reached through the tree, by the lanes themselves
      [[maybe_unused]] int32_t inst_rec = n_top, inst_first = 0x7fffffff;  // wave-uniform cursor in the table behind the slots' records
      if constexpr (INST) inst_first = dev_load_uniform(&wdesc[inst_rec].g_a);
      for (int32_t e = 0; e < n_top; ++e) {
        if constexpr (INST) if (e == inst_first) {
          const int32_t n_slots = dev_load_uniform(&wdesc[inst_rec].g_b), root = dev_load_uniform(&wdesc[inst_rec].medium_mat);
          inst_first = dev_load_uniform(&wdesc[++inst_rec].g_a);
          if (stage == WS_WALK && cur == WALK_DONE && ei == e) {  // the slot walk is complete: the scan goes on behind the tree
            ei = e + n_slots; stage = WS_ENTRY; im = 0u;
          } else if (stage == WS_ENTRY && ei == e) {
            q = rt::make_ray32(ps.ray, rt::ray_t_min(ps.ray));
            dir_neg = rt::ray_dir_neg(ps.ray);
            t_max32 = rt::cull_round_up(closest);
            stack.reset();
            cur = root;
            im = 1u; ph = 0u; walk_plain = false;
            stage = WS_WALK;
          }
          e += n_slots - 1;
          continue;
        }
        const bool done_here = stage == WS_WALK && cur == WALK_DONE && ei == e;
        const bool begin_here = stage == WS_ENTRY && ei == e;
        if (wave_ballot(done_here || begin_here) == 0ull) continue;
        const WorldDesc* D = &wdesc[e];  // wave-uniform: scalar loads
        const int32_t flags = dev_load_uniform(&D->flags);
        const bool is_medium = (F & rt::F_MEDIUM) && (flags & WD_MEDIUM);
        const bool is_xform = (F & rt::F_XFORM) && (flags & WD_XFORM);
        const int32_t n_ops = is_xform ? dev_load_uniform(&D->n_ops) : 0;
        rt::FlatEntry G;  // kind, a, b are all a geometry entry holds
        G.kind = dev_load_uniform(&D->g_kind); G.a = dev_load_uniform(&D->g_a); G.b = dev_load_uniform(&D->g_b);
        const bool is_bvh = (F & rt::F_BVH) && ((flags & WD_BVH) || !(F & (rt::F_PRIM_ENTRY | rt::F_GROUP)));
        // the medium's decision once both boundary hits are known (hit.rs:961-985; world_hit in core/geometry.hpp)
        auto medium_decide = [&](rt::real rec1_t, rt::real rec2_t) {
          rt::real t1 = rt::rt_fmax(rec1_t, rt::ray_t_min(ps.ray));
          rt::real t2 = rt::rt_fmin(rec2_t, closest);
          if (t1 >= t2) return;
          if (t1 < 0.0) t1 = 0.0;
          const rt::real ray_length = rt::length(ps.ray.direction);
          const rt::real distance_inside_boundary = (t2 - t1) * ray_length;
          const rt::real hit_distance = dev_load_uniform(&D->neg_inv_density) * rt::rt_log(rt::rng_f64(ps.rng));
          if (hit_distance > distance_inside_boundary) return;
          closest = t1 + hit_distance / ray_length;
          win_e = e; win_ref = 0; hit_any = true;
        };
        auto entry_ray = [&]() {
          rt::Ray rq = ps.ray;
          if (is_xform) {
            rq = rt::xform_ray(load_op_uniform(&D->ops[0]), ps.ray);
            if (n_ops > 1) rq = rt::xform_ray(load_op_uniform(&D->ops[1]), rq);
            for (int k = 2; k < n_ops; ++k) rq = rt::xform_ray(load_op_uniform(&D->ops[k]), rq);  // three or four wrappers: rare
          }
          return rq;
        };
        // media over anything but one plain sphere (which the fused block below serves) only exist in worlds with F_MEDIUM_GENERAL
        const bool is_general_medium = (F & rt::F_MEDIUM_GENERAL) && is_medium;
        if (is_bvh) {
          if (done_here) {
            if (!is_general_medium) {
              if (best.ref != WALK_NO_REF) { closest = best.t; win_e = e; win_ref = best.ref; hit_any = true; }
              ei = e + 1; stage = WS_ENTRY;
            } else if (ph == 0u) {
              if (best.ref == WALK_NO_REF) { ei = e + 1; stage = WS_ENTRY; }
              else {  // rec2 = boundary.hit(rec1.t + 0.0001, inf)
                aux_t = best.t;
                const rt::Ray rq = slot_ray();
                begin_walk(rq, rt::medium_second_t_min(aux_t), RT_INFINITY, walk_root, first_ref);
                ph = 1u;
              }
            } else {
              if (best.ref != WALK_NO_REF) medium_decide(aux_t, best.t);
              ph = 0u; ei = e + 1; stage = WS_ENTRY;
            }
          }
          if (begin_here) {
            const rt::Ray rq = entry_ray();
            begin_walk(rq, is_general_medium ? -RT_INFINITY : rt::ray_t_min(ps.ray), is_general_medium ? RT_INFINITY : closest, G.a, (uint32_t)G.b);
            ph = 0u;
            walk_plain = !is_general_medium;
            stage = WS_WALK;
          }
        } else if (begin_here) {
          bool may = true;
          bool boxed = (flags & WD_BOXED_PRIM) != 0;
          if ((F & rt::F_MOVING_SPHERE) && (flags & WD_TIME_BOX))  // every ray time of this render lies in [cam.time1, cam.time2)
            boxed = rp.cam.time1 >= dev_load_uniform(&D->neg_inv_density) && rp.cam.time2 <= dev_load_uniform(&D->aux);
          if ((F & rt::F_PRIM_ENTRY) && boxed) {
            // conservative f32 box test per lane; the f64 test is skipped when no lane of the wave can pass it
            const float lo[3] = {dev_load_uniform(&D->box[0]), dev_load_uniform(&D->box[1]), dev_load_uniform(&D->box[2])};
            const float hi[3] = {dev_load_uniform(&D->box[3]), dev_load_uniform(&D->box[4]), dev_load_uniform(&D->box[5])};
            may = rt::cull32_may_hit(lo, hi, rt::make_ray32(ps.ray, rt::ray_t_min(ps.ray)), rt::cull_round_up(closest));
          }
          DIAG_ADD(5, wave_ballot(may));
          if (wave_ballot(may) != 0ull) DIAG_ADD(6, wave_ballot(may));
          if ((F & rt::F_MEDIUM_SPHERE) && (flags & WD_SPHERE) && (is_medium || (flags & WD_PAIR))) {
            // one static sphere asked more than once: the quadratic is solved once (core/geometry.hpp: sphere_roots)
            if (wave_ballot(may) != 0ull && may) {
              const rt::FlatSphere& sp = sv.spheres[rt::primref_index((rt::PrimRef)G.a)];  // wave-uniform address
              rt::real r1, r2, guard, t;
              const bool real_roots = rt::sphere_roots(rt::v3(sp.cx, sp.cy, sp.cz), sp.radius, ps.ray, &r1, &r2, &guard);
              bool as_medium = is_medium;
              if (!is_medium) {  // the glass ball itself, then (WD_PAIR) the medium inside it, which is the next entry
                if (real_roots && rt::sphere_pick(r1, r2, rt::ray_t_min(ps.ray) + guard, closest, &t)) { closest = t; win_e = e; win_ref = (rt::PrimRef)G.a; hit_any = true; }
                as_medium = true;
              }
              if (as_medium && real_roots) {
                const int32_t me = is_medium ? e : e + 1;
                rt::real t2;
                if (rt::sphere_pick(r1, r2, -RT_INFINITY, RT_INFINITY, &t) && rt::sphere_pick(r1, r2, rt::medium_second_t_min(t) + guard, RT_INFINITY, &t2)) {
                  // hit.rs:969-985, as medium_decide above, for entry `me`
                  rt::real t1 = rt::rt_fmax(t, rt::ray_t_min(ps.ray));
                  t2 = rt::rt_fmin(t2, closest);
                  if (!(t1 >= t2)) {
                    if (t1 < 0.0) t1 = 0.0;
                    const rt::real ray_length = rt::length(ps.ray.direction);
                    const rt::real distance_inside_boundary = (t2 - t1) * ray_length;
                    const rt::real hit_distance = dev_load_uniform(&wdesc[me].neg_inv_density) * rt::rt_log(rt::rng_f64(ps.rng));
                    if (!(hit_distance > distance_inside_boundary)) { closest = t1 + hit_distance / ray_length; win_e = me; win_ref = 0; hit_any = true; }
                  }
                }
              }
            }
            // a lane the box test ruled out goes to the next entry on its own; a pair that was solved here skips the medium's slot
            ei = (!is_medium && may) ? e + 2 : e + 1;
            continue;
          }
          if (wave_ballot(may) != 0ull && may) {
            const rt::Ray rq = entry_ray();
            rt::real t;
            rt::PrimRef ref = 0;
            if (!is_general_medium) {
              if (direct_closest<F>(sv, G, rq, rt::ray_t_min(ps.ray), closest, &t, &ref)) { closest = t; win_e = e; win_ref = ref; hit_any = true; }
            } else {
              rt::real t2;
              if (direct_closest<F>(sv, G, rq, -RT_INFINITY, RT_INFINITY, &t, &ref) &&
                  direct_closest<F>(sv, G, rq, rt::medium_second_t_min(t), RT_INFINITY, &t2, &ref))
                medium_decide(t, t2);
            }
          }
          ei = e + 1;
        }
      }
      if (stage == WS_ENTRY && ei >= n_top) stage = WS_SHADE;
    } else {
      // ------------------------------------------------------------------ hand new paths to the lanes without one
      const unsigned long long need_mask = m_need;
      DIAG_ADD(4, m_need);
      {
        if (chunk_pos >= chunk_end && !queue_empty) {
          uint32_t base = 0;
          if (lane == 0) base = atomicAdd(work_counter, TRACE_CHUNK);
          base = __builtin_amdgcn_readfirstlane(base);
          if (base >= total) queue_empty = true;
          else { chunk_pos = base; chunk_end = (total - base < TRACE_CHUNK) ? total : base + TRACE_CHUNK; }
        }
        if (chunk_pos < chunk_end) {
          const uint32_t rank = lane_rank(need_mask);
          const uint32_t n_want = (uint32_t)__popcll(need_mask);
          const uint32_t avail = chunk_end - chunk_pos;
          if (stage == WS_NEED && rank < avail) {
            g = start_path(rp, sm, s_begin, chunk_pos + rank, &ps);
            begin_bounce_fast();
          }
          chunk_pos += (n_want < avail) ? n_want : avail;
        }
      }
    }
  }
  if (DIAG && lane == 0)
    for (int k = 0; k < 16; ++k) atomicAdd(&diag[k], dg[k]);
}
