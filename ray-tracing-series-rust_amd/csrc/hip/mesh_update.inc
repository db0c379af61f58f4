// rtx_scene_set_triangles / rtx_scene_set_spheres and their _device entries on a resident f64 scene: ONE update path for "new
// records of a static primitive kind" (included by render.hip, namespace rtx; the f64 compilation only: an f32 scene does not
// hold the f64 records of the untouched primitives in a touched leaf, which a refit starts from).
//
// New values for named primitives reach these device arrays and no other:
//   triangles                       v0 v1 v2 and the normal of every flat copy of a triangle id (k_set_prims)
//   spheres                         cx cy cz radius of the record of a sphere id; mat stays (k_set_prims)
//   nodes / nodes32 / motion32      every BVH that holds an updated primitive, refitted whole and bottom-up (k_refit_bvh: a leaf's
//                                   box, then scene_update.inc's refit_climb)
//   nodes4                          the planes of every slot of those BVHs' wide records; which nodes the collapse opened is kept,
//                                   so WidePlan::levels and every launch plan stand (k_refit_wide)
//   d_local_box, then the instance tree above a touched member (k_member_local_boxes, k_refit_instance_tree of scene_update.inc)
//   top_box32 / WorldDesc           a plain top-level slot of one updated triangle or sphere: both boxes and the record's "box is
//                                   finite" flag (k_slot_boxes, with core/prim_box.hpp's rules)
// for MovingSpheres (rtx_scene_set_moving_spheres*; DESIGN.md 8.7):
//   moving_spheres                  c0 c1 radius of the record of a mover id; time0, time1, mat stay (k_set_prims)
//   nodes / nodes32 / motion32      every BVH that holds an updated mover (k_refit_timed_bvh): the unions over the BVH's own interval
//                                   and, where the BVH gets time-aware boxes, the planes and slopes from the unions at its two ends
//                                   (scene_update.inc's refit_climb<true>, core/mover_box.hpp's rules); nodes4 as above
//   WorldDesc                       a plain mover in the world list: its box, WD_TIME_BOX and the two times (k_slot_boxes)
//   the slope mask                  one word per BVH, the axes its slopes run along: read back by launch_lds, which plans
//                                   k_trace_lds's time-aware instantiation by it (render.hip: plan_lds_motion_axis)
// and for static spheres only:
//   WorldDesc                       the boundary sphere of a medium: the record's box and "box is finite" flag; a plain sphere
//                                   slot before such a medium: the "same sphere as the medium behind me" flag (k_slot_boxes)
//   the light table                 when an updated sphere is a sampled light: its area, and every light's cdf and pmf
//                                   (k_refresh_lights, with host/light_table.hpp's weight rule and cdf pass)
// for rectangles (rtx_scene_set_rects*; DESIGN.md 8.8) -- walls, the six faces of a RectPrism, the boundary box of a medium,
// rectangular area lights:
//   rects                           a0 a1 b0 b1 k of the record of a rectangle id; axis and mat stay (k_set_prims)
//   nodes / nodes32 / motion32 / nodes4, d_local_box and the instance trees, top_box32 / WorldDesc of a plain rectangle slot:
//                                   as for a triangle
//   the light table                 when an updated rectangle is a sampled light: as for a sphere
//   VotePlan::top                   the HOST's copy of up to eight top-level rectangle records that travels to k_trace_vote as a
//                                   kernel argument (refresh_vote_top: rewritten by the host entry, given up by the device entry)
// with the arithmetic of the flattener (core/prim_box.hpp, host/set_triangles.hpp), so that the arrays equal those of the
// host-updated flat scene uploaded afresh -- the judge of tests/test_gpu_set_triangles.py, tests/test_gpu_set_spheres.py,
// tests/test_gpu_set_moving_spheres.py and tests/test_gpu_set_rects.py.
// k_trace_lds copies nodes32 and the sphere records into LDS at the start of every launch and keeps no packed copy from the
// upload, so it needs nothing more.  Topology is not touched: child codes, split axes, refs, entries; SceneView, the trace
// kernels, their arguments and every launch plan do not change.
//
// No index is derived from a value.  Every index a kernel forms comes from a table the host built from the caller's ids and
// the upload's shadow, both checked against the array sizes (host/set_triangles.hpp: build_mesh_shadow, check_prim_ids); a
// value is only ever stored, added or compared.  A non-finite value through a device entry therefore cannot leave an
// allocation: it gives its primitive and the boxes above it unspecified culling.  The kernels here need no visibility beyond
// kernel boundaries: each thread writes what only it owns (the climb of a refit states its own, once, in scene_update.inc).

__device__ __forceinline__ void set_record(rt::FlatTriangle* t, const double* v) { rt::set_triangle_vertices(t, v); }
__device__ __forceinline__ void set_record(rt::FlatSphere* s, const double* v) { rt::set_sphere_values(s, v); }
__device__ __forceinline__ void set_record(rt::FlatMovingSphere* s, const double* v) { rt::set_moving_sphere_values(s, v); }
__device__ __forceinline__ void set_record(rt::FlatRect* q, const double* v) { rt::set_rect_values(q, v); }

// One thread per (flat record, the caller's W values for it): pairs[2 i] = flat index, pairs[2 i + 1] = index of the W-tuple in
// `values`.
template <int W, class Record>
__global__ __launch_bounds__(256) void k_set_prims(const int32_t* __restrict__ pairs, int n_pairs, const double* __restrict__ values,
                                                  Record* __restrict__ records) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n_pairs) return;
  double v[W];
  const double* src = values + W * (size_t)pairs[2 * (size_t)i + 1];
  for (int k = 0; k < W; ++k) v[k] = src[k];
  set_record(&records[pairs[2 * (size_t)i]], v);
}

struct BvhRefitArgs {
  rt::FlatNode* nodes;
  rt::FlatNode32* nodes32;
  rt::FlatMotion32* motion32;       // NULL: the scene has no time-aware boxes
  const rt::PrimRef* refs;          // this BVH's first reference first
  const rt::FlatSphere* spheres;
  const rt::FlatRect* rects;
  const rt::FlatTriangle* triangles;
  const int32_t* leaves;            // 3 per leaf of this BVH: leaf code, node, child index
  const int32_t* node_parent;       // 2 per node of this BVH, by node - node_base: parent (-1: root), child index
  unsigned int* arrivals;           // 1 per node of this BVH, zero at launch
  int32_t n_leaves, node_base;
};

// One thread per leaf of ONE BVH -- every leaf, not only the touched ones: the union of its primitives' boxes, then the climb
// (scene_update.inc: refit_climb).
__global__ __launch_bounds__(256) void k_refit_bvh(BvhRefitArgs a) {
  const int l = (int)(blockIdx.x * 256u + threadIdx.x);
  if (l >= a.n_leaves) return;
  double b[6];
  bvh_leaf_box(a.leaves[3 * (size_t)l], a.refs, a.spheres, a.rects, a.triangles, b);
  double lo[3], hi[3];
  for (int x = 0; x < 3; ++x) { lo[x] = b[x]; hi[x] = b[3 + x]; }
  const TreePiece t = {a.nodes, a.nodes32, a.motion32, a.node_parent, a.arrivals, a.node_base};
  refit_climb(t, a.leaves[3 * (size_t)l + 1], a.leaves[3 * (size_t)l + 2], lo, hi);
}

struct TimedRefitArgs {
  BvhRefitArgs tree;                // motion32: NULL when this BVH gets time-aware boxes (no static copy is written), else as k_refit_bvh's
  const rt::FlatMovingSphere* movers;
  rt::FlatMotion32* time_boxes;     // the scene's motion32 when this BVH gets time-aware boxes, else NULL
  double* scratch;                  // 24 doubles per node of this BVH (scene_update.inc: EndBoxes)
  unsigned int* slope_mask;         // this BVH's word, zero at launch
  double t0, t1;                    // the BVH's own interval
};

// k_refit_bvh for a BVH that holds MovingSpheres, whose values have just changed: one thread per leaf, every leaf.  The leaf's
// union over [t0, t1] climbs into nodes / nodes32 as a static BVH's box does; where the BVH gets time-aware boxes the unions AT
// t0 and AT t1 climb with it and become motion32 (scene_update.inc: refit_climb<true>).  A BVH that gets none -- an interval that
// is not ordered, a scene without motion32 -- takes the plain climb, with the static copy where the scene has motion32.
__global__ __launch_bounds__(256) void k_refit_timed_bvh(TimedRefitArgs a) {
  const int l = (int)(blockIdx.x * 256u + threadIdx.x);
  if (l >= a.tree.n_leaves) return;
  const int32_t code = a.tree.leaves[3 * (size_t)l];
  double b[6];
  timed_leaf_box(code, a.tree.refs, a.tree.spheres, a.movers, a.tree.rects, a.tree.triangles, a.t0, a.t1, b);
  double lo[3], hi[3];
  for (int x = 0; x < 3; ++x) { lo[x] = b[x]; hi[x] = b[3 + x]; }
  const TreePiece t = {a.tree.nodes, a.tree.nodes32, a.tree.motion32, a.tree.node_parent, a.tree.arrivals, a.tree.node_base};
  const int32_t node = a.tree.leaves[3 * (size_t)l + 1], c = a.tree.leaves[3 * (size_t)l + 2];
  if (!a.time_boxes) { refit_climb(t, node, c, lo, hi); return; }
  EndBoxes e;
  e.motion32 = a.time_boxes; e.scratch = a.scratch; e.slope_mask = a.slope_mask;
  timed_leaf_box(code, a.tree.refs, a.tree.spheres, a.movers, a.tree.rects, a.tree.triangles, a.t0, a.t0, e.b[0]);
  timed_leaf_box(code, a.tree.refs, a.tree.spheres, a.movers, a.tree.rects, a.tree.triangles, a.t1, a.t1, e.b[1]);
  refit_climb<true>(t, node, c, lo, hi, &e);
}

// The f64 box the binary tree keeps for child code `code` below node i: the collapse (host/wide_tree.hpp) opens at most two
// nodes, so a slot's code is a child of i, of a child of i, or of a grandchild of i.  false: not there (a record no walk reaches).
__device__ __forceinline__ bool wide_slot_box(const rt::FlatNode* __restrict__ nodes, int32_t i, int32_t code, const rt::FlatNode** at, int* which) {
  for (int c0 = 0; c0 < 2; ++c0)
    if (nodes[i].child[c0] == code) { *at = &nodes[i]; *which = c0; return true; }
  for (int c0 = 0; c0 < 2; ++c0) {
    const int32_t n1 = nodes[i].child[c0];
    if (rt::node_child_is_leaf(n1)) continue;
    for (int c1 = 0; c1 < 2; ++c1)
      if (nodes[n1].child[c1] == code) { *at = &nodes[n1]; *which = c1; return true; }
  }
  for (int c0 = 0; c0 < 2; ++c0) {
    const int32_t n1 = nodes[i].child[c0];
    if (rt::node_child_is_leaf(n1)) continue;
    for (int c1 = 0; c1 < 2; ++c1) {
      const int32_t n2 = nodes[n1].child[c1];
      if (rt::node_child_is_leaf(n2)) continue;
      for (int c2 = 0; c2 < 2; ++c2)
        if (nodes[n2].child[c2] == code) { *at = &nodes[n2]; *which = c2; return true; }
    }
  }
  return false;
}

// One thread per node of ONE BVH, its own launch after the binary refit (plain loads: the kernel boundary made the boxes
// visible).  Every occupied slot of the node's wide record gets the outward-narrowed box of its child code; child codes, empty
// slots (+inf, -inf) and the all-zero records of nodes no wide walk reaches stay as they are.  Child indices read from `nodes`
// are the upload's own (validated by build_mesh_shadow: every one lies inside this BVH's piece).
__global__ __launch_bounds__(256) void k_refit_wide(const rt::FlatNode* __restrict__ nodes, FlatNode4* __restrict__ wide, int32_t node_base, int32_t n_nodes) {
  const int t = (int)(blockIdx.x * 256u + threadIdx.x);
  if (t >= n_nodes) return;
  const int32_t i = node_base + t;
  FlatNode4* w = &wide[i];
  if (w->child[0] == 0 && w->child[1] == 0 && w->child[2] == 0 && w->child[3] == 0) return;  // never opened
  for (int k = 0; k < 4; ++k) {
    const int32_t code = w->child[k];
    if (code == 0x7fffffff) continue;
    const rt::FlatNode* at;
    int c;
    if (!wide_slot_box(nodes, i, code, &at, &c)) continue;
    for (int x = 0; x < 3; ++x) {
      w->lo[x][k] = rt::f32_narrow_down(at->bmin[c][x]);
      w->hi[x][k] = rt::f32_narrow_up(at->bmax[c][x]);
    }
  }
}

// One thread per touched member of an instance tree: list[2 i] = the member's index in d_local_box, list[2 i + 1] = its PRIM /
// GROUP / BVH entry.  After the BVH refits on the same stream.
__global__ __launch_bounds__(256) void k_member_local_boxes(const int32_t* __restrict__ list, int n, const rt::FlatEntry* __restrict__ entries,
                                                           const rt::FlatNode* __restrict__ nodes, const rt::PrimRef* __restrict__ refs,
                                                           const rt::FlatSphere* __restrict__ spheres, const rt::FlatRect* __restrict__ rects,
                                                           const rt::FlatTriangle* __restrict__ triangles, double* __restrict__ local_box) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  double b[6];
  member_local_box_of(entries[list[2 * (size_t)i + 1]], nodes, refs, spheres, rects, triangles, b);
  for (int x = 0; x < 6; ++x) local_box[6 * (size_t)list[2 * (size_t)i] + x] = b[x];
}

// One thread per listed slot: slots[2 i] = the slot, slots[2 i + 1] = 0 a plain triangle, static sphere or rectangle, 1 a medium bounded
// by a sphere, 2 a plain MovingSphere (the record's box, WD_TIME_BOX and its two times by core/mover_box.hpp's rule, as
// build_world_desc sets them: a box that is not finite clears the flag and the times; top_box32 of such a slot is unbounded and stays).  top_box32 (plain only) and the box, the WD_BOXED_PRIM and the WD_PAIR flag of the slot's WorldDesc record, as
// the flattener and build_world_desc derive them; a triangle slot has no WD_SPHERE flag and so no pair rule.  A thread writes
// its own slot's record only; of the next slot's it reads what no update changes (flags other than WD_BOXED_PRIM, g_a).
__global__ __launch_bounds__(256) void k_slot_boxes(const int32_t* __restrict__ slots, int n, int n_top, const rt::FlatEntry* __restrict__ entries,
                                                   const int32_t* __restrict__ top_level, const rt::FlatSphere* __restrict__ spheres,
                                                   const rt::FlatRect* __restrict__ rects, const rt::FlatTriangle* __restrict__ triangles,
                                                   const rt::FlatMovingSphere* __restrict__ movers, float* __restrict__ top_box32,
                                                   WorldDesc* __restrict__ desc) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  const int32_t slot = slots[2 * (size_t)i];
  const bool medium = slots[2 * (size_t)i + 1] == 1;
  const rt::FlatEntry E = entries[top_level[slot]];
  if (slots[2 * (size_t)i + 1] == 2) {
    if (!desc) return;
    const rt::FlatMovingSphere ms = movers[rt::primref_index((rt::PrimRef)E.a)];
    float bx[6];
    for (int x = 0; x < 6; ++x) bx[x] = top_box32[6 * (size_t)slot + x];  // what build_world_desc starts from
    const bool finite = rt::mover_slot_box32(ms, bx);
    for (int x = 0; x < 6; ++x) desc[slot].box[x] = bx[x];
    desc[slot].flags = finite ? (desc[slot].flags | WD_TIME_BOX) : (desc[slot].flags & ~WD_TIME_BOX);
    desc[slot].neg_inv_density = finite ? ms.time0 : rt::real(0);
    desc[slot].aux = finite ? ms.time1 : rt::real(0);
    return;
  }
  const rt::PrimRef ref = (rt::PrimRef)(medium ? entries[E.a].a : E.a);
  float bx[6];
  bool finite = true;
  if (medium) finite = rt::medium_sphere_box32(spheres[rt::primref_index(ref)], bx);
  else {
    rt::plain_slot_box32(ref, spheres, rects, triangles, bx);
    for (int x = 0; x < 6; ++x) {
      top_box32[6 * (size_t)slot + x] = bx[x];
      finite = finite && rt::rt_fabs(bx[x]) < __builtin_huge_valf();
    }
  }
  if (!desc) return;
  for (int x = 0; x < 6; ++x) desc[slot].box[x] = bx[x];
  int32_t flags = finite ? (desc[slot].flags | WD_BOXED_PRIM) : (desc[slot].flags & ~WD_BOXED_PRIM);
  if (!medium && (flags & WD_SPHERE) && slot + 1 < n_top) {
    const int32_t next = desc[slot + 1].flags;
    if ((next & WD_SPHERE) && (next & WD_MEDIUM)) {
      const rt::FlatSphere& a = spheres[rt::primref_index(ref)];
      const rt::FlatSphere& b = spheres[rt::primref_index((rt::PrimRef)desc[slot + 1].g_a)];
      // centre and radius, bit for bit (build_world_desc compares the bytes)
      const bool same = __double_as_longlong(a.cx) == __double_as_longlong(b.cx) && __double_as_longlong(a.cy) == __double_as_longlong(b.cy) &&
                        __double_as_longlong(a.cz) == __double_as_longlong(b.cz) && __double_as_longlong(a.radius) == __double_as_longlong(b.radius);
      flags = same ? (flags | WD_PAIR) : (flags & ~WD_PAIR);
    }
  }
  desc[slot].flags = flags;
}

// ONE block.  A thread per light (in strides of the block) for the area and the pick weight; then one thread for the serial
// sum, the fallback and the cdf: lights are few, and the serial order of the additions is what makes the bytes the host's.
// Every light's area is stored back, a rectangle's as a sphere's: light_area_centre is the function that built the table, so an
// untouched light gets the bytes it had.
__global__ __launch_bounds__(256) void k_refresh_lights(rt::SceneView sv, rt::FlatLight* __restrict__ lights, int32_t n_lights, double* __restrict__ weight) {
  for (int32_t k = (int32_t)threadIdx.x; k < n_lights; k += 256) {
    rt::Point3 centre;
    const rt::real area = rt::light_area_centre(lights[k], sv.spheres, sv.rects, &centre);
    lights[k].area = area;
    weight[k] = rt::light_pick_weight(sv, lights[k].mat, area, centre);
  }
  __syncthreads();
  if (threadIdx.x == 0) rt::light_cdf_pass(lights, weight, n_lights);
}

// ------------------------------------------------------------------ host side
// The shadow's leaf and parent tables go up with the first update of either kind.
static rtx_status upload_mesh_tables(DeviceScene* ds) {
  MeshUpdate& mu = ds->mesh;
  const MeshShadow& sh = mu.shadow;
  if (mu.uploaded) return RTX_OK;
  if (!sh.leaves.empty()) HIP_TRY(mu.d_leaves.upload(sh.leaves.data(), sh.leaves.size()));
  if (!sh.node_parent.empty()) {
    HIP_TRY(mu.d_node_parent.upload(sh.node_parent.data(), sh.node_parent.size()));
    HIP_TRY(mu.d_arrivals.alloc(sh.node_parent.size() / 2 * sizeof(unsigned int)));
  }
  mu.uploaded = true;
  return RTX_OK;
}

// Every touched BVH refitted whole on `stream`: k_refit_bvh, then k_refit_wide where the scene has a 4-wide tree.
static rtx_status launch_bvh_refits(DeviceScene* ds, const std::vector<int32_t>& bvhs, hipStream_t stream) {
  MeshUpdate& mu = ds->mesh;
  for (int32_t bi : bvhs) {
    const BvhShadow& b = mu.shadow.bvhs[(size_t)bi];
    if (b.n_leaves == 0 || b.n_nodes == 0) continue;  // a leaf code for a root: only its primitives changed
    BvhRefitArgs a;
    a.nodes = (rt::FlatNode*)ds->view.nodes; a.nodes32 = (rt::FlatNode32*)ds->view.nodes32; a.motion32 = (rt::FlatMotion32*)ds->view.motion32;
    a.refs = ds->view.refs + b.first_ref;
    a.spheres = ds->view.spheres; a.rects = ds->view.rects; a.triangles = ds->view.triangles;
    a.leaves = mu.d_leaves + 3 * (size_t)b.leaf_first;
    a.node_parent = mu.d_node_parent + 2 * (size_t)b.node_first;
    a.arrivals = mu.d_arrivals + (size_t)b.node_first;
    a.n_leaves = b.n_leaves; a.node_base = b.node_base;
    HIP_TRY(hipMemsetAsync(a.arrivals, 0, (size_t)b.n_nodes * sizeof(unsigned int), stream));
    hipLaunchKernelGGL(k_refit_bvh, dim3((unsigned)((b.n_leaves + 255) / 256)), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    if (ds->wide.nodes4) {
      hipLaunchKernelGGL(k_refit_wide, dim3((unsigned)((b.n_nodes + 255) / 256)), dim3(256), 0, stream, (const rt::FlatNode*)ds->view.nodes,
                         (FlatNode4*)ds->wide.nodes4, b.node_base, b.n_nodes);
      HIP_TRY(hipGetLastError());
    }
  }
  return RTX_OK;
}

// The same for an update of MovingSpheres: k_refit_timed_bvh per touched BVH, with the climb's scratch and the slope words
// (allocated here, by the first such update); then the words on their way to launch_lds where a k_trace_lds plan hangs on them.
static rtx_status launch_timed_refits(DeviceScene* ds, const std::vector<int32_t>& bvhs, hipStream_t stream) {
  MeshUpdate& mu = ds->mesh;
  const size_t n_bvh_nodes = mu.shadow.node_parent.size() / 2;
  bool slopes = false;
  for (int32_t bi : bvhs) {
    const BvhShadow& b = mu.shadow.bvhs[(size_t)bi];
    if (b.n_leaves == 0 || b.n_nodes == 0) continue;  // a leaf code for a root: only its records changed
    const bool time_boxes = b.time_boxes && ds->view.motion32;
    if (time_boxes && !mu.d_end_boxes) HIP_TRY(mu.d_end_boxes.alloc(24 * n_bvh_nodes * sizeof(double)));
    if (time_boxes && !mu.d_slope_mask) HIP_TRY(mu.d_slope_mask.upload(mu.slope_mask.data(), mu.slope_mask.size()));
    TimedRefitArgs a;
    a.tree.nodes = (rt::FlatNode*)ds->view.nodes; a.tree.nodes32 = (rt::FlatNode32*)ds->view.nodes32;
    a.tree.motion32 = time_boxes ? nullptr : (rt::FlatMotion32*)ds->view.motion32;
    a.tree.refs = ds->view.refs + b.first_ref;
    a.tree.spheres = ds->view.spheres; a.tree.rects = ds->view.rects; a.tree.triangles = ds->view.triangles;
    a.tree.leaves = mu.d_leaves + 3 * (size_t)b.leaf_first;
    a.tree.node_parent = mu.d_node_parent + 2 * (size_t)b.node_first;
    a.tree.arrivals = mu.d_arrivals + (size_t)b.node_first;
    a.tree.n_leaves = b.n_leaves; a.tree.node_base = b.node_base;
    a.movers = ds->view.moving_spheres;
    a.time_boxes = time_boxes ? (rt::FlatMotion32*)ds->view.motion32 : nullptr;
    a.scratch = time_boxes ? mu.d_end_boxes + 24 * (size_t)b.node_first : nullptr;
    a.slope_mask = time_boxes ? mu.d_slope_mask + (size_t)bi : nullptr;
    a.t0 = b.t0; a.t1 = b.t1;
    HIP_TRY(hipMemsetAsync(a.tree.arrivals, 0, (size_t)b.n_nodes * sizeof(unsigned int), stream));
    if (time_boxes) HIP_TRY(hipMemsetAsync(a.slope_mask, 0, sizeof(unsigned int), stream));
    hipLaunchKernelGGL(k_refit_timed_bvh, dim3((unsigned)((b.n_leaves + 255) / 256)), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    slopes = slopes || time_boxes;
    if (ds->wide.nodes4) {
      hipLaunchKernelGGL(k_refit_wide, dim3((unsigned)((b.n_nodes + 255) / 256)), dim3(256), 0, stream, (const rt::FlatNode*)ds->view.nodes,
                         (FlatNode4*)ds->wide.nodes4, b.node_base, b.n_nodes);
      HIP_TRY(hipGetLastError());
    }
  }
  // a k_trace_lds plan is a world of ONE BVH: its word is the first (and only) one
  if (slopes && ds->lds.motion_planned) HIP_TRY(mu.slope_readback.fetch(mu.d_slope_mask, 1, stream));
  return RTX_OK;
}

// The local boxes of the touched members (d_members: index, entry per member, in the call's staging), then the instance trees
// above them.  After the BVH refits on the same stream.
static rtx_status launch_member_refits(DeviceScene* ds, const int32_t* d_members, size_t n_members, const std::vector<int32_t>& trees, hipStream_t stream) {
  SceneUpdate& u = ds->upd;
  if (!n_members) return RTX_OK;
  hipLaunchKernelGGL(k_member_local_boxes, dim3((unsigned)((n_members + 255) / 256)), dim3(256), 0, stream, d_members, (int)n_members,
                     ds->view.entries, ds->view.nodes, ds->view.refs, ds->view.spheres, ds->view.rects, ds->view.triangles, (double*)u.d_local_box);
  HIP_TRY(hipGetLastError());
  ds->mesh.local_box_stale = true;
  for (int32_t t : trees) {
    const rtx_status st = launch_instance_refit(ds, u.shadow.trees[(size_t)t], stream);
    if (st != RTX_OK) return st;
  }
  return RTX_OK;
}

// k_trace_vote's copy of the top-level rectangle records (render.hip: VoteTop, a kernel argument made at upload) after an update
// of rectangles.  pairs: 2 per flat rectangle, its index and the index of its values.  values (host memory): the copy takes them
// by the function the kernel stores them with, before the call returns -- a launch reads its arguments when it is enqueued, so
// a render enqueued after this call sees the new records and one enqueued before it the old, as with `rects` itself on one
// stream.  values == NULL (the device entry: the host never sees them): a copy that holds a touched rectangle is given up for
// good, top.n = -1, and every later launch walks the world list as it does for a world of more than eight plain entries -- the
// same hits, three dependent scalar loads per entry and ray instead of one (DESIGN.md 8.8).
static void refresh_vote_top(DeviceScene* ds, const std::vector<int32_t>& pairs, const double* values) {
  VoteTop& top = ds->vote.top;
  if (top.n < 0) return;
  for (size_t k = 0; k < pairs.size(); k += 2)
    for (int32_t i = 0; i < top.n; ++i) {
      if (rt::primref_type((rt::PrimRef)top.ref[i]) != rt::PRIM_RECT || rt::primref_index((rt::PrimRef)top.ref[i]) != (uint32_t)pairs[k]) continue;
      if (!values) { top.n = -1; return; }
      rt::set_rect_values(&top.rect[i], values + 5 * (size_t)pairs[k + 1]);
    }
}

// ids (host memory) have passed check_prim_ids against ds->mesh.shadow.  values: host memory (staged here, one copy) when
// host_values, else a device pointer.  Everything that can refuse comes first; then one copy and the launches, all on `stream`.
static rtx_status scene_set_prims_impl(DeviceScene* ds, const PrimKind& K, const char* who, const int32_t* ids, int64_t n, const double* values,
                                       bool host_values, hipStream_t stream) {
  MeshUpdate& mu = ds->mesh;
  const MeshShadow& sh = mu.shadow;
  const bool tri = K.type == rt::PRIM_TRIANGLE, mov = K.type == rt::PRIM_MOVING_SPHERE, rect = K.type == rt::PRIM_RECT;
  std::string err;
  UpdatePlan plan;
  const rtx_status pst = plan_prim_update(K, who, sh, ids, n, &plan, &err);
  if (pst != RTX_OK) { set_error(err); return pst; }
  const rtx_status dst = check_scene_device(ds, who, "was uploaded to");
  if (dst != RTX_OK) return dst;
  rtx_status st = upload_mesh_tables(ds);
  if (st != RTX_OK) return st;
  bool lights = false;  // a listed sphere or rectangle is a sampled light
  const std::vector<char>& is_light = rect ? mu.rect_is_light : mu.sphere_is_light;
  for (int64_t i = 0; !tri && !mov && i < n; ++i) lights = lights || ((size_t)ids[i] < is_light.size() && is_light[(size_t)ids[i]]);
  if (lights && !mu.d_light_weight) HIP_TRY(mu.d_light_weight.alloc((size_t)ds->lights.n_lights * sizeof(double)));
  // staging layout: [values, width x 8 B each (host entry only)] [pairs] [members: index, entry] [slots: slot, kind]
  const size_t value_bytes = host_values ? (size_t)n * (size_t)K.width * sizeof(double) : 0;
  const size_t n_pairs = plan.pairs.size() / 2, n_members = plan.members.size(), n_slots = plan.slots.size() / 2;
  const size_t bytes = value_bytes + (2 * n_pairs + 2 * n_members + 2 * n_slots) * sizeof(int32_t);
  void* pinned = nullptr;
  HIP_TRY(mu.staging.reserve(bytes, stream, &pinned));
  unsigned char* h = (unsigned char*)pinned;
  if (host_values) memcpy(h, values, value_bytes);
  int32_t* h_pairs = (int32_t*)(h + value_bytes);
  int32_t* h_members = h_pairs + 2 * n_pairs;
  int32_t* h_slots = h_members + 2 * n_members;
  memcpy(h_pairs, plan.pairs.data(), 2 * n_pairs * sizeof(int32_t));
  for (size_t k = 0; k < n_members; ++k) { h_members[2 * k] = plan.members[k]; h_members[2 * k + 1] = sh.members[(size_t)plan.members[k]].geom; }
  if (n_slots) memcpy(h_slots, plan.slots.data(), 2 * n_slots * sizeof(int32_t));
  HIP_TRY(mu.staging.copy(bytes, stream));
  unsigned char* d = mu.staging.device();
  const double* d_values = host_values ? (const double*)d : values;
  const int32_t* d_pairs = (const int32_t*)(d + value_bytes);
  const int32_t* d_members = d_pairs + 2 * n_pairs;
  const int32_t* d_slots = d_members + 2 * n_members;
  const dim3 pair_grid((unsigned)((n_pairs + 255) / 256));
  if (rect) refresh_vote_top(ds, plan.pairs, host_values ? values : nullptr);  // (nothing below refuses: only a HIP error ends the call early)
  if (rect) hipLaunchKernelGGL((k_set_prims<5, rt::FlatRect>), pair_grid, dim3(256), 0, stream, d_pairs, (int)n_pairs, d_values, (rt::FlatRect*)ds->view.rects);
  else if (tri) hipLaunchKernelGGL((k_set_prims<9, rt::FlatTriangle>), pair_grid, dim3(256), 0, stream, d_pairs, (int)n_pairs, d_values, (rt::FlatTriangle*)ds->view.triangles);
  else if (mov) hipLaunchKernelGGL((k_set_prims<7, rt::FlatMovingSphere>), pair_grid, dim3(256), 0, stream, d_pairs, (int)n_pairs, d_values, (rt::FlatMovingSphere*)ds->view.moving_spheres);
  else hipLaunchKernelGGL((k_set_prims<4, rt::FlatSphere>), pair_grid, dim3(256), 0, stream, d_pairs, (int)n_pairs, d_values, (rt::FlatSphere*)ds->view.spheres);
  HIP_TRY(hipGetLastError());
  if ((st = mov ? launch_timed_refits(ds, plan.bvhs, stream) : launch_bvh_refits(ds, plan.bvhs, stream)) != RTX_OK) return st;
  if ((st = launch_member_refits(ds, d_members, n_members, plan.trees, stream)) != RTX_OK) return st;
  if (n_slots) {
    hipLaunchKernelGGL(k_slot_boxes, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, stream, d_slots, (int)n_slots, ds->view.n_top_level,
                       ds->view.entries, ds->view.top_level, ds->view.spheres, ds->view.rects, ds->view.triangles, ds->view.moving_spheres,
                       (float*)ds->view.top_box32, (WorldDesc*)ds->world.desc);
    HIP_TRY(hipGetLastError());
  }
  if (lights) {
    hipLaunchKernelGGL(k_refresh_lights, dim3(1), dim3(256), 0, stream, ds->view, (rt::FlatLight*)ds->lights.lights, ds->lights.n_lights,
                       (double*)mu.d_light_weight);
    HIP_TRY(hipGetLastError());
  }
  return RTX_OK;
}
