// rtx_scene_set_transforms on a resident scene (included by render.hip, namespace rtx; compiled by both compilations).
//
// New parameters for the Translate / RotateY chains of top-level slots reach three device arrays and no other:
//   entries[xform].ops      what every scan transforms a ray by (core/geometry.hpp)
//   WorldDesc[slot].ops     k_trace_world's copy of the same ops (trace_world.inc)
//   nodes / nodes32 / motion32 of the instance tree the slot is a member of: the members' boxes in WORLD space
// k_set_slot_ops scatters the first two; k_refit_instance_tree recomputes the third for one tree, bottom-up, with the
// arithmetic the flattener used (core/member_box.hpp), so that the arrays equal those of a scene flattened and uploaded from
// scratch with the new parameters -- the judge of tests/test_gpu_set_transforms.py.  Topology is not touched: child codes,
// split axes and every other array stay as uploaded, and no existing kernel changes.
//
// What the other updates of a resident scene share lives here too, once: refit_climb (the bottom-up climb of this refit and of
// mesh_update.inc's k_refit_bvh and k_refit_timed_bvh, with the one statement of its cross-workgroup visibility), store_child_planes32 (the narrowed
// planes of a child; also scene_rebuild.inc's k_rebuild_emit) and, on the host side, check_scene_device.  A member's world box
// is core/member_box.hpp's member_world_box; the pinned staging of a call is device_buffer.hpp's StagingBuffer.
//
// The boxes are computed in f64 in BOTH compilations and narrowed last: an f32 scene's node planes are the f64 planes rounded
// down / up (host/f32_layout.hpp: "d6 u6"), so its refit starts from the f64 ops it keeps in SceneUpdate::slot_ops64 -- the
// ops in its own entries went through a (float) cast.  Min and max commute with a monotone rounding, so above the leaves the
// f32 compilation unites the narrowed planes and still gets the narrowed unions.

// One update as the device takes it: the slot, its ENTRY_XFORM and the resolved ops (a rotate_y as sin, cos).
struct SlotOpsRecord {  // 144 B
  int32_t slot, xform, n_ops, pad;
  rt::XformOp64 ops[RT_MAX_XFORM_OPS];
};

// One thread per update.  The host has checked slot, xform and n_ops against the scene (host/update_shadow.hpp).
__global__ __launch_bounds__(256) void k_set_slot_ops(const SlotOpsRecord* __restrict__ rec, int n, rt::FlatEntry* __restrict__ entries,
                                                     WorldDesc* __restrict__ desc, rt::XformOp64* __restrict__ slot_ops64) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  const int32_t slot = rec[i].slot, xform = rec[i].xform;
  const int n_ops = rec[i].n_ops < RT_MAX_XFORM_OPS ? rec[i].n_ops : RT_MAX_XFORM_OPS;
  for (int k = 0; k < n_ops; ++k) {
    const rt::XformOp64 in = rec[i].ops[k];
    rt::FlatXformOp o;
    o.op = in.op; o.pad = 0;
    for (int a = 0; a < 3; ++a) o.v[a] = (rt::real)in.v[a];  // the converter's cast (host/f32_layout.hpp: 'r')
    entries[xform].ops[k] = o;
    desc[slot].ops[k] = o;
    if (slot_ops64) slot_ops64[(size_t)slot * RT_MAX_XFORM_OPS + k] = in;
  }
}

struct RefitArgs {
  const rt::FlatEntry* entries;
  const int32_t* top_level;
  rt::FlatNode* nodes;
  rt::FlatNode32* nodes32;
  rt::FlatMotion32* motion32;         // NULL: the scene has no time-aware boxes
  const double* local_box;            // 6 per member, this tree's first member first
  const int32_t* leaf_parent;         // 2 per member: node, child index
  const int32_t* node_parent;         // 2 per node of this tree, by node - node_base: parent (-1: root), child index
  unsigned int* arrivals;             // 1 per node of this tree, zero at launch
  const rt::XformOp64* slot_ops64;    // the f32 compilation's f64 ops, RT_MAX_XFORM_OPS per slot; NULL in the f64 compilation
  int32_t first_slot, n_slots, node_base;
};

__device__ __forceinline__ rt::real refit_plane_down(double x) {
#ifdef RT_F32
  return rt::f32_narrow_down(x);
#else
  return x;
#endif
}
__device__ __forceinline__ rt::real refit_plane_up(double x) {
#ifdef RT_F32
  return rt::f32_narrow_up(x);
#else
  return x;
#endif
}

// Axis x of child c of `node` where the f32 walkers read it: the plane pair narrowed outward into FlatNode32 and, where the
// scene has time-aware boxes, into FlatMotion32 as a static box without slopes (flatten.cpp: build_motion_boxes gives that to an
// instance tree, which has no time interval, and to a BVH without a moving sphere).  Plain stores: each field is written by one
// thread and read by nobody in the same launch.
__device__ __forceinline__ void store_child_planes32(rt::FlatNode32* nodes32, rt::FlatMotion32* motion32, int32_t node, int c, int x, rt::real lo,
                                                     rt::real hi) {
  const float l32 = rt::f32_narrow_down((double)lo), h32 = rt::f32_narrow_up((double)hi);
  nodes32[node].lo[c][x] = l32;
  nodes32[node].hi[c][x] = h32;
  if (motion32) {
    motion32[node].lo0[c][x] = l32; motion32[node].hi0[c][x] = h32;
    motion32[node].dlo[c][x] = 0.0f; motion32[node].dhi[c][x] = 0.0f;
  }
}

// One binary tree as a refit climbs it (an instance tree here, a BVH in mesh_update.inc): its nodes are
// nodes[node_base .. node_base + n), and node_parent and arrivals are indexed by node - node_base.
struct TreePiece {
  rt::FlatNode* nodes;
  rt::FlatNode32* nodes32;
  rt::FlatMotion32* motion32;  // NULL: the scene has no time-aware boxes
  const int32_t* node_parent;  // 2 per node: parent (-1: root), child index
  unsigned int* arrivals;      // 1 per node, zero at launch
  int32_t node_base;
};

// What a climber of a BVH with time-aware boxes carries beside (lo, hi) (mesh_update.inc: k_refit_timed_bvh; TIMED below): the
// unions of its subtree AT the BVH's time0 and AT its time1, in f64 -- FlatMotion32 keeps only their narrowed planes and slopes,
// so a parent could not be derived from its children's records.
struct EndBoxes {
  double b[2][6];              // [at time0, at time1][lo xyz, hi xyz]
  rt::FlatMotion32* motion32;  // the scene's, not NULL (TreePiece::motion32 is NULL for such a climb: no static copy is written)
  double* scratch;             // 24 doubles per node of the piece, by node - node_base: [end][child][lo xyz, hi xyz]
  unsigned int* slope_mask;    // this BVH's word: the OR of core/mover_box.hpp's axis bits over every slope written
};

// THE bottom-up climb of every refit.  A thread comes with the box (lo, hi) of child c of `node`: it writes the box where the
// node keeps it and arrives at the node.  Of the two threads that reach a node the first leaves; the second unites the node's
// two child boxes and carries the union to the node's place in ITS parent, up to the root.  Unions are exact min / max, so the
// result does not depend on who arrives first.  TIMED: the two end boxes travel the same way; at every node the climber writes
// child c's time-aware planes from them (core/mover_box.hpp: motion_child_planes) and parks them in the scratch for its sibling.
// Visibility across workgroups is lbvh.hip's k_refit recipe (MI355X_MICROARCH.md, inter-workgroup visibility: a CU's L1 is
// never refreshed by another CU's stores, and the XCDs' L2s are not coherent): agent-scope relaxed stores of the FlatNode
// planes -- and, TIMED, of the end boxes in the scratch -- which a sibling's climber on another CU reads; __threadfence; the
// agent-scope atomic arrival; __threadfence; agent-scope relaxed loads of the sibling's planes and end boxes -- a plain load
// could be served stale from this CU's L1.  (nodes32 and motion32 are written with plain stores: nobody reads them in the
// launch.  The slope mask is an agent-scope atomic OR that only the host reads, after the kernel.)
template <bool TIMED = false>
__device__ __forceinline__ void refit_climb(const TreePiece& t, int32_t node, int32_t c, rt::real* lo, rt::real* hi, EndBoxes* e = nullptr) {
  unsigned int moves = 0u;
  for (;;) {
    rt::FlatNode* nd = &t.nodes[node];
    for (int x = 0; x < 3; ++x) {
      __hip_atomic_store(&nd->bmin[c][x], lo[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&nd->bmax[c][x], hi[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      store_child_planes32(t.nodes32, t.motion32, node, c, x, lo[x], hi[x]);
    }
    const int32_t rel = node - t.node_base;
    if constexpr (TIMED) {
      rt::FlatMotion32* m = &e->motion32[node];
      moves |= rt::motion_child_planes(e->b[0], e->b[1], m->lo0[c], m->dlo[c], m->hi0[c], m->dhi[c]);
      double* mine = e->scratch + 24 * (size_t)rel + 6 * c;
      for (int end = 0; end < 2; ++end)
        for (int k = 0; k < 6; ++k) __hip_atomic_store(&mine[12 * end + k], e->b[end][k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const int32_t parent = t.node_parent[2 * (size_t)rel], pc = t.node_parent[2 * (size_t)rel + 1];
    auto leave = [&] {  // (a climber ORs the axes of all the slopes it wrote, once)
      if constexpr (TIMED)
        if (moves) (void)__hip_atomic_fetch_or(e->slope_mask, moves, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    if (parent < 0) { leave(); return; }  // the root: its two child boxes are the whole tree
    __threadfence();
    if (atomicAdd(&t.arrivals[rel], 1u) == 0u) { leave(); return; }  // first of the two: the sibling's climber finishes the node
    __threadfence();
    for (int x = 0; x < 3; ++x) {
      const rt::real slo = __hip_atomic_load(&nd->bmin[1 - c][x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const rt::real shi = __hip_atomic_load(&nd->bmax[1 - c][x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      lo[x] = rt::rt_fmin(lo[x], slo);
      hi[x] = rt::rt_fmax(hi[x], shi);
    }
    if constexpr (TIMED) {
      const double* theirs = e->scratch + 24 * (size_t)rel + 6 * (1 - c);
      for (int end = 0; end < 2; ++end)
        for (int x = 0; x < 3; ++x) {
          const double slo = __hip_atomic_load(&theirs[12 * end + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          const double shi = __hip_atomic_load(&theirs[12 * end + 3 + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          e->b[end][x] = rt::rt_fmin(e->b[end][x], slo);
          e->b[end][3 + x] = rt::rt_fmax(e->b[end][3 + x], shi);
        }
    }
    node = parent;
    c = pc;
  }
}

// One thread per member slot of ONE tree -- every member, not only the moved ones: the member's world box, then the climb.
__global__ __launch_bounds__(256) void k_refit_instance_tree(RefitArgs a) {
  const int m = (int)(blockIdx.x * 256u + threadIdx.x);
  if (m >= a.n_slots) return;
  const int32_t slot = a.first_slot + m;
  double b[6];
  rt::member_world_box(a.entries[a.top_level[slot]], slot, a.slot_ops64, a.local_box + 6 * (size_t)m, b);
  rt::real lo[3], hi[3];
  for (int x = 0; x < 3; ++x) { lo[x] = refit_plane_down(b[x]); hi[x] = refit_plane_up(b[3 + x]); }
  const TreePiece t = {a.nodes, a.nodes32, a.motion32, a.node_parent, a.arrivals, a.node_base};
  refit_climb(t, a.leaf_parent[2 * (size_t)m], a.leaf_parent[2 * (size_t)m + 1], lo, hi);
}

// ------------------------------------------------------------------ host side
// What an update needs beside the scene's arrays, built once at upload (scene_upload_impl).
static rtx_status build_scene_update(DeviceScene* ds, const FlatScene& fs) {
  SceneUpdate& u = ds->upd;
  u.shadow = build_update_shadow(fs);
  u.local_box = fs.member_local_box;
  u.n_entries = fs.entries.size(); u.n_nodes = fs.nodes.size(); u.n_motion = fs.motion32.size();
  u.n_desc = fs.top_level.size();
  u.n_triangles = fs.triangles.size(); u.n_top = fs.top_box32.size() / 6; u.n_spheres = fs.spheres.size();
  u.n_moving_spheres = fs.moving_spheres.size();
  u.n_rects = fs.rects.size();
#ifndef RTX_F32_TU
  ds->mesh.shadow = build_mesh_shadow(fs, u.shadow);  // rtx_scene_set_triangles (mesh_update.inc); its tables go up with the first update
  // per BVH, the axes along which its time-aware boxes have a slope as uploaded: what k_refit_timed_bvh keeps current from then on
  ds->mesh.slope_mask.assign(ds->mesh.shadow.bvhs.size(), 0u);
  if (ds->mesh.shadow.broken.empty() && !fs.motion32.empty())
    for (size_t b = 0; b < ds->mesh.shadow.bvhs.size(); ++b) {
      const BvhShadow& B = ds->mesh.shadow.bvhs[b];
      ds->mesh.slope_mask[b] = rt::motion_slope_mask(fs.motion32.data() + B.node_base, (size_t)B.n_nodes);
    }
#endif
  if (fs.features & rt::F_INSTANCE)
    for (const rt::FlatEntry& e : fs.entries) u.n_desc += e.kind == rt::ENTRY_INSTANCE ? 1 : 0;
  if (!u.shadow.broken.empty() || u.shadow.trees.empty()) return RTX_OK;
  // the parts of max_stack (flatten.cpp: inst_depth + 1 + the members' deepest BVH), kept apart for a rebuild
  for (const TreeShadow& t : u.shadow.trees) u.tree_depth.push_back(instance_tree_depth(fs.nodes.data(), t.root));
  u.member_stack = fs.max_stack - instance_max_stack(0, u.tree_depth);
  HIP_TRY(u.d_local_box.upload(u.local_box.data(), u.local_box.size()));
  HIP_TRY(u.d_leaf_parent.upload(u.shadow.leaf_parent.data(), u.shadow.leaf_parent.size()));
  HIP_TRY(u.d_node_parent.upload(u.shadow.node_parent.data(), u.shadow.node_parent.size()));
  HIP_TRY(u.d_arrivals.alloc(u.shadow.node_parent.size() / 2 * sizeof(unsigned int)));
#ifdef RT_F32
  if (fs.slot_ops64.size() != fs.top_level.size() * RT_MAX_XFORM_OPS) {
    u.shadow.broken = "the f32 scene did not receive the f64 ops of its slots";
    return RTX_OK;
  }
  HIP_TRY(u.d_slot_ops64.upload(fs.slot_ops64.data(), fs.slot_ops64.size()));
#endif
  return RTX_OK;
}

// A resident scene is edited and read on its own device only.  verb: "was uploaded to" (the updates) or "lives on" (the readers).
static rtx_status check_scene_device(const DeviceScene* ds, const char* who, const char* verb) {
  int cur = -1;
  HIP_TRY(hipGetDevice(&cur));
  if (cur != ds->device) { set_error(std::string(who) + ": scene " + verb + " a different device than the current one"); return RTX_EINVAL; }
  return RTX_OK;
}

// Instance tree t refitted on `stream` from d_local_box and the ops now in `entries` (also mesh_update.inc's last step).
static rtx_status launch_instance_refit(DeviceScene* ds, const TreeShadow& t, hipStream_t stream) {
  SceneUpdate& u = ds->upd;
  RefitArgs a;
  a.entries = ds->view.entries; a.top_level = ds->view.top_level;
  a.nodes = (rt::FlatNode*)ds->view.nodes; a.nodes32 = (rt::FlatNode32*)ds->view.nodes32; a.motion32 = (rt::FlatMotion32*)ds->view.motion32;
  a.local_box = u.d_local_box + 6 * (size_t)t.member_first;
  a.leaf_parent = u.d_leaf_parent + 2 * (size_t)t.member_first;
  a.node_parent = u.d_node_parent + 2 * (size_t)t.node_first;
  a.arrivals = u.d_arrivals + (size_t)t.node_first;
  a.slot_ops64 = u.d_slot_ops64;
  a.first_slot = t.first_slot; a.n_slots = t.n_slots; a.node_base = t.node_base;
  HIP_TRY(hipMemsetAsync(a.arrivals, 0, (size_t)t.n_nodes * sizeof(unsigned int), stream));
  hipLaunchKernelGGL(k_refit_instance_tree, dim3((unsigned)((t.n_slots + 255) / 256)), dim3(256), 0, stream, a);
  HIP_TRY(hipGetLastError());
  return RTX_OK;
}

// `resolved` (host memory, n > 0) has passed check_slot_ops_shape.  Every check against the scene comes first; then one copy,
// k_set_slot_ops and one k_refit_instance_tree per tree that holds an updated member, all on `stream`.
static rtx_status scene_set_transforms_impl(DeviceScene* ds, const RtxSlotOps* resolved, int64_t n, hipStream_t stream) {
  SceneUpdate& u = ds->upd;
  std::string err;
  const rtx_status dst = check_scene_device(ds, "rtx_scene_set_transforms", "was uploaded to");
  if (dst != RTX_OK) return dst;
#ifndef RTX_F32_TU
  if (ds->mesh.local_box_stale) {
    // rtx_scene_set_triangles* (either entry) recomputed members' local boxes on the device only -- the host holds neither the
    // refitted nodes nor the untouched primitives of a touched member -- and the check below reads the host copy: the FIRST
    // set_transforms after such an update waits for the device once and reads the boxes back (include/rtx_abi.h says so)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(u.local_box.data(), (const double*)u.d_local_box, u.local_box.size() * sizeof(double), hipMemcpyDeviceToHost));
    ds->mesh.local_box_stale = false;
  }
#endif
  if (!check_slot_ops_scene("rtx_scene_set_transforms", u.shadow, u.local_box.data(), resolved, n, &err)) { set_error(err); return RTX_EINVAL; }
  const size_t bytes = (size_t)n * sizeof(SlotOpsRecord);
  void* h = nullptr;
  HIP_TRY(u.staging.reserve(bytes, stream, &h));
  SlotOpsRecord* rec = (SlotOpsRecord*)h;
  std::vector<char> touched(u.shadow.trees.size(), 0);
  for (int64_t i = 0; i < n; ++i) {
    const SlotChain& c = u.shadow.slots[(size_t)resolved[i].slot];
    memset(&rec[i], 0, sizeof(SlotOpsRecord));
    rec[i].slot = resolved[i].slot; rec[i].xform = c.xform; rec[i].n_ops = c.n_ops;
    static_assert(sizeof(rec[i].ops) == sizeof(resolved[i].ops), "RtxSlotOps::ops is rt::XformOp64");
    memcpy(rec[i].ops, resolved[i].ops, sizeof(rec[i].ops));
    if (c.tree >= 0) touched[(size_t)c.tree] = 1;
  }
  HIP_TRY(u.staging.copy(bytes, stream));
  hipLaunchKernelGGL(k_set_slot_ops, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const SlotOpsRecord*)u.staging.device(),
                     (int)n, (rt::FlatEntry*)ds->view.entries, (WorldDesc*)ds->world.desc, (rt::XformOp64*)u.d_slot_ops64);
  HIP_TRY(hipGetLastError());
  for (size_t k = 0; k < u.shadow.trees.size(); ++k) {
    if (!touched[k]) continue;
    const rtx_status st = launch_instance_refit(ds, u.shadow.trees[k], stream);
    if (st != RTX_OK) return st;
  }
  return RTX_OK;
}

// rtx_device_scene_array: one resident array back to the host, after everything enqueued on the device.
static rtx_status scene_read_array_impl(DeviceScene* ds, int32_t which, void* out, size_t bytes) {
  const SceneUpdate& u = ds->upd;
  const void* p = nullptr;
  size_t have = 0;
  switch (which) {
    case 0: p = ds->view.entries; have = u.n_entries * sizeof(rt::FlatEntry); break;
    case 1: p = ds->view.nodes; have = u.n_nodes * sizeof(rt::FlatNode); break;
    case 2: p = ds->view.nodes32; have = u.n_nodes * sizeof(rt::FlatNode32); break;
    case 3: p = ds->view.motion32; have = u.n_motion * sizeof(rt::FlatMotion32); break;
    case 4: p = ds->world.desc; have = u.n_desc * sizeof(WorldDesc); break;
    case 10: p = ds->view.triangles; have = u.n_triangles * sizeof(rt::FlatTriangle); break;
    case 11: p = ds->view.top_box32; have = u.n_top * 6 * sizeof(float); break;
    case 13: p = ds->view.spheres; have = u.n_spheres * sizeof(rt::FlatSphere); break;
    case 14: p = ds->lights.lights; have = (size_t)ds->lights.n_lights * sizeof(rt::FlatLight); break;
    case 15: p = ds->view.materials; have = u.n_materials * sizeof(rt::FlatMaterial); break;
    case 16: p = ds->view.textures; have = u.n_textures * sizeof(rt::FlatTexture); break;
    case 17: p = ds->view.moving_spheres; have = u.n_moving_spheres * sizeof(rt::FlatMovingSphere); break;
    case 19: p = ds->view.rects; have = u.n_rects * sizeof(rt::FlatRect); break;
    case 7: p = ds->wide.nodes4; have = ds->wide.nodes4 ? u.n_nodes * sizeof(FlatNode4) : 0; break;
    case 9:  // max_stack as the binary walks are now launched with: host memory, one int32
      if (bytes != sizeof(int32_t) || !out) { set_error("rtx_device_scene_array: the array holds 4 bytes, not " + std::to_string(bytes)); return RTX_EINVAL; }
      *(int32_t*)out = ds->view.max_stack;
      return RTX_OK;
    case 8:  // the stack levels of a wide walk: host memory, one int32
      if (bytes != sizeof(int32_t) || !out) { set_error("rtx_device_scene_array: the array holds 4 bytes, not " + std::to_string(bytes)); return RTX_EINVAL; }
      *(int32_t*)out = ds->wide.nodes4 ? (int32_t)ds->wide.levels : 0;
      return RTX_OK;
    default: set_error("rtx_device_scene_array: which names no resident array"); return RTX_EINVAL;
  }
  if (bytes != have) { set_error("rtx_device_scene_array: the array holds " + std::to_string(have) + " bytes, not " + std::to_string(bytes)); return RTX_EINVAL; }
  if (have == 0) return RTX_OK;
  if (!out) { set_error("rtx_device_scene_array: out is NULL"); return RTX_EINVAL; }
  const rtx_status dst = check_scene_device(ds, "rtx_device_scene_array", "lives on");
  if (dst != RTX_OK) return dst;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, p, have, hipMemcpyDeviceToHost));
  return RTX_OK;
}
