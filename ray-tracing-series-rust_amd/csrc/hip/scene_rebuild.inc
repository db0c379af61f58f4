// rtx_scene_rebuild_instance_trees and rtx_scene_instance_tree_cost on a resident scene (included by render.hip behind
// scene_update.inc, namespace rtx; compiled by both compilations).
//
// A refit (scene_update.inc) keeps the topology the flattener chose for the first pose; once members have travelled far its
// boxes overlap and cull badly.  A rebuild gives tree k a new topology from the members' world boxes at the ops NOW in
// `entries`, in place: the same n_slots member slots, the same piece of n_slots - 1 nodes.  For one tree of m members, all on
// the caller's stream:
//   k_member_boxes     one thread per member: its world box in f64 (member_world_box, what k_refit_instance_tree starts from),
//                      the block-reduced bounds of the centroids
//   k_member_morton    63-bit Morton codes (core/karras.hpp: lbvh.hip's arithmetic), then a stable radix sort (rocPRIM, through
//                      lbvh.hip's rtx_sort_pairs_u64_u32 so that this file pulls no sort templates into render.hip)
//   k_rebuild_radix    Karras' tree, one thread per internal node; internal node 0 is the root = node node_base
//   k_rebuild_emit     one thread per member: depth of its leaf, then it writes its box into its parent's child box and climbs
//                      with k_refit's visibility recipe (stated at scene_update.inc's refit_climb; this climb exchanges f64 boxes
//                      through box64 and keeps its own loop); the second thread at a node unites the two f64 boxes, chooses the
//                      split axis and goes on.  The narrowed planes go through store_child_planes32.  Everything goes into a SCRATCH piece (FlatNode / FlatNode32 / FlatMotion32 and
//                      the two parent tables), so that a tree too deep for the launchers' stacks is refused with the resident
//                      tree untouched.
// The host then reads the depths (and the new parent tables) in ONE wait on the stream, checks the stack budget and commits
// with device-to-device copies.  Topology comes from the f64 boxes in both compilations, so an f64 and an f32 scene get the
// same tree; the host twin is host/rebuild_instances.hpp: RTX_REBUILD_MORTON.

__device__ __forceinline__ double rebuild_atomic_min_f64(double* addr, double val) {
  unsigned long long* a = (unsigned long long*)addr;
  unsigned long long old = *a;
  while (__longlong_as_double((long long)old) > val) {
    const unsigned long long assumed = old;
    old = atomicCAS(a, assumed, (unsigned long long)__double_as_longlong(val));
    if (old == assumed) break;
  }
  return __longlong_as_double((long long)old);
}
__device__ __forceinline__ double rebuild_atomic_max_f64(double* addr, double val) {
  unsigned long long* a = (unsigned long long*)addr;
  unsigned long long old = *a;
  while (__longlong_as_double((long long)old) < val) {
    const unsigned long long assumed = old;
    old = atomicCAS(a, assumed, (unsigned long long)__double_as_longlong(val));
    if (old == assumed) break;
  }
  return __longlong_as_double((long long)old);
}

// bounds = +inf x 3, -inf x 3; *depth = 0 (one tree's, in stream order before k_member_boxes)
__global__ void k_rebuild_init(double* bounds, int32_t* depth) {
  if (threadIdx.x < 3) bounds[threadIdx.x] = __builtin_huge_val();
  else if (threadIdx.x < 6) bounds[threadIdx.x] = -__builtin_huge_val();
  else if (threadIdx.x == 6) *depth = 0;
}

struct MemberBoxArgs {
  const rt::FlatEntry* entries;
  const int32_t* top_level;
  const double* local_box;            // 6 per member, this tree's first member first
  const rt::XformOp64* slot_ops64;    // the f32 compilation's f64 ops; NULL in the f64 compilation
  double* boxes;                      // out: 6 per member
  double* bounds;                     // out: min xyz, max xyz of the centroids
  int32_t first_slot, n_slots;
};

// One thread per member: its world box at the ops now in `entries` (core/member_box.hpp: member_world_box), in f64.  Every
// thread of the block takes part in the reduction.
__global__ __launch_bounds__(256) void k_member_boxes(MemberBoxArgs a) {
  __shared__ double red[6][256];
  const int m = (int)(blockIdx.x * 256u + threadIdx.x);
  const bool valid = m < a.n_slots;
  double c[3] = {0.0, 0.0, 0.0};
  if (valid) {
    const int32_t slot = a.first_slot + m;
    double b[6];
    rt::member_world_box(a.entries[a.top_level[slot]], slot, a.slot_ops64, a.local_box + 6 * (size_t)m, b);
    for (int x = 0; x < 6; ++x) a.boxes[6 * (size_t)m + x] = b[x];
    for (int x = 0; x < 3; ++x) c[x] = 0.5 * (b[x] + b[3 + x]);
  }
  for (int x = 0; x < 3; ++x) {
    red[x][threadIdx.x] = valid ? c[x] : __builtin_huge_val();
    red[3 + x][threadIdx.x] = valid ? c[x] : -__builtin_huge_val();
  }
  __syncthreads();
  for (uint32_t s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s)
      for (int x = 0; x < 3; ++x) {
        red[x][threadIdx.x] = fmin(red[x][threadIdx.x], red[x][threadIdx.x + s]);
        red[3 + x][threadIdx.x] = fmax(red[3 + x][threadIdx.x], red[3 + x][threadIdx.x + s]);
      }
    __syncthreads();
  }
  if (threadIdx.x < 3) rebuild_atomic_min_f64(&a.bounds[threadIdx.x], red[threadIdx.x][0]);
  else if (threadIdx.x < 6) rebuild_atomic_max_f64(&a.bounds[threadIdx.x], red[threadIdx.x][0]);
}

__global__ __launch_bounds__(256) void k_member_morton(const double* __restrict__ boxes, int m, const double* __restrict__ bounds,
                                                      unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= m) return;
  double bd[6];
  for (int x = 0; x < 6; ++x) bd[x] = bounds[x];
  keys[i] = rt::morton63(boxes + 6 * (size_t)i, bd);
  vals[i] = (uint32_t)i;
}

// children: 2 per internal node (>= 0 internal node, < 0: ~position in the sorted order); the root's parent is -1
__global__ __launch_bounds__(256) void k_rebuild_radix(const unsigned long long* __restrict__ keys, int m, int32_t* __restrict__ children,
                                                      int32_t* __restrict__ parent_of_node, int32_t* __restrict__ parent_of_leaf) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= m - 1) return;
  const rt::KarrasNode n = rt::karras_node(keys, m, i);
  children[2 * (size_t)i] = n.left;
  children[2 * (size_t)i + 1] = n.right;
  if (n.left >= 0) parent_of_node[n.left] = i; else parent_of_leaf[~n.left] = i;
  if (n.right >= 0) parent_of_node[n.right] = i; else parent_of_leaf[~n.right] = i;
  if (i == 0) parent_of_node[0] = -1;
}

struct RebuildEmitArgs {
  const double* boxes;                // 6 per member
  const uint32_t* order;              // sorted position -> member
  const int32_t* children;            // 2 per internal node
  const int32_t* parent_of_node;
  const int32_t* parent_of_leaf;
  double* box64;                      // scratch: 12 per node, the two child boxes in f64 (what the climbers exchange)
  rt::FlatNode* nodes;                // scratch pieces of m - 1 elements, indexed by internal node
  rt::FlatNode32* nodes32;
  rt::FlatMotion32* motion32;         // NULL: the scene has no time-aware boxes
  int32_t* leaf_parent;               // scratch: 2 per member (UpdateShadow's format: absolute node, child index)
  int32_t* node_parent;               // scratch: 2 per node (absolute parent or -1, child index or -1)
  unsigned int* arrivals;             // 1 per node, zero at launch
  int32_t* depth;                     // zero at launch: the deepest leaf, in nodes
  int32_t first_slot, n_slots, node_base;
};

// One thread per member, in sorted order.  A climber writes its box into child c of `node` -- the f64 planes with agent-scope
// stores, since the sibling's climber on another CU reads them; the FlatNode / FlatNode32 / FlatMotion32 fields plainly, each
// is written by one thread and read by nobody in this kernel -- then arrives.  The first of the two leaves; the second loads
// the sibling's f64 box, chooses the axis, unites and carries the union to the node's parent.  Unions are exact min / max.
__global__ __launch_bounds__(256) void k_rebuild_emit(RebuildEmitArgs a) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= a.n_slots) return;
  const uint32_t member = a.order[i];
  double b[6];
  for (int x = 0; x < 6; ++x) b[x] = a.boxes[6 * (size_t)member + x];
  int32_t node = a.parent_of_leaf[i];
  int d = 0;
  for (int32_t up = node; up >= 0; up = a.parent_of_node[up]) ++d;
  atomicMax(a.depth, d);
  int c = a.children[2 * (size_t)node] == ~i ? 0 : 1;
  a.leaf_parent[2 * (size_t)member] = a.node_base + node;
  a.leaf_parent[2 * (size_t)member + 1] = c;
  int32_t code = rt::make_leaf((uint32_t)a.first_slot + member, 1u);
  for (;;) {
    rt::FlatNode* nd = &a.nodes[node];
    for (int x = 0; x < 3; ++x) {
      __hip_atomic_store(&a.box64[12 * (size_t)node + 6 * c + x], b[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&a.box64[12 * (size_t)node + 6 * c + 3 + x], b[3 + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const rt::real lo = refit_plane_down(b[x]), hi = refit_plane_up(b[3 + x]);
      nd->bmin[c][x] = lo;
      nd->bmax[c][x] = hi;
      store_child_planes32(a.nodes32, a.motion32, node, c, x, lo, hi);
    }
    nd->child[c] = code;
    a.nodes32[node].child[c] = code;
    __threadfence();
    if (atomicAdd(&a.arrivals[node], 1u) == 0u) return;  // first of the two: the sibling's climber finishes the node
    __threadfence();
    double s[6];
    for (int x = 0; x < 6; ++x) s[x] = __hip_atomic_load(&a.box64[12 * (size_t)node + 6 * (1 - c) + x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int axis = c == 0 ? rt::karras_split_axis(b, s) : rt::karras_split_axis(s, b);
    nd->pad[0] = axis;
    nd->pad[1] = 0;
    a.nodes32[node].axis = axis;
    a.nodes32[node].pad = 0;
    for (int x = 0; x < 3; ++x) { b[x] = rt::rt_fmin(b[x], s[x]); b[3 + x] = rt::rt_fmax(b[3 + x], s[3 + x]); }
    const int32_t parent = a.parent_of_node[node];
    if (parent < 0) {  // the root: its two child boxes are the whole tree
      a.node_parent[2 * (size_t)node] = -1;
      a.node_parent[2 * (size_t)node + 1] = -1;
      return;
    }
    const int pc = a.children[2 * (size_t)parent] == node ? 0 : 1;
    a.node_parent[2 * (size_t)node] = a.node_base + parent;
    a.node_parent[2 * (size_t)node + 1] = pc;
    code = a.node_base + node;
    node = parent;
    c = pc;
  }
}

// The committed root, where the scans read it: the tree's ENTRY_INSTANCE record and its record behind k_trace_world's slots.
__global__ void k_set_tree_root(rt::FlatEntry* entries, int32_t entry, WorldDesc* desc, int32_t desc_index, int32_t root) {
  if (threadIdx.x == 0) { entries[entry].a = root; desc[desc_index].medium_mat = root; }
}

// term[i] = the areas of node node_base + i's two child boxes, added; term[n_nodes] = the area of the union of the root's two.
// Planes are widened to f64 first (an f32 scene's are floats).
__global__ __launch_bounds__(256) void k_tree_cost_terms(const rt::FlatNode* __restrict__ nodes, int32_t node_base, int32_t n_nodes, int32_t root,
                                                        double* __restrict__ term) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i > n_nodes) return;
  const rt::FlatNode* nd = &nodes[i < n_nodes ? node_base + i : root];
  double lo[2][3], hi[2][3];
  for (int c = 0; c < 2; ++c)
    for (int x = 0; x < 3; ++x) { lo[c][x] = (double)nd->bmin[c][x]; hi[c][x] = (double)nd->bmax[c][x]; }
  if (i < n_nodes) {
    term[i] = rt::box_surface_area(lo[0], hi[0]) + rt::box_surface_area(lo[1], hi[1]);
  } else {
    double ulo[3], uhi[3];
    for (int x = 0; x < 3; ++x) { ulo[x] = rt::rt_fmin(lo[0][x], lo[1][x]); uhi[x] = rt::rt_fmax(hi[0][x], hi[1][x]); }
    term[i] = rt::box_surface_area(ulo, uhi);
  }
}

// ------------------------------------------------------------------ host side
// The scratch of a rebuild, laid out like the shadow's per-member and per-node tables (tree k's piece starts at member_first /
// node_first), so several trees of one call are built side by side and committed after one readback.  Sized once: a scene's
// trees never change their member counts.
static rtx_status rebuild_scratch(DeviceScene* ds) {
  SceneUpdate& u = ds->upd;
  const size_t members = u.shadow.leaf_parent.size() / 2, nodes = u.shadow.node_parent.size() / 2, trees = u.shadow.trees.size();
  if (u.r_boxes) return RTX_OK;
  HIP_TRY(u.r_boxes.alloc(6 * members * sizeof(double)));
  HIP_TRY(u.r_bounds.alloc(6 * trees * sizeof(double)));
  HIP_TRY(u.r_keys.alloc(members * 8));
  HIP_TRY(u.r_keys_sorted.alloc(members * 8));
  HIP_TRY(u.r_vals.alloc(members * 4));
  HIP_TRY(u.r_vals_sorted.alloc(members * 4));
  HIP_TRY(u.r_children.alloc(2 * nodes * 4));
  HIP_TRY(u.r_parent_node.alloc(nodes * 4));
  HIP_TRY(u.r_parent_leaf.alloc(members * 4));
  HIP_TRY(u.r_box64.alloc(12 * nodes * sizeof(double)));
  HIP_TRY(u.r_nodes.alloc(nodes * sizeof(rt::FlatNode)));
  HIP_TRY(u.r_nodes32.alloc(nodes * sizeof(rt::FlatNode32)));
  if (ds->view.motion32) HIP_TRY(u.r_motion32.alloc(nodes * sizeof(rt::FlatMotion32)));
  HIP_TRY(u.r_leaf_parent.alloc(2 * members * 4));
  HIP_TRY(u.r_node_parent.alloc(2 * nodes * 4));
  HIP_TRY(u.r_depth.alloc(trees * 4));
  return RTX_OK;
}

static rtx_status scene_rebuild_impl(DeviceScene* ds, const int32_t* trees, int32_t n, hipStream_t stream, RtxRebuildStats* out) {
  const char* who = "rtx_scene_rebuild_instance_trees";
  SceneUpdate& u = ds->upd;
  std::string err;
  if (!u.shadow.broken.empty()) { set_error(std::string(who) + ": " + u.shadow.broken); return RTX_EINVAL; }
  std::vector<int32_t> list;
  if (!check_rebuild_list(who, ds, u.shadow.trees.size(), trees, n, &list, &err)) { set_error(err); return RTX_EINVAL; }
  rtx_status st = check_scene_device(ds, who, "was uploaded to");
  if (st != RTX_OK) return st;
  if (out) {
    out->trees_rebuilt = 0; out->max_depth = 0;
    out->max_stack_before = out->max_stack_after = ds->view.max_stack;
  }
  if (list.empty()) return RTX_OK;
  st = rebuild_scratch(ds);
  if (st != RTX_OK) return st;
  int m_max = 0;
  for (int32_t k : list) m_max = std::max(m_max, (int)u.shadow.trees[(size_t)k].n_slots);
  size_t temp_bytes = 0;
  HIP_TRY(rtx_sort_pairs_u64_u32(nullptr, &temp_bytes, u.r_keys, u.r_keys_sorted, u.r_vals, u.r_vals_sorted, m_max, stream));
  HIP_TRY(u.r_sort_temp.grow(temp_bytes ? temp_bytes : 1, stream));

  for (int32_t k : list) {
    const TreeShadow& t = u.shadow.trees[(size_t)k];
    const int m = t.n_slots;
    const size_t mf = (size_t)t.member_first, nf = (size_t)t.node_first;
    const unsigned gm = (unsigned)((m + 255) / 256);
    double* bounds = u.r_bounds + 6 * (size_t)k;
    int32_t* depth = u.r_depth + (size_t)k;
    HIP_TRY(hipMemsetAsync(u.d_arrivals + nf, 0, (size_t)t.n_nodes * sizeof(unsigned int), stream));
    hipLaunchKernelGGL(k_rebuild_init, dim3(1), dim3(64), 0, stream, bounds, depth);
    MemberBoxArgs mb;
    mb.entries = ds->view.entries; mb.top_level = ds->view.top_level;
    mb.local_box = u.d_local_box + 6 * mf;
    mb.slot_ops64 = u.d_slot_ops64;
    mb.boxes = u.r_boxes + 6 * mf; mb.bounds = bounds;
    mb.first_slot = t.first_slot; mb.n_slots = m;
    hipLaunchKernelGGL(k_member_boxes, dim3(gm), dim3(256), 0, stream, mb);
    hipLaunchKernelGGL(k_member_morton, dim3(gm), dim3(256), 0, stream, (const double*)mb.boxes, m, (const double*)bounds, u.r_keys + mf, u.r_vals + mf);
    HIP_TRY(hipGetLastError());
    size_t tb = u.r_sort_temp.bytes();
    HIP_TRY(rtx_sort_pairs_u64_u32(u.r_sort_temp, &tb, u.r_keys + mf, u.r_keys_sorted + mf, u.r_vals + mf, u.r_vals_sorted + mf, m, stream));
    hipLaunchKernelGGL(k_rebuild_radix, dim3(gm), dim3(256), 0, stream, (const unsigned long long*)(u.r_keys_sorted + mf), m, u.r_children + 2 * nf,
                       u.r_parent_node + nf, u.r_parent_leaf + mf);
    RebuildEmitArgs e;
    e.boxes = mb.boxes; e.order = u.r_vals_sorted + mf;
    e.children = u.r_children + 2 * nf; e.parent_of_node = u.r_parent_node + nf; e.parent_of_leaf = u.r_parent_leaf + mf;
    e.box64 = u.r_box64 + 12 * nf;
    e.nodes = u.r_nodes + nf; e.nodes32 = u.r_nodes32 + nf; e.motion32 = ds->view.motion32 ? u.r_motion32 + nf : nullptr;
    e.leaf_parent = u.r_leaf_parent + 2 * mf; e.node_parent = u.r_node_parent + 2 * nf;
    e.arrivals = u.d_arrivals + nf; e.depth = depth;
    e.first_slot = t.first_slot; e.n_slots = m; e.node_base = t.node_base;
    hipLaunchKernelGGL(k_rebuild_emit, dim3(gm), dim3(256), 0, stream, e);
    HIP_TRY(hipGetLastError());
  }

  // the one wait of the call: the new depths, and with them the new parent tables for the host's shadow
  std::vector<int32_t> h_depth(u.shadow.trees.size(), 0), h_leaf(u.shadow.leaf_parent.size()), h_node(u.shadow.node_parent.size());
  HIP_TRY(hipMemcpyAsync(h_depth.data(), u.r_depth, h_depth.size() * 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(h_leaf.data(), u.r_leaf_parent, h_leaf.size() * 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(h_node.data(), u.r_node_parent, h_node.size() * 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));

  std::vector<int32_t> tree_depth = u.tree_depth;
  int32_t deepest = 0;
  for (int32_t k : list) { tree_depth[(size_t)k] = h_depth[(size_t)k]; deepest = std::max(deepest, h_depth[(size_t)k]); }
  const int32_t max_stack = instance_max_stack(u.member_stack, tree_depth);
  if (stack_bytes((uint32_t)max_stack + 1u) > 64 * 1024) {
    set_error(std::string(who) + ": the rebuilt trees need a walk stack of " + std::to_string(max_stack + 1) + " levels, the launchers accept " +
              std::to_string(kMaxWalkStack + 1) + " (the scene is unchanged)");
    return RTX_EUNSUPPORTED;
  }

  for (int32_t k : list) {
    TreeShadow& t = u.shadow.trees[(size_t)k];
    const size_t mf = (size_t)t.member_first, nf = (size_t)t.node_first, nn = (size_t)t.n_nodes, nm = (size_t)t.n_slots;
    HIP_TRY(hipMemcpyAsync((rt::FlatNode*)ds->view.nodes + t.node_base, u.r_nodes + nf, nn * sizeof(rt::FlatNode), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync((rt::FlatNode32*)ds->view.nodes32 + t.node_base, u.r_nodes32 + nf, nn * sizeof(rt::FlatNode32), hipMemcpyDeviceToDevice, stream));
    if (ds->view.motion32)
      HIP_TRY(hipMemcpyAsync((rt::FlatMotion32*)ds->view.motion32 + t.node_base, u.r_motion32 + nf, nn * sizeof(rt::FlatMotion32), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(u.d_leaf_parent + 2 * mf, u.r_leaf_parent + 2 * mf, 2 * nm * 4, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(u.d_node_parent + 2 * nf, u.r_node_parent + 2 * nf, 2 * nn * 4, hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(k_set_tree_root, dim3(1), dim3(64), 0, stream, (rt::FlatEntry*)ds->view.entries, (int32_t)ds->view.inst_entries + k,
                       (WorldDesc*)ds->world.desc, ds->view.n_top_level + k, t.node_base);
    HIP_TRY(hipGetLastError());
    std::copy(h_leaf.begin() + 2 * mf, h_leaf.begin() + 2 * (mf + nm), u.shadow.leaf_parent.begin() + 2 * mf);
    std::copy(h_node.begin() + 2 * nf, h_node.begin() + 2 * (nf + nn), u.shadow.node_parent.begin() + 2 * nf);
    t.root = t.node_base;
  }
  u.tree_depth = tree_depth;
  // the stack budget: every launcher reads view.max_stack when it launches (render_impl, features_impl, launch_cast_rays,
  // trace_rays_impl); what was derived from it at upload and an instance world can reach is k_trace_world's plan
  const int32_t before = ds->view.max_stack;
  ds->view.max_stack = max_stack;
  if (max_stack != before) plan_world_stacks(ds);
  if (out) { out->trees_rebuilt = (int32_t)list.size(); out->max_depth = deepest; out->max_stack_before = before; out->max_stack_after = max_stack; }
  return RTX_OK;
}

// rtx_scene_instance_tree_cost: the per-node terms from a kernel, added here in index order (blocking).
static rtx_status scene_tree_cost_impl(DeviceScene* ds, int32_t k, double* cost) {
  const char* who = "rtx_scene_instance_tree_cost";
  SceneUpdate& u = ds->upd;
  if (!u.shadow.broken.empty()) { set_error(std::string(who) + ": " + u.shadow.broken); return RTX_EINVAL; }
  if (k < 0 || (size_t)k >= u.shadow.trees.size()) {
    set_error(std::string(who) + ": k is out of range (the scene has " + std::to_string(u.shadow.trees.size()) + " instance trees)");
    return RTX_EINVAL;
  }
  const rtx_status dst = check_scene_device(ds, who, "lives on");
  if (dst != RTX_OK) return dst;
  const TreeShadow& t = u.shadow.trees[(size_t)k];
  HIP_TRY(hipDeviceSynchronize());  // after everything enqueued on the device, like rtx_device_scene_array
  HIP_TRY(u.r_terms.grow(((size_t)t.n_nodes + 1) * sizeof(double), nullptr));
  hipLaunchKernelGGL(k_tree_cost_terms, dim3((unsigned)((t.n_nodes + 1 + 255) / 256)), dim3(256), 0, nullptr, (const rt::FlatNode*)ds->view.nodes,
                     t.node_base, t.n_nodes, t.root, (double*)u.r_terms);
  HIP_TRY(hipGetLastError());
  std::vector<double> term((size_t)t.n_nodes + 1);
  HIP_TRY(hipMemcpy(term.data(), u.r_terms, term.size() * sizeof(double), hipMemcpyDeviceToHost));
  *cost = instance_tree_cost_from_terms(term.data(), t.n_nodes, term[(size_t)t.n_nodes]);
  return RTX_OK;
}
