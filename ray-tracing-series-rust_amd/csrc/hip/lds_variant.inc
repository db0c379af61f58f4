// Which k_trace_lds a render launches, decided on the host from the scene's time intervals: the MovingSpheres' own
// (time0, time1), the interval of the BVH above them and the camera's shutter.  plan_lds and launch_lds (render.hip) take
// every such decision from here and report it in RtxRenderStats.trace_variant.  Included inside namespace rtx; host-compilable
// on its own (tests/lds_variant_host_check.cpp).

// bits of RtxRenderStats.trace_variant
enum : int32_t {
  LDSV_TIME_BOXES = 1,    // the time-aware boxes (MOTION bit 0 of k_trace_lds)
  LDSV_ONE_AXIS = 2,      // ... with slopes along y only (MOTION bit 1)
  LDSV_COMMON_RATIO = 4,  // one (time - mv_t0) / (mv_t1 - mv_t0) per bounce for every primitive record
};

// One ratio per bounce serves every record when all MovingSpheres share one interval -- and that interval is not empty:
// static spheres ride along as movers with c1 = c0, and with time0 == time1 the shared ratio is x / 0, its product with
// their c1 - c0 = 0 a NaN, so every STATIC sphere of the scene would take a NaN centre (Sphere::hit never reads the time).
// Records of such a scene are tested with their own intervals instead (a static sphere's is (0, 1)).
// MS: any record with time0 and time1.
template <class MS>
inline bool lds_common_interval(const MS* ms, size_t n, double* t0, double* t1) {
  if (n == 0 || (double)ms[0].time0 == (double)ms[0].time1) return false;
  for (size_t k = 1; k < n; ++k)
    if (ms[k].time0 != ms[0].time0 || ms[k].time1 != ms[0].time1) return false;
  *t0 = (double)ms[0].time0;
  *t1 = (double)ms[0].time1;
  return true;
}

// Which primitive record k_trace_lds keeps in LDS.  static_preset: the feature mask of the lean instantiation
// (P_STATIC_SPHERES: static spheres, no checker).  A world with any feature beyond it -- moving spheres, or static spheres
// under a checker texture -- runs k_trace_lds<P_SPHERES>, which keeps EVERY sphere as an 80-byte moving-sphere record
// (trace_lds.inc: UNI).  plan_lds sizes the LDS and launch_lds picks the instantiation from this one answer: asked of the
// scene's primitives instead, a static world with a checker got room for 40-byte sphere records under a kernel that writes
// moving-sphere records.
inline bool lds_records_are_moving(uint32_t features, uint32_t static_preset) { return (features & ~static_preset) != 0u; }
// The record counts of the plan for a BVH of max_end leaf slots over n_static static spheres: {n_spheres, n_moving, n_uni}.
inline void lds_record_counts(uint32_t features, uint32_t static_preset, uint32_t n_static, uint32_t max_end, uint32_t out[3]) {
  const bool moving = lds_records_are_moving(features, static_preset);
  out[0] = moving ? 0u : max_end;
  out[1] = moving ? max_end : 0u;
  out[2] = moving ? n_static : 0u;
}

#ifdef LDSK_DONE  // (wants ldsk_item: lds_layout.inc first, as in render.hip and tests/lds_entry_host_check.cpp)
// Where a walk of k_trace_lds enters the tree: out[0] is the first work item, out[1] the item under it on the stack, or
// LDSK_DONE for "nothing".  A root that is a leaf-first node (split "axis" 3: child 0, a leaf, is visited first whatever the
// ray's direction -- bvh_build.cpp) leaves the same state behind for every ray that may hit both children: the leaf in hand,
// child 1 stacked.  A walk that STARTS in that state skips the root step; a ray whose root step would have culled a child
// meets that cull one step later (the leaf's own exact test, the children of child 1), and for a ray that is finite in every
// component culling never decides a result (core/cull32.hpp; the kernel sends the others through the root).  The stack is no
// deeper than after the root step, so its levels stay what the tree's height asks for.
// Any other root is entered as before: {root, LDSK_DONE}.
// N: any node record with child[2] and axis (FlatNode32).
// Host and device: the kernel asks it of the tree it is about to copy (trace_lds.inc), a test asks it on the host.
template <class N>
__host__ __device__ inline void lds_entry_pair(const N* nodes, int32_t root, int32_t out[2]) {
  const int32_t axis = nodes[root].axis, c0 = nodes[root].child[0], c1 = nodes[root].child[1];
  if (axis == 3 && c0 < 0) {
    out[0] = ldsk_item(c0);
    out[1] = c1 >= 0 ? (c1 | (nodes[c1].axis << 13)) : ldsk_item(c1);
  } else {
    out[0] = root | (axis << 13);
    out[1] = LDSK_DONE;
  }
}
#endif

// A BVH's interval admits time-aware boxes when it is ordered: the boxes are lerps between its two ends (flatten.cpp).
inline bool lds_motion_interval_ok(double bvh_t0, double bvh_t1) { return bvh_t0 < bvh_t1; }

// The variant of one render.  time_boxes: the scene has a time-aware instantiation that fits (LdsPlan::motion.ok) over
// [bvh_t0, bvh_t1]; it is taken when every ray time of the render, [shutter1, shutter2) (camera.rs:69), lies inside that interval --
// outside it a lerped box is no bound.  motion_axis: LdsPlan::motion_axis.
inline int32_t lds_trace_variant(bool time_boxes, double bvh_t0, double bvh_t1, double shutter1, double shutter2, int motion_axis,
                                 bool mv_common) {
  const bool motion = time_boxes && lds_motion_interval_ok(bvh_t0, bvh_t1) && shutter1 >= bvh_t0 && shutter2 <= bvh_t1;
  return (motion ? LDSV_TIME_BOXES : 0) | (motion && motion_axis == 1 ? LDSV_ONE_AXIS : 0) | (mv_common ? LDSV_COMMON_RATIO : 0);
}
