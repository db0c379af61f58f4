// rtx_scene_set_spheres / rtx_scene_set_spheres_device on a resident f64 scene (included by render.hip after mesh_update.inc,
// namespace rtx; the f64 compilation only, like mesh_update.inc: a refit starts from the f64 records of the untouched
// primitives in a touched leaf).
//
// A new centre and radius for named static spheres reach these device arrays and no other:
//   spheres                         cx cy cz radius of the record; mat stays (k_set_spheres)
//   nodes / nodes32 / motion32      every BVH that holds an updated sphere, refitted whole (mesh_update.inc: k_refit_bvh)
//   nodes4                          the planes of those BVHs' wide records (k_refit_wide)
//   d_local_box, then the instance tree above a touched member (k_member_local_boxes, k_refit_instance_tree)
//   top_box32 / WorldDesc           a plain top-level sphere slot: both boxes; the boundary sphere of a medium: the record's box;
//                                   either: the record's "box is finite" and "same sphere as the medium behind me" flags
//                                   (k_sphere_slot_boxes, with core/prim_box.hpp's two rules)
//   the light table                 when an updated sphere is a sampled light: its area, and every light's cdf and pmf
//                                   (k_refresh_lights, with host/light_table.hpp's weight rule and cdf pass)
// so that the arrays equal those of the host-updated flat scene uploaded afresh -- the judge of tests/test_gpu_set_spheres.py.
// k_trace_lds copies nodes32 and the sphere records into LDS at the start of every launch and keeps no packed copy from the
// upload, so it needs nothing more.  Topology, SceneView, the trace kernels and every launch plan stay as they are.
//
// No index is derived from a value.  Every index a kernel forms comes from a table the host built from the caller's ids and
// the upload's shadow, both checked against the array sizes (host/set_spheres.hpp); a value is only ever stored, added or
// compared.  The kernels here need no visibility beyond kernel boundaries: each thread writes what only it owns (the climb of
// a refit states its own, once, in scene_update.inc).

// One thread per (flat sphere, value quadruple): pairs[2 i] = flat index, pairs[2 i + 1] = index of the quadruple in `values`.
__global__ __launch_bounds__(256) void k_set_spheres(const int32_t* __restrict__ pairs, int n_pairs, const double* __restrict__ values,
                                                    rt::FlatSphere* __restrict__ spheres) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n_pairs) return;
  double v[4];
  const double* src = values + 4 * (size_t)pairs[2 * (size_t)i + 1];
  for (int k = 0; k < 4; ++k) v[k] = src[k];
  rt::set_sphere_values(&spheres[pairs[2 * (size_t)i]], v);
}

// One thread per listed slot: slots[2 i] = the slot, slots[2 i + 1] = 0 a plain static sphere, 1 a medium bounded by one.
// top_box32 (plain only) and the box, the WD_BOXED_PRIM and the WD_PAIR flag of the slot's WorldDesc record, as the flattener
// and build_world_desc derive them.  A thread writes its own slot's record only; of the next slot's it reads what no update
// changes (flags other than WD_BOXED_PRIM, g_a).
__global__ __launch_bounds__(256) void k_sphere_slot_boxes(const int32_t* __restrict__ slots, int n, int n_top, const rt::FlatEntry* __restrict__ entries,
                                                          const int32_t* __restrict__ top_level, const rt::FlatSphere* __restrict__ spheres,
                                                          float* __restrict__ top_box32, WorldDesc* __restrict__ desc) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  const int32_t slot = slots[2 * (size_t)i];
  const bool medium = slots[2 * (size_t)i + 1] != 0;
  const rt::FlatEntry E = entries[top_level[slot]];
  const rt::PrimRef ref = (rt::PrimRef)(medium ? entries[E.a].a : E.a);
  float bx[6];
  bool finite = true;
  if (medium) finite = rt::medium_sphere_box32(spheres[rt::primref_index(ref)], bx);
  else {
    rt::plain_slot_box32(ref, spheres, nullptr, nullptr, bx);
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
__global__ __launch_bounds__(256) void k_refresh_lights(rt::SceneView sv, rt::FlatLight* __restrict__ lights, int32_t n_lights, double* __restrict__ weight) {
  for (int32_t k = (int32_t)threadIdx.x; k < n_lights; k += 256) {
    rt::Point3 centre;
    const rt::real area = rt::light_area_centre(lights[k], sv.spheres, sv.rects, &centre);
    if (lights[k].kind == rt::LIGHT_SPHERE) lights[k].area = area;
    weight[k] = rt::light_pick_weight(sv, lights[k].mat, area, centre);
  }
  __syncthreads();
  if (threadIdx.x == 0) rt::light_cdf_pass(lights, weight, n_lights);
}

// ------------------------------------------------------------------ host side
// ids (host memory) have passed check_sphere_ids against ds->mesh.shadow.  values: host memory (staged here, one copy) when
// host_values, else a device pointer.  Everything that can refuse comes first; then one copy and the launches, all on `stream`.
static rtx_status scene_set_spheres_impl(DeviceScene* ds, const char* who, const int32_t* ids, int64_t n, const double* values, bool host_values,
                                         hipStream_t stream) {
  MeshUpdate& mu = ds->mesh;
  const MeshShadow& sh = mu.shadow;
  std::string err;
  SpherePlan plan;
  const rtx_status pst = plan_sphere_update(who, sh, ids, n, &plan, &err);
  if (pst != RTX_OK) { set_error(err); return pst; }
  const rtx_status dst = check_scene_device(ds, who, "was uploaded to");
  if (dst != RTX_OK) return dst;
  rtx_status st = upload_mesh_tables(ds);
  if (st != RTX_OK) return st;
  bool lights = false;
  for (int64_t i = 0; i < n; ++i) lights = lights || ((size_t)ids[i] < mu.sphere_is_light.size() && mu.sphere_is_light[(size_t)ids[i]]);
  if (lights && !mu.d_light_weight) HIP_TRY(mu.d_light_weight.alloc((size_t)ds->lights.n_lights * sizeof(double)));
  // staging layout: [values, 32 B each (host entry only)] [pairs] [members: index, entry] [slots: slot, kind]
  const size_t value_bytes = host_values ? (size_t)n * 4 * sizeof(double) : 0;
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
  hipLaunchKernelGGL(k_set_spheres, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, stream, d_pairs, (int)n_pairs, d_values,
                     (rt::FlatSphere*)ds->view.spheres);
  HIP_TRY(hipGetLastError());
  if ((st = launch_bvh_refits(ds, plan.bvhs, stream)) != RTX_OK) return st;
  if ((st = launch_member_refits(ds, d_members, n_members, plan.trees, stream)) != RTX_OK) return st;
  if (n_slots) {
    hipLaunchKernelGGL(k_sphere_slot_boxes, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, stream, d_slots, (int)n_slots, ds->view.n_top_level,
                       ds->view.entries, ds->view.top_level, ds->view.spheres, (float*)ds->view.top_box32, (WorldDesc*)ds->world.desc);
    HIP_TRY(hipGetLastError());
  }
  if (lights) {
    hipLaunchKernelGGL(k_refresh_lights, dim3(1), dim3(256), 0, stream, ds->view, (rt::FlatLight*)ds->lights.lights, ds->lights.n_lights,
                       (double*)mu.d_light_weight);
    HIP_TRY(hipGetLastError());
  }
  return RTX_OK;
}
