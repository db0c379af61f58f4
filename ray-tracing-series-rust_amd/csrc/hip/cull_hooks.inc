// Device test hooks of the f32 culling code (rtx_device_cull_verdicts, rtx_device_walk_steps; included by render.hip, namespace
// rtx, in both compilations).  Kernels of their own: no render kernel includes from this file, and the functions under test
// (core/cull32.hpp, trace_vote.inc) are called exactly as the trace kernels call them.

// One item per thread: the box (already narrowed outward by the host), the ray in f64.  Builds the Ray32 as a bounce does and
// asks every form of the box test; the plane picks are the kernels' (ray32_dir_neg, wide_sign_pack).
__global__ void k_cull_verdicts(long long n, const float* __restrict__ box32, const double* __restrict__ ray, float* __restrict__ ray32,
                                float* __restrict__ key, uint32_t* __restrict__ verdict) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const float* lo = box32 + 6 * k;
  const float* hi = lo + 3;
  const double* in = ray + 8 * k;
  const rt::Ray r = rt::make_ray(rt::v3((rt::real)in[0], (rt::real)in[1], (rt::real)in[2]), rt::v3((rt::real)in[3], (rt::real)in[4], (rt::real)in[5]), rt::real(0));
  const rt::real t_min = (rt::real)in[6];
  const rt::Ray32 q = rt::make_ray32(r, t_min);
  const float t_max32 = rt::cull_round_up((rt::real)in[7]);
  const uint32_t neg = rt::ray32_dir_neg(q), pack = wide_sign_pack(r);
  uint32_t v = 0;
  if (rt::cull32_may_hit(lo, hi, q, t_max32)) v |= 1u;
  const float nx = (neg & 1u) ? hi[0] : lo[0], fx = (neg & 1u) ? lo[0] : hi[0];
  const float ny = (neg & 2u) ? hi[1] : lo[1], fy = (neg & 2u) ? lo[1] : hi[1];
  const float nz = (neg & 4u) ? hi[2] : lo[2], fz = (neg & 4u) ? lo[2] : hi[2];
  if (rt::cull32_may_hit_nf(nx, fx, ny, fy, nz, fz, q, t_max32)) v |= 2u;
  if (t_min > rt::real(0)) {
    v |= 64u;  // the positive-t_min form applies
    if (rt::cull32_may_hit_nf_pos(nx, fx, ny, fy, nz, fz, q, t_max32)) v |= 4u;
  }
  bool h0, h1;
  rt::cull32_may_hit2(lo, hi, lo, hi, q, t_max32, &h0, &h1);
  if (h0) v |= 8u;
  if (h1) v |= 16u;
  // the wide step's picks: byte offsets of the near planes inside a FlatNode4 (lo at 0 / 16 / 32, hi at 48 / 64 / 80)
  const uint32_t ox = pack & 0xffu, oy = (pack >> 8) & 0xffu, oz = pack >> 16;
  float t_near;
  if (slab_interval_nf(ox == 48u ? hi[0] : lo[0], ox == 48u ? lo[0] : hi[0], oy == 64u ? hi[1] : lo[1], oy == 64u ? lo[1] : hi[1],
                       oz == 80u ? hi[2] : lo[2], oz == 80u ? lo[2] : hi[2], q, t_max32, &t_near)) v |= 32u;
  const float qq[8] = {q.ix, q.iy, q.iz, q.oix, q.oiy, q.oiz, q.err2, q.t_min};
  for (int a = 0; a < 8; ++a) ray32[8 * k + a] = qq[a];
  key[k] = t_near;
  verdict[k] = v;
}

// Slots above `levels` that every lane's column has: a step stores into slot n + 3 at the most and the host admits n <= levels,
// so no store can leave the allocation whatever the records say.  They hold HOOK_CANARY; the caller checks them.
#define HOOK_GUARD_SLOTS 4
#define HOOK_CANARY 0x5ca1ab1e
#define HOOK_UNWRITTEN 0x0badf00d
// One step per thread on a TRACE_BLOCK-thread block, the stack in LDS as in the trace kernels.  KIND 0: walk_node_step32 on
// FlatNode32 records, 1: walk_node_step4 on FlatNode4 records.
template <int KIND, class STACK>
__global__ __launch_bounds__(TRACE_BLOCK) void k_walk_steps(const void* __restrict__ nodes, uint32_t levels, long long n,
                                                            const RtxWalkStepItem* __restrict__ items, int32_t* __restrict__ out) {
  extern __shared__ int32_t hook_stack[];
  const long long g = (long long)blockIdx.x * TRACE_BLOCK + threadIdx.x;
  if (g >= n) return;
  const RtxWalkStepItem it = items[g];
  STACK stack;
  stack.base = hook_stack + threadIdx.x;
  for (uint32_t l = 0; l < levels + HOOK_GUARD_SLOTS; ++l) stack.base[l * TRACE_BLOCK] = l < levels ? HOOK_UNWRITTEN : HOOK_CANARY;
  stack.reset();
  for (int32_t k = 0; k < it.n_stack; ++k) stack.push(k + 4 < it.n_stack ? (0x40000000 | k) : it.stack[k - (it.n_stack > 4 ? it.n_stack - 4 : 0)]);
  const rt::Ray32 q = {it.q[0], it.q[1], it.q[2], it.q[3], it.q[4], it.q[5], it.q[6], it.q[7]};
  const rt::Ray r = rt::make_ray(rt::v3(0, 0, 0), rt::v3((rt::real)it.dir[0], (rt::real)it.dir[1], (rt::real)it.dir[2]), rt::real(0));
  const uint32_t pick = KIND ? wide_sign_pack(r) : rt::ray_dir_neg(r);
  int32_t cur = it.node;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) {
      if (it.second_node < 0) break;
      stack.reset();  // a new walk on the same lane
      cur = it.second_node;
    }
    if (KIND) walk_node_step4((const FlatNode4*)nodes, q, pick, it.t_max32, &cur, stack);
    else walk_node_step32(((const rt::FlatNode32*)nodes)[cur], q, pick, it.t_max32, &cur, stack);
  }
  int32_t* o = out + g * (long long)(2 + levels + HOOK_GUARD_SLOTS);
  o[0] = cur;
  o[1] = stack.n;
  for (uint32_t l = 0; l < levels + HOOK_GUARD_SLOTS; ++l) o[2 + l] = stack.base[l * TRACE_BLOCK];
}

static rtx_status cull_verdicts_impl(int64_t n, const double* box, const double* ray, float* ray32, float* key, uint32_t* verdict) {
  if (n < 0 || n > 65536 || (n > 0 && (!box || !ray || !ray32 || !key || !verdict))) {
    set_error("rtx_device_cull_verdicts: NULL argument, or n outside [0, 65536]");
    return RTX_EINVAL;
  }
  if (n == 0) return RTX_OK;
  // the product's outward rounding (flatten.cpp: nodes32; wide_tree.hpp)
  std::vector<float> b32(6 * (size_t)n);
  for (int64_t k = 0; k < n; ++k)
    for (int a = 0; a < 3; ++a) {
      const double blo = box[6 * k + a], bhi = box[6 * k + 3 + a];
      float lo = (float)blo;
      if ((double)lo > blo) lo = std::nextafterf(lo, -INFINITY);
      float hi = (float)bhi;
      if ((double)hi < bhi) hi = std::nextafterf(hi, INFINITY);
      b32[6 * k + a] = lo; b32[6 * k + 3 + a] = hi;
    }
  DeviceBuffer<float> d_box, d_q, d_key;
  DeviceBuffer<double> d_ray;
  DeviceBuffer<uint32_t> d_v;
  HIP_TRY(d_box.upload(b32.data(), b32.size()));
  HIP_TRY(d_ray.upload(ray, 8 * (size_t)n));
  HIP_TRY(d_q.alloc(8 * (size_t)n * sizeof(float)));
  HIP_TRY(d_key.alloc((size_t)n * sizeof(float)));
  HIP_TRY(d_v.alloc((size_t)n * sizeof(uint32_t)));
  hipLaunchKernelGGL(k_cull_verdicts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (long long)n, d_box, d_ray, d_q, d_key, d_v);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(ray32, d_q, 8 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(key, d_key, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(verdict, d_v, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return RTX_OK;
}

static rtx_status walk_steps_impl(int32_t kind, int32_t bottom, const void* nodes, int64_t n_nodes, int32_t levels, int64_t n,
                                  const RtxWalkStepItem* items, int32_t* out) {
  const size_t lds = ((size_t)levels + HOOK_GUARD_SLOTS) * TRACE_BLOCK * sizeof(int32_t);
  if ((kind != 0 && kind != 1) || (bottom != 0 && bottom != 1) || !nodes || n_nodes <= 0 || n_nodes > (1 << 24) || levels < 1 ||
      lds > 64 * 1024 || n < 0 || n > 65536 || (n > 0 && (!items || !out))) {
    set_error("rtx_device_walk_steps: bad argument (kind and bottom are 0 / 1, 1 <= levels <= 60, n <= 65536)");
    return RTX_EINVAL;
  }
  for (int64_t k = 0; k < n; ++k) {
    const RtxWalkStepItem& it = items[k];
    // every index the kernel forms from an item is inside what it was given: the records, and the lane's stack column
    if (it.node < 0 || it.node >= n_nodes || it.second_node >= n_nodes || it.n_stack < 0 || it.n_stack + bottom > levels) {
      set_error("rtx_device_walk_steps: item " + std::to_string(k) + ": node outside the records, or more stack entries than levels");
      return RTX_EINVAL;
    }
  }
  if (n == 0) return RTX_OK;
  const size_t rec = kind ? sizeof(FlatNode4) : sizeof(rt::FlatNode32);
  const size_t per = 2 + (size_t)levels + HOOK_GUARD_SLOTS;
  DeviceBuffer<unsigned char> d_nodes;
  DeviceBuffer<RtxWalkStepItem> d_items;
  DeviceBuffer<int32_t> d_out;
  HIP_TRY(d_nodes.upload((const unsigned char*)nodes, (size_t)n_nodes * rec));
  HIP_TRY(d_items.upload(items, (size_t)n));
  HIP_TRY(d_out.alloc((size_t)n * per * sizeof(int32_t)));
  const dim3 grid((unsigned)((n + TRACE_BLOCK - 1) / TRACE_BLOCK)), block(TRACE_BLOCK);
  const void* dn = (const unsigned char*)d_nodes;
  if (kind && bottom) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_walk_steps<1, LdsStackB>), grid, block, lds, 0, dn, (uint32_t)levels, (long long)n, d_items, d_out);
  else if (kind) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_walk_steps<1, LdsStack>), grid, block, lds, 0, dn, (uint32_t)levels, (long long)n, d_items, d_out);
  else if (bottom) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_walk_steps<0, LdsStackB>), grid, block, lds, 0, dn, (uint32_t)levels, (long long)n, d_items, d_out);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_walk_steps<0, LdsStack>), grid, block, lds, 0, dn, (uint32_t)levels, (long long)n, d_items, d_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, d_out, (size_t)n * per * sizeof(int32_t), hipMemcpyDeviceToHost));
  return RTX_OK;
}
