// One process, several GPUs: rtx_multi_* (included by render.hip after render_impl).
//
// Replaces the reference's band threads + mpsc collect loop (world.rs:1198-1244) at node scale.  The image is cut into
// row-interleaved shards (RtxShard: rows j with (j / block_rows) % n == r -- sky and ground rows alternate, so shards
// cost the same, unlike the reference's contiguous bands), every device holds the whole scene (<= 0.25 GB) and renders its
// shard into its own HBM on its own stream, then ONE ncclGather (RCCL) brings the tone-mapped shards (and the f64
// accumulators, when asked for) to device 0, a kernel puts the rows where they belong and one copy hands the frame
// to the host.  Over xGMI every peer owns a direct link to the root, so the gather is one hop (C5: 24.9 MB of RGB8 in all).
// Streams are keyed by the global pixel index: the frame is byte-identical for every shard count and device set.
//
// RCCL is bound at run time (dlopen): the library keeps loading on hosts without it, and a process that has torch's
// bundled librccl.so mapped already shares that copy instead of pulling in a second one.
#include <dlfcn.h>

namespace rtx {

typedef void* nccl_comm_t;
struct RcclApi {
  void* handle = nullptr;
  int (*CommInitAll)(nccl_comm_t*, int, const int*) = nullptr;
  int (*CommDestroy)(nccl_comm_t) = nullptr;
  int (*CommCount)(nccl_comm_t, int*) = nullptr;  // optional: what the communicator itself says its size is
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Gather)(const void*, void*, size_t, int, int, nccl_comm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok() const { return CommInitAll && CommDestroy && GroupStart && GroupEnd && Gather && GetErrorString; }
};
static RcclApi load_rccl() {
  RcclApi api;
  for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
    api.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (api.handle) break;
  }
  if (!api.handle) return api;
  api.CommInitAll = (int (*)(nccl_comm_t*, int, const int*))dlsym(api.handle, "ncclCommInitAll");
  api.CommDestroy = (int (*)(nccl_comm_t))dlsym(api.handle, "ncclCommDestroy");
  api.CommCount = (int (*)(nccl_comm_t, int*))dlsym(api.handle, "ncclCommCount");
  api.GroupStart = (int (*)())dlsym(api.handle, "ncclGroupStart");
  api.GroupEnd = (int (*)())dlsym(api.handle, "ncclGroupEnd");
  api.Gather = (int (*)(const void*, void*, size_t, int, int, nccl_comm_t, hipStream_t))dlsym(api.handle, "ncclGather");
  api.GetErrorString = (const char* (*)(int))dlsym(api.handle, "ncclGetErrorString");
  return api;
}
// The table is filled exactly once, by whichever thread comes first (function-local static: C++11 guarantees the others wait):
// an rtx_flat may be shared between threads that each create their own rtx_multi.
static RcclApi* rccl_api() {
  static RcclApi api = load_rccl();
  return api.ok() ? &api : nullptr;
}
#define NCCL_UINT8 1  /* ncclUint8, rccl.h */

// gathered[r][lr][i][c] (shards padded to max_rows rows) -> image[j][i][c]
template <class T>
__global__ __launch_bounds__(256) void k_untile_rows(const T* __restrict__ gathered, T* __restrict__ image, uint32_t width,
                                                     uint32_t height, uint32_t n_shards, uint32_t block_rows, uint32_t max_rows) {
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;  // element of the image
  const uint64_t row_elems = (uint64_t)width * 3u;
  if (k >= (uint64_t)height * row_elems) return;
  const uint32_t j = (uint32_t)(k / row_elems);
  const uint64_t within = k - (uint64_t)j * row_elems;
  const uint32_t blk = j / block_rows;
  const uint32_t r = blk % n_shards;
  const uint32_t lr = (blk / n_shards) * block_rows + (j - blk * block_rows);
  image[k] = gathered[((uint64_t)r * max_rows + lr) * row_elems + within];
}

struct MultiDevice {
  int device = 0;
  rtx_scene* scene = nullptr;
  hipStream_t stream = nullptr;
  DeviceBuffer<uint8_t> d_rgb8;  // this shard's tone-mapped rows (max_rows x w x 3)
  DeviceBuffer<double> d_accum;  // this shard's accumulators, when the caller wants them
  nccl_comm_t comm = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

}  // namespace rtx

struct rtx_multi {
  std::vector<rtx::MultiDevice> dev;   // one per distinct device (same-device rehearsal: one entry)
  int n_shards = 1, block_rows = 1;
  bool same_device = false, use_rccl = false;
  int rccl_ranks = 0;                  // ncclCommCount of the communicator (0: no communicator, or the symbol is missing)
  DeviceBuffer<uint8_t> d_gather8, d_image8;   // on dev[0]
  DeviceBuffer<double> d_gather64, d_image64;  // on dev[0]
  hipEvent_t ev_gather0 = nullptr, ev_gather1 = nullptr;  // on dev[0]: around gather + un-tiling
};

namespace rtx {

static void multi_free(rtx_multi* m) {
  if (!m) return;
  RcclApi* api = rccl_api();
  // nothing may still be running on a stream when its communicator, buffers or scene go away
  for (MultiDevice& d : m->dev)
    if (d.stream && hipSetDevice(d.device) == hipSuccess) (void)hipStreamSynchronize(d.stream);
  for (MultiDevice& d : m->dev) {
    (void)hipSetDevice(d.device);
    if (d.comm && api) (void)api->CommDestroy(d.comm);
    if (d.scene) rtx_scene_destroy(d.scene);
    (void)d.d_rgb8.release();  // with its device current
    (void)d.d_accum.release();
    if (d.ev0) (void)hipEventDestroy(d.ev0);
    if (d.ev1) (void)hipEventDestroy(d.ev1);
    if (d.stream) (void)hipStreamDestroy(d.stream);
  }
  if (!m->dev.empty()) (void)hipSetDevice(m->dev[0].device);
  if (m->ev_gather0) (void)hipEventDestroy(m->ev_gather0);
  if (m->ev_gather1) (void)hipEventDestroy(m->ev_gather1);
  delete m;  // the gather and image buffers, with dev[0] current
}

}  // namespace rtx

static rtx_status multi_create(const rtx_flat* f, int32_t n_shards, const int32_t* device_ids, int32_t block_rows, bool f32,
                               rtx_multi** out) {
  using namespace rtx;
  if (!f || !out || n_shards <= 0 || n_shards > 64 || block_rows <= 0) { set_error("rtx_multi_create: bad argument"); return RTX_EINVAL; }
  *out = nullptr;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { set_error("rtx_multi_create: no GPU (this library has no CPU render path)"); return RTX_EHIP; }
  std::vector<int> ids((size_t)n_shards);
  for (int r = 0; r < n_shards; ++r) ids[r] = device_ids ? device_ids[r] : r;
  bool all_same = true, all_distinct = true;
  for (int r = 0; r < n_shards; ++r) {
    if (ids[r] < 0 || ids[r] >= n_dev) { set_error("rtx_multi_create: device " + std::to_string(ids[r]) + " does not exist (" + std::to_string(n_dev) + " visible)"); return RTX_EINVAL; }
    if (ids[r] != ids[0]) all_same = false;
    for (int q = 0; q < r; ++q) if (ids[q] == ids[r]) all_distinct = false;
  }
  if (!all_distinct && !all_same) { set_error("rtx_multi_create: device ids must be all distinct (one shard per GPU) or all equal (rehearsal on one GPU)"); return RTX_EINVAL; }
  int saved = 0;
  (void)hipGetDevice(&saved);
  rtx_multi* m = new (std::nothrow) rtx_multi();
  if (!m) { set_error("out of memory"); return RTX_ENOMEM; }
  m->n_shards = n_shards;
  m->block_rows = block_rows;
  m->same_device = all_same && n_shards > 1;
  m->use_rccl = !m->same_device;  // n_shards == 1 goes through RCCL too: one code path for 1..8 GPUs
  const int n_entries = m->same_device ? 1 : n_shards;
  m->dev.resize((size_t)n_entries);
  rtx_status st = RTX_OK;
  for (int k = 0; k < n_entries && st == RTX_OK; ++k) {
    MultiDevice& d = m->dev[k];
    d.device = ids[k];
    if (hipSetDevice(d.device) != hipSuccess) { set_error("rtx_multi_create: hipSetDevice failed"); st = RTX_EHIP; break; }
    if (hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&d.ev0) != hipSuccess || hipEventCreate(&d.ev1) != hipSuccess) { set_error("rtx_multi_create: stream/event creation failed"); st = RTX_EHIP; break; }
    st = f32 ? rtx_scene_upload_f32(f, &d.scene) : rtx_scene_upload(f, &d.scene);
  }
  if (st == RTX_OK && (hipSetDevice(m->dev[0].device) != hipSuccess || hipEventCreate(&m->ev_gather0) != hipSuccess ||
                       hipEventCreate(&m->ev_gather1) != hipSuccess)) { set_error("rtx_multi_create: event creation failed"); st = RTX_EHIP; }
  if (st == RTX_OK && m->use_rccl) {
    RcclApi* api = rccl_api();
    if (!api) { set_error("rtx_multi_create: librccl.so could not be loaded"); st = RTX_ENCCL; }
    else {
      std::vector<nccl_comm_t> comms((size_t)n_entries, nullptr);
      const int rc = api->CommInitAll(comms.data(), n_entries, ids.data());
      if (rc != 0) { set_error(std::string("ncclCommInitAll: ") + api->GetErrorString(rc)); st = RTX_ENCCL; }
      else {
        for (int k = 0; k < n_entries; ++k) m->dev[k].comm = comms[k];
        int cnt = 0;
        if (api->CommCount && api->CommCount(comms[0], &cnt) == 0) m->rccl_ranks = cnt;
      }
    }
  }
  (void)hipSetDevice(saved);
  if (st != RTX_OK) { multi_free(m); return st; }
  *out = m;
  return RTX_OK;
}

extern "C" {

rtx_status rtx_multi_create(const rtx_flat* f, int32_t n_shards, const int32_t* device_ids, int32_t block_rows, rtx_multi** out) {
  return multi_create(f, n_shards, device_ids, block_rows, false, out);
}
rtx_status rtx_multi_create_f32(const rtx_flat* f, int32_t n_shards, const int32_t* device_ids, int32_t block_rows, rtx_multi** out) {
  return multi_create(f, n_shards, device_ids, block_rows, true, out);
}

void rtx_multi_destroy(rtx_multi* m) {
  int saved = 0;
  (void)hipGetDevice(&saved);
  rtx::multi_free(m);
  (void)hipSetDevice(saved);
}

rtx_status rtx_multi_render(rtx_multi* m, const RtxCamera* cam, const RtxConfig* cfg, RtxFrame* out, RtxMultiStats* stats) {
  using namespace rtx;
  if (!m || !cam || !cfg || !out) { set_error("rtx_multi_render: NULL argument"); return RTX_EINVAL; }
  RtxShard whole;
  rtx_status st = validate(m->dev[0].scene, cam, cfg, nullptr, &whole);
  if (st != RTX_OK) return st;
  const int32_t w = cfg->image_width, h = rtx_image_height(cfg);
  const int n = m->n_shards;
  int32_t max_rows = 0;
  for (int r = 0; r < n; ++r) {
    RtxShard sh = {r, n, m->block_rows, 0};
    max_rows = std::max(max_rows, rtx_shard_rows(cfg, &sh));
  }
  const size_t shard_px = (size_t)max_rows * (size_t)w;
  const bool want_accum = out->accum_rgb != nullptr;
  int saved = 0;
  (void)hipGetDevice(&saved);
  // Leaving early (a failed launch, a failed collective) must not leave work in flight: a later grow() / hipFree / destroy would
  // race it.  Every exit that is not the regular one drains all device streams first; then the caller's device is current again.
  struct Drain {
    rtx_multi* m; int d; bool armed;
    ~Drain() {
      if (armed)
        for (MultiDevice& x : m->dev)
          if (x.stream && hipSetDevice(x.device) == hipSuccess) (void)hipStreamSynchronize(x.stream);
      (void)hipSetDevice(d);
    }
  } drain{m, saved, true};
  const auto t_begin = std::chrono::steady_clock::now();

  // ---- buffers
  for (MultiDevice& d : m->dev) {
    HIP_TRY(hipSetDevice(d.device));
    const size_t per = m->same_device ? (size_t)n : 1;  // the rehearsal device holds every shard
    HIP_TRY(d.d_rgb8.grow(per * shard_px * 3, d.stream));
    if (want_accum) HIP_TRY(d.d_accum.grow(per * shard_px * 24, d.stream));
  }
  MultiDevice& root = m->dev[0];
  HIP_TRY(hipSetDevice(root.device));
  HIP_TRY(m->d_gather8.grow((size_t)n * shard_px * 3, root.stream));
  HIP_TRY(m->d_image8.grow((size_t)w * h * 3, root.stream));
  if (want_accum) {
    HIP_TRY(m->d_gather64.grow((size_t)n * shard_px * 24, root.stream));
    HIP_TRY(m->d_image64.grow((size_t)w * h * 24, root.stream));
  }

  // ---- render: every device its shard, all at once (launches are asynchronous)
  for (int r = 0; r < n; ++r) {
    MultiDevice& d = m->same_device ? m->dev[0] : m->dev[r];
    HIP_TRY(hipSetDevice(d.device));
    RtxShard sh = {r, n, m->block_rows, 0};
    uint8_t* rgb = d.d_rgb8 + (m->same_device ? (size_t)r * shard_px * 3 : 0);
    double* acc = want_accum ? d.d_accum + (m->same_device ? (size_t)r * shard_px * 3 : 0) : nullptr;
    if (r == 0 || !m->same_device) HIP_TRY(hipEventRecord(d.ev0, d.stream));
    st = render_any(d.scene, cam, cfg, &sh, acc, rgb, d.stream, nullptr);
    if (st != RTX_OK) return st;
    if (r == n - 1 || !m->same_device) HIP_TRY(hipEventRecord(d.ev1, d.stream));
  }
  // ---- gather to device 0
  HIP_TRY(hipSetDevice(root.device));
  HIP_TRY(hipEventRecord(m->ev_gather0, root.stream));
  if (m->use_rccl) {
    RcclApi* api = rccl_api();
    int rc = api->GroupStart();
    for (int r = 0; r < n && rc == 0; ++r) {
      MultiDevice& d = m->dev[r];
      rc = api->Gather(d.d_rgb8, r == 0 ? m->d_gather8 : nullptr, shard_px * 3, NCCL_UINT8, 0, d.comm, d.stream);
      if (rc == 0 && want_accum)
        rc = api->Gather(d.d_accum, r == 0 ? (void*)m->d_gather64 : nullptr, shard_px * 24, NCCL_UINT8, 0, d.comm, d.stream);
    }
    const int rc2 = api->GroupEnd();
    if (rc != 0 || rc2 != 0) { set_error(std::string("ncclGather: ") + api->GetErrorString(rc != 0 ? rc : rc2)); return RTX_ENCCL; }
  } else {
    HIP_TRY(hipSetDevice(root.device));
    HIP_TRY(hipMemcpyAsync(m->d_gather8, root.d_rgb8, (size_t)n * shard_px * 3, hipMemcpyDeviceToDevice, root.stream));
    if (want_accum) HIP_TRY(hipMemcpyAsync(m->d_gather64, root.d_accum, (size_t)n * shard_px * 24, hipMemcpyDeviceToDevice, root.stream));
  }
  // ---- rows back into image order, frame to the host
  HIP_TRY(hipSetDevice(root.device));
  {
    const uint64_t elems = (uint64_t)w * h * 3;
    const uint32_t grid = (uint32_t)((elems + 255) / 256);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_untile_rows<uint8_t>), dim3(grid), dim3(256), 0, root.stream, m->d_gather8, m->d_image8,
                       (uint32_t)w, (uint32_t)h, (uint32_t)n, (uint32_t)m->block_rows, (uint32_t)max_rows);
    if (want_accum)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_untile_rows<double>), dim3(grid), dim3(256), 0, root.stream, m->d_gather64, m->d_image64,
                         (uint32_t)w, (uint32_t)h, (uint32_t)n, (uint32_t)m->block_rows, (uint32_t)max_rows);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(m->ev_gather1, root.stream));
    if (out->rgb8) HIP_TRY(hipMemcpyAsync(out->rgb8, m->d_image8, elems, hipMemcpyDeviceToHost, root.stream));
    if (want_accum) HIP_TRY(hipMemcpyAsync(out->accum_rgb, m->d_image64, elems * 8, hipMemcpyDeviceToHost, root.stream));
  }
  for (MultiDevice& d : m->dev) {
    HIP_TRY(hipSetDevice(d.device));
    HIP_TRY(hipStreamSynchronize(d.stream));
  }
  drain.armed = false;
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    stats->n_shards = n;
    stats->n_devices = (int32_t)m->dev.size();
    stats->used_rccl = m->use_rccl ? 1 : 0;
    stats->rccl_ranks = m->rccl_ranks;
    for (size_t k = 0; k < m->dev.size(); ++k) {
      MultiDevice& d = m->dev[k];
      float ms = 0.f;
      HIP_TRY(hipSetDevice(d.device));
      if (hipEventElapsedTime(&ms, d.ev0, d.ev1) == hipSuccess) {
        stats->render_ms_max = std::max(stats->render_ms_max, (double)ms);
        if (k < 16) stats->render_ms[k] = (double)ms;
      }
    }
    {
      // root's stream: end of its own shard -> shards of every device in place and in row order (waits for the slowest peer)
      float ms = 0.f;
      HIP_TRY(hipSetDevice(root.device));
      if (hipEventElapsedTime(&ms, m->ev_gather0, m->ev_gather1) == hipSuccess) stats->gather_ms = (double)ms;
    }
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    stats->gathered_bytes = (uint64_t)n * shard_px * (want_accum ? 27u : 3u);
  }
  return RTX_OK;
}

rtx_status rtx_render_multi(const rtx_flat* f, const RtxCamera* cam, const RtxConfig* cfg, int32_t n_gpus, RtxFrame* out) {
  rtx_multi* m = nullptr;
  rtx_status st = rtx_multi_create(f, n_gpus, nullptr, 1, &m);
  if (st != RTX_OK) return st;
  st = rtx_multi_render(m, cam, cfg, out, nullptr);
  rtx_multi_destroy(m);
  return st;
}

}  // extern "C"
