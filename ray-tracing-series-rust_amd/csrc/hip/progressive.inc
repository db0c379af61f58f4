// Progressive rendering (rtx_progressive_*, included by render.hip's f64 compilation after the C ABI).
//
// A handle keeps one (scene, camera, config, shard)'s accumulators S (sum of radiances) and Q (sum of their squares) in
// device memory across calls.  rtx_progressive_add(n) traces the absolute samples [spp_done, spp_done + n) of every pixel
// through render_impl (SampleRange: same passes, pipelining and kernel choice as a one-shot render) and adds them onto S and
// Q in sample order.  Since every path's random stream is keyed by its absolute (pixel, sample) index, the frame after k
// samples -- however they were split across calls -- is bit-identical to a one-shot render at k spp.
//
// Adaptive rounds (rtx_progressive_add_adaptive / _until_adaptive) stop tracing the pixels that reached the target: a
// retirement check (k_retire_flag / _scan / _scatter) freezes a pixel's count n_p at spp_done once its relative error is at
// most the target, and compacts the ascending list of the still-active pixels; the round's samples are then traced for the
// listed pixels only (SampleRange::active, pass_items.inc).  Every active pixel holds spp_done samples, so a pass keeps one
// s_begin.  Until the first pixel retires, rounds trace through the uniform path and the handle is a uniform one.
//
// The handle borrows the scene's render workspace (sample buffer, work counters, pipelining stream): it must not run at the
// same time as another render of the same scene on another stream, and it must be destroyed before its scene.

// The filter's device buffers for one image (denoise_launch): two (c, sigma2) planes to ping-pong between, n^, and the
// finished mean and rgb8.
struct DenoiseBuffers {
  DeviceBuffer<float4> cv[2], nhat;
  DeviceBuffer<double> mean;
  DeviceBuffer<uint8_t> rgb8;
};

// The retirement check's compaction scratch (retire_scratch_alloc): one ballot per wave, the block counts, their offsets and total.
struct RetireScratch {
  DeviceBuffer<unsigned long long> keep_mask;
  DeviceBuffer<uint32_t> block_count, block_offset;
};

struct rtx_progressive {
  const rtx_scene* scene;
  RtxCamera cam;
  RtxConfig cfg;
  RtxShard shard;
  int device;
  uint32_t npix_all;  // pixels of the shard
  uint32_t npix;      // of which active (row_chunk_compat leaves the rest zero)
  int32_t spp_done;
  bool light_sampling;  // every add traces with next-event estimation (rtx_progressive_create_ex)
  bool broken;        // a failed add left S / Q partly updated
  DeviceBuffer<double> S, Q;
  DeviceBuffer<NoisePartial> partials;  // one per 256 active pixels, then the final result (noise_partials_alloc)
  // adaptive state, allocated by the first adaptive call (a uniform handle keeps its 48 bytes per pixel)
  bool adaptive;
  int cur;                  // active[cur]: the ascending list of the n_active local pixels still active
  DeviceBuffer<uint32_t> active[2];  // (the other one: the compaction's target)
  uint32_t n_active;        // npix until the first pixel retires
  DeviceBuffer<int32_t> counts;  // per pixel of the shard: n_p of a retired pixel, 0 for an active one (or a row never rendered)
  RetireScratch scratch;
  uint64_t retired_samples;  // sum of n_p over the retired pixels
  // denoising state, allocated by the first features / denoise call (denoise.inc)
  int32_t feature_spp;       // of the features held (0: none yet)
  DeviceBuffer<float4> albedo, normal;  // per pixel: the feature pass's albedo, normal
  DenoiseBuffers denoise;    // the filter's buffers, allocated by the first denoise call
};

namespace {

bool any_retired(const rtx_progressive* p) { return p->adaptive && p->n_active < p->npix; }

// Traces the samples [spp_done, spp_done + n) onto S and Q: of every pixel, or -- once pixels have retired (adaptive rounds) --
// of the listed pixels still active; with none active it traces nothing (spp_done still advances).  A failed trace leaves S
// and Q partly updated: the handle is broken.
rtx_status progressive_add(rtx_progressive* p, int32_t n, hipStream_t stream, RtxRenderStats* stats) {
  const bool listed = any_retired(p);
  if (listed && p->n_active == 0) {
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->trace_kernel = RTX_KERNEL_SIMPLE; }  // nothing traced
    p->spp_done += n;
    return RTX_OK;
  }
  // (a pixel retires at spp_done >= 2 at the earliest: a listed range always continues)
  const SampleRange range = {(uint32_t)p->spp_done, (uint32_t)n, p->spp_done > 0 ? 1 : 0, p->Q,
                             listed ? (const uint32_t*)p->active[p->cur] : nullptr, listed ? p->n_active : 0u, p->light_sampling};
  const rtx_status st = p->scene->ops->render(p->scene->device_scene, &p->cam, &p->cfg, &p->shard, p->S, nullptr, stream, stats, &range);
  if (st != RTX_OK) { p->broken = true; return st; }
  p->spp_done += n;
  return RTX_OK;
}

// The entries' check of a number of samples to add.
bool n_samples_ok(const rtx_progressive* p, const char* fn, int32_t n_samples) {
  if (n_samples > 0 && n_samples <= p->cfg.samples_per_pixel - p->spp_done) return true;
  set_error(std::string(fn) + ": n_samples must be in [1, samples_per_pixel - spp_done] = [1, " +
            std::to_string(p->cfg.samples_per_pixel - p->spp_done) + "]");
  return false;
}

// The noise reduction's partials for npix pixels: one per 256-pixel block, then the final result.
hipError_t noise_partials_alloc(uint32_t npix, DeviceBuffer<NoisePartial>* partials) {
  return partials->alloc((((size_t)npix + 255) / 256 + 1) * sizeof(NoisePartial));
}

// The noise reduction on device arrays, shared by the handle and rtx_device_noise_reduce: k_noise_stats (counts NULL) or
// k_noise_stats_counts over the npix >= 1 pixels into partials[0, nb), nb = ceil(npix / 256), then k_noise_stats_final
// into partials[nb] (noise_partials_alloc), copied to *r.  Blocking; runs on the default stream.
rtx_status noise_reduce_launch(const double* S, const double* Q, const int32_t* counts, uint32_t npix, uint32_t spp,
                               double target, NoisePartial* partials, NoisePartial* r) {
  const uint32_t nb = (npix + 255u) / 256u;
  if (counts)
    hipLaunchKernelGGL(k_noise_stats_counts, dim3(nb), dim3(256), 0, (hipStream_t) nullptr, S, Q, counts, npix, spp, target,
                       partials);
  else
    hipLaunchKernelGGL(k_noise_stats, dim3(nb), dim3(256), 0, (hipStream_t) nullptr, S, Q, npix, spp, target, partials);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_noise_stats_final, dim3(1), dim3(256), 0, (hipStream_t) nullptr, partials, nb, partials + nb);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(r, partials + nb, sizeof(*r), hipMemcpyDeviceToHost));
  return RTX_OK;
}

// Reduces r over the shard's active pixels (each pixel at its own n_p once one has retired).
rtx_status noise_reduce(rtx_progressive* p, double target, NoisePartial* r) {
  HIP_TRY(hipDeviceSynchronize());  // the adds ran on the caller's stream
  return noise_reduce_launch(p->S, p->Q, any_retired(p) ? p->counts : nullptr, p->npix, (uint32_t)p->spp_done, target,
                             p->partials, r);
}

// The error fields of a stats struct (RtxNoiseStats, RtxAdaptiveStats) from the reduction over the handle's npix >= 1 pixels.
template <class Stats>
rtx_status error_stats(rtx_progressive* p, double target, Stats* out) {
  NoisePartial r;
  const rtx_status st = noise_reduce(p, target, &r);
  if (st != RTX_OK) return st;
  out->pixels_above = (int32_t)r.above;
  out->max_rel_err = r.max_r;
  out->mean_rel_err = r.sum_r / (double)p->npix;
  return RTX_OK;
}

// A RtxNoiseStats without its error fields.
void noise_stats_head(const rtx_progressive* p, double target, RtxNoiseStats* out) {
  memset(out, 0, sizeof(*out));
  out->spp_done = p->spp_done;
  out->pixels = (int32_t)p->npix;
  out->target_rel_err = target;
}

rtx_status progressive_stats(rtx_progressive* p, double target, RtxNoiseStats* out) {
  noise_stats_head(p, target, out);
  return p->npix == 0 ? RTX_OK : error_stats(p, target, out);
}

bool progressive_usable(const rtx_progressive* p, const char* fn) {
  if (!p) { set_error(std::string(fn) + ": NULL handle"); return false; }
  if (p->broken) { set_error(std::string(fn) + ": an earlier rtx_progressive_add failed; the accumulators are incomplete"); return false; }
  return true;
}

// The uniform entries would give every pixel the next samples, leaving a gap in a retired pixel's sample indices.
bool uniform_allowed(const rtx_progressive* p, const char* fn) {
  if (!any_retired(p)) return true;
  set_error(std::string(fn) + ": pixels of this handle have retired (adaptive rounds); continue with the adaptive entries");
  return false;
}

// The adaptive entries' common argument checks (before any device call).
bool adaptive_args_ok(const rtx_progressive* p, const char* fn, int32_t min_spp, double target) {
  if (min_spp < 2 || min_spp > p->cfg.samples_per_pixel) {
    set_error(std::string(fn) + ": min_spp must be in [2, samples_per_pixel] = [2, " + std::to_string(p->cfg.samples_per_pixel) + "]");
    return false;
  }
  if (!(target >= 0.0)) { set_error(std::string(fn) + ": target_rel_err must be >= 0"); return false; }
  return true;
}

// The retirement check's scratch for lists of up to n pixels (nb = ceil(n / 256) blocks): one ballot per wave (nb * 4, and
// one spare), the block counts (nb + 1) and their exclusive offsets with the total at [nb] (nb + 1).
hipError_t retire_scratch_alloc(uint32_t n, RetireScratch* s) {
  const uint32_t nb = (n + 255u) / 256u;
  hipError_t e = s->keep_mask.alloc(((size_t)nb * 4 + 1) * 8);
  if (e == hipSuccess) e = s->block_count.alloc(((size_t)nb + 1) * 4);
  if (e == hipSuccess) e = s->block_offset.alloc(((size_t)nb + 1) * 4);
  return e;
}

// The retirement check on device arrays, shared by the handle and rtx_device_retire: every pixel of list[0, n) (n >= 1)
// with r <= target at spp samples gets counts[lp] = spp; the others are compacted, in order, into next[0, *kept).  The
// scratch comes from retire_scratch_alloc for at least n pixels.  Blocking (the host needs the count).
rtx_status retire_launch(const double* S, const double* Q, const uint32_t* list, uint32_t n, uint32_t spp, double target,
                         int32_t* counts, const RetireScratch& sc, uint32_t* next, hipStream_t stream, uint32_t* kept) {
  const uint32_t nb = (n + 255u) / 256u;
  hipLaunchKernelGGL(k_retire_flag, dim3(nb), dim3(256), 0, stream, S, Q, list, n, spp, target, counts, sc.keep_mask,
                     sc.block_count);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_retire_scan, dim3(1), dim3(256), 0, stream, sc.block_count, nb, sc.block_offset);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_retire_scatter, dim3(nb), dim3(256), 0, stream, list, n, sc.keep_mask, sc.block_offset, next);
  HIP_TRY(hipGetLastError());
  *kept = 0;
  HIP_TRY(hipMemcpyAsync(kept, sc.block_offset + nb, sizeof(*kept), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  if (*kept > n) { set_error("progressive: the retirement check counted more pixels than it was given"); return RTX_EHIP; }
  return RTX_OK;
}

// Allocates the adaptive buffers on the first adaptive call: every active pixel listed, no count frozen.  The buffers are
// built in locals and move into the handle together with `adaptive`: a failure frees them all and leaves the handle as it was.
rtx_status adaptive_init(rtx_progressive* p) {
  if (p->adaptive) return RTX_OK;
  const uint32_t nb = (p->npix + 255u) / 256u;
  DeviceBuffer<uint32_t> active[2];
  DeviceBuffer<int32_t> counts;
  RetireScratch scratch;
  hipError_t e = hipSuccess;
  for (DeviceBuffer<uint32_t>& a : active)
    if (e == hipSuccess) e = a.alloc(((size_t)p->npix + 1) * 4);
  if (e == hipSuccess) e = counts.alloc(((size_t)p->npix_all + 1) * 4);
  if (e == hipSuccess) e = retire_scratch_alloc(p->npix, &scratch);
  if (e == hipSuccess) e = hipMemset(counts, 0, ((size_t)p->npix_all + 1) * 4);
  if (e == hipSuccess && p->npix) {
    hipLaunchKernelGGL(k_iota, dim3(nb), dim3(256), 0, (hipStream_t) nullptr, active[0], p->npix);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error(std::string("progressive: adaptive buffers: ") + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? RTX_ENOMEM : RTX_EHIP;
  }
  p->active[0] = std::move(active[0]);
  p->active[1] = std::move(active[1]);
  p->counts = std::move(counts);
  p->scratch = std::move(scratch);
  p->adaptive = true;
  p->cur = 0;
  p->n_active = p->npix;
  p->retired_samples = 0;
  return RTX_OK;
}

// The retirement check of an adaptive round at n = spp_done (the caller has checked spp_done >= max(2, min_spp)): freezes the
// count of every active pixel with r <= target and compacts the list of the others.  Blocking (the host needs the new count).
rtx_status adaptive_retire_launch(rtx_progressive* p, double target, hipStream_t stream) {
  if (p->n_active == 0) return RTX_OK;
  const uint32_t n = p->n_active, spp = (uint32_t)p->spp_done;
  uint32_t kept = 0;
  const rtx_status st = retire_launch(p->S, p->Q, p->active[p->cur], n, spp, target, p->counts, p->scratch,
                                      p->active[1 - p->cur], stream, &kept);
  if (st != RTX_OK) return st;
  p->retired_samples += (uint64_t)(n - kept) * spp;
  p->n_active = kept;
  p->cur = 1 - p->cur;
  return RTX_OK;
}

rtx_status adaptive_retire(rtx_progressive* p, double target, hipStream_t stream) {
  const rtx_status st = adaptive_retire_launch(p, target, stream);
  if (st != RTX_OK) p->broken = true;  // counts may be frozen for a list that was not compacted
  return st;
}

// A retirement check is due at spp_done >= max(2, min_spp); min_spp >= 2 is checked by every entry.
bool check_due(const rtx_progressive* p, int32_t min_spp) { return p->spp_done >= min_spp; }

rtx_status adaptive_stats(rtx_progressive* p, int32_t min_spp, double target, RtxAdaptiveStats* out) {
  memset(out, 0, sizeof(*out));
  out->spp_done = p->spp_done;
  out->min_spp = min_spp;
  out->pixels = (int32_t)p->npix;
  out->pixels_active = (int32_t)(p->adaptive ? p->n_active : p->npix);
  out->samples = p->adaptive ? p->retired_samples + (uint64_t)p->n_active * (uint64_t)p->spp_done
                             : (uint64_t)p->npix * (uint64_t)p->spp_done;
  out->target_rel_err = target;
  if (p->npix == 0 || p->spp_done < 2) return RTX_OK;
  return error_stats(p, target, out);
}

// Spare bytes behind every device copy of a self-test entry's array: never 0 bytes.
const size_t SELF_TEST_SPARE = 8;

// The self-test entries' argument checks (before any device call).
bool self_test_args_ok(const char* fn, bool pointers, uint32_t npix, uint32_t spp, double target) {
  if (!pointers) { set_error(std::string(fn) + ": NULL argument"); return false; }
  if (npix >= (1u << 31)) { set_error(std::string(fn) + ": more than 2^31 pixels"); return false; }
  if (spp < 2 || spp > (uint32_t)INT32_MAX) { set_error(std::string(fn) + ": spp must be in [2, 2^31)"); return false; }
  if (!(target >= 0.0)) { set_error(std::string(fn) + ": target must be >= 0"); return false; }
  return true;
}

// ---- denoising (denoise.inc)

// The filter's parameters with the defaults filled in, checked before any device call; feature_spp gets the feature pass's.
bool denoise_rule(const RtxDenoiseParams* params, const char* fn, DenoiseRule* r, int32_t* feature_spp) {
  RtxDenoiseParams d;
  memset(&d, 0, sizeof(d));
  if (params) d = *params;
  const int32_t k = d.iterations ? d.iterations : 5, fs = d.feature_spp ? d.feature_spp : 4;
  if (k < 1 || k > 8) { set_error(std::string(fn) + ": iterations must be in [1, 8] (0 = 5)"); return false; }
  if (fs < 1 || fs > 64) { set_error(std::string(fn) + ": feature_spp must be in [1, 64] (0 = 4)"); return false; }
  if (d.demodulate < -1 || d.demodulate > 1) { set_error(std::string(fn) + ": demodulate must be -1 (off), 0 or 1 (on)"); return false; }
  const double sig[3] = {d.sigma_luminance, d.sigma_normal, d.sigma_albedo}, dflt[3] = {4.0, 32.0, 0.3};
  double v[3];
  for (int c = 0; c < 3; ++c) {
    if (!(sig[c] >= 0.0 && sig[c] <= 1e30)) { set_error(std::string(fn) + ": sigmas must be in [0, 1e30] (0 = default)"); return false; }
    v[c] = sig[c] > 0.0 ? sig[c] : dflt[c];
  }
  r->iterations = k;
  r->demodulate = d.demodulate >= 0 ? 1 : 0;
  r->sigma_l = (float)v[0];
  r->sigma_n = (float)v[1];
  const double inv_a2 = 1.0 / (v[2] * v[2]);  // a tiny sigma_a: FLT_MAX, not inf (0 * inf at equal albedos would be NaN)
  r->inv_sigma_a2 = inv_a2 < (double)FLT_MAX ? (float)inv_a2 : FLT_MAX;
  if (feature_spp) *feature_spp = fs;
  return true;
}

// The filter over a w x h image on the default stream: k_denoise_prepare from S and Q at each pixel's count (moments = 1) or
// from m and v (moments = 0), then the levels; the last one finishes into b.mean / b.rgb8 where want_mean / want_rgb8.
// Blocking.
rtx_status denoise_launch(int32_t w, int32_t h, const DenoiseRule& r, const double* s_or_m, const double* q_or_v,
                          const int32_t* counts, uint32_t spp, int moments, const float4* albedo, const float4* normal,
                          const DenoiseBuffers& b, bool want_mean, bool want_rgb8) {
  const uint32_t npix = (uint32_t)((size_t)w * (size_t)h);
  if (npix == 0) return RTX_OK;
  hipLaunchKernelGGL(k_denoise_prepare, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t) nullptr, s_or_m, q_or_v, counts,
                     spp, moments, npix, r.demodulate, albedo, normal, b.cv[0], b.nhat);
  HIP_TRY(hipGetLastError());
  const uint32_t nbx = ((uint32_t)w + DENOISE_BX - 1) / DENOISE_BX, nby = ((uint32_t)h + DENOISE_BY - 1) / DENOISE_BY;
  const dim3 grid(nbx * nby), block(DENOISE_BX, DENOISE_BY);
  for (int k = 0; k < r.iterations; ++k) {
    const float4* in = b.cv[k & 1];
    if (k + 1 < r.iterations)
      hipLaunchKernelGGL(k_denoise_level<false>, grid, block, 0, (hipStream_t) nullptr, in, albedo, b.nhat, w, h, 1 << k, nbx, r,
                         b.cv[(k + 1) & 1], nullptr, nullptr);
    else
      hipLaunchKernelGGL(k_denoise_level<true>, grid, block, 0, (hipStream_t) nullptr, in, albedo, b.nhat, w, h, 1 << k, nbx, r,
                         nullptr, want_mean ? (double*)b.mean : nullptr, want_rgb8 ? (uint8_t*)b.rgb8 : nullptr);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipDeviceSynchronize());
  return RTX_OK;
}

// The filter's buffers for an image of n pixels.
hipError_t denoise_buffers_alloc(size_t n, DenoiseBuffers* b) {
  hipError_t e = b->cv[0].alloc(n * 16 + 16);
  if (e == hipSuccess) e = b->cv[1].alloc(n * 16 + 16);
  if (e == hipSuccess) e = b->nhat.alloc(n * 16 + 16);
  if (e == hipSuccess) e = b->mean.alloc(n * 24 + 8);
  if (e == hipSuccess) e = b->rgb8.alloc(n * 3 + 8);
  return e;
}

// Denoising needs every row of the image: a whole-image handle without row_chunk_compat.
bool denoise_supported(const rtx_progressive* p, const char* fn) {
  if (p->shard.shard_count == 1 && !p->cfg.row_chunk_compat) return true;
  set_error(std::string(fn) + ": a sharded or row_chunk_compat handle has rows missing; the spatial filter needs them all");
  return false;
}

// The handle's features for feature_spp samples, computed (and the buffers allocated) unless they are already there.  Blocking.
rtx_status ensure_features(rtx_progressive* p, int32_t feature_spp) {
  if (p->feature_spp == feature_spp) return RTX_OK;
  HIP_TRY(hipDeviceSynchronize());  // adds may still run on the caller's stream (the feature pass shares nothing with them)
  const size_t bytes = (size_t)p->npix_all * 16 + 16;
  if (!p->albedo) HIP_TRY(p->albedo.alloc(bytes));
  if (!p->normal) HIP_TRY(p->normal.alloc(bytes));
  p->feature_spp = 0;
  const rtx_status st = p->scene->ops->features(p->scene->device_scene, &p->cam, &p->cfg, feature_spp, p->albedo, p->normal,
                                                 (hipStream_t) nullptr);
  if (st != RTX_OK) return st;
  HIP_TRY(hipDeviceSynchronize());
  p->feature_spp = feature_spp;
  return RTX_OK;
}

// float4 per pixel (device) -> 3 floats per pixel (host).
rtx_status download_xyz(const float4* d, size_t npix, float* out) {
  std::vector<float4> h(npix);
  if (npix) HIP_TRY(hipMemcpy(h.data(), d, npix * 16, hipMemcpyDeviceToHost));
  for (size_t k = 0; k < npix; ++k) { out[3 * k] = h[k].x; out[3 * k + 1] = h[k].y; out[3 * k + 2] = h[k].z; }
  return RTX_OK;
}

}  // namespace

extern "C" {

rtx_status rtx_progressive_create_ex(const rtx_scene* s, const RtxCamera* cam, const RtxConfig* cfg, const RtxShard* shard,
                                     const RtxIntegratorOptions* opt, rtx_progressive** out) {
  if (!out) { set_error("rtx_progressive_create_ex: NULL out"); return RTX_EINVAL; }
  *out = nullptr;
  bool nee = false;
  rtx_status st = check_integrator_options(s, opt, "rtx_progressive_create_ex", &nee);
  if (st != RTX_OK) return st;
  st = rtx_progressive_create(s, cam, cfg, shard, out);
  if (st == RTX_OK) (*out)->light_sampling = nee;
  return st;
}

rtx_status rtx_progressive_create(const rtx_scene* s, const RtxCamera* cam, const RtxConfig* cfg, const RtxShard* shard,
                                  rtx_progressive** out) {
  if (!out) { set_error("rtx_progressive_create: NULL out"); return RTX_EINVAL; }
  *out = nullptr;
  RtxShard sh;
  rtx_status st = validate(s, cam, cfg, shard, &sh);
  if (st != RTX_OK) return st;
  const int32_t w = cfg->image_width, h = rtx_image_height(cfg);
  const int32_t row_limit = cfg->row_chunk_compat ? (h / cfg->threads) * cfg->threads : h;
  const uint64_t npix_all = (uint64_t)shard_row_count(h, sh, h) * w, npix = (uint64_t)shard_row_count(h, sh, row_limit) * w;
  if (npix_all >= (1ull << 31)) { set_error("rtx_progressive_create: shard larger than 2^31 pixels"); return RTX_EINVAL; }
  rtx_progressive* p = new rtx_progressive();
  p->scene = s;
  p->cam = *cam;
  p->cfg = *cfg;
  p->shard = sh;
  p->npix_all = (uint32_t)npix_all;
  p->npix = (uint32_t)npix;
  hipError_t e = hipGetDevice(&p->device);
  const size_t plane = (size_t)npix_all * 24;
  if (e == hipSuccess && plane) e = p->S.alloc(plane);
  if (e == hipSuccess && plane) e = p->Q.alloc(plane);
  if (e == hipSuccess) e = noise_partials_alloc(p->npix, &p->partials);
  if (e == hipSuccess && plane) e = hipMemset(p->S, 0, plane);  // rows beyond row_chunk_compat's limit stay zero
  if (e == hipSuccess && plane) e = hipMemset(p->Q, 0, plane);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error(std::string("rtx_progressive_create: ") + hipGetErrorString(e));
    delete p;
    return e == hipErrorOutOfMemory ? RTX_ENOMEM : RTX_EHIP;
  }
  *out = p;
  return RTX_OK;
}

void rtx_progressive_destroy(rtx_progressive* p) {
  if (!p) return;
  (void)hipDeviceSynchronize();  // an add may still be running on the caller's stream
  delete p;
}

int32_t rtx_progressive_spp(const rtx_progressive* p) { return p ? p->spp_done : -1; }

rtx_status rtx_progressive_add(rtx_progressive* p, int32_t n_samples, void* hip_stream, RtxRenderStats* stats) {
  if (!progressive_usable(p, "rtx_progressive_add") || !uniform_allowed(p, "rtx_progressive_add")) return RTX_EINVAL;
  if (!n_samples_ok(p, "rtx_progressive_add", n_samples)) return RTX_EINVAL;
  return progressive_add(p, n_samples, (hipStream_t)hip_stream, stats);
}

rtx_status rtx_progressive_read(const rtx_progressive* p, RtxFrame* out, double* sumsq_rgb) {
  if (!progressive_usable(p, "rtx_progressive_read")) return RTX_EINVAL;
  if (!out) { set_error("rtx_progressive_read: NULL frame"); return RTX_EINVAL; }
  if (p->spp_done <= 0) { set_error("rtx_progressive_read: no samples yet"); return RTX_EINVAL; }
  const size_t plane = (size_t)p->npix_all * 24;
  HIP_TRY(hipDeviceSynchronize());
  if (out->accum_rgb && plane) HIP_TRY(hipMemcpy(out->accum_rgb, p->S, plane, hipMemcpyDeviceToHost));
  if (sumsq_rgb && plane) HIP_TRY(hipMemcpy(sumsq_rgb, p->Q, plane, hipMemcpyDeviceToHost));
  if (out->rgb8 && plane) {
    DeviceBuffer<uint8_t> d_rgb;
    HIP_TRY(d_rgb.alloc((size_t)p->npix_all * 3));
    HIP_TRY(hipMemset(d_rgb, 0, (size_t)p->npix_all * 3));
    // once pixels have retired, each pixel by its own count
    const rtx_status st = p->scene->ops->tonemap(p->S, d_rgb, any_retired(p) ? (const int32_t*)p->counts : nullptr, p->npix,
                                                 (uint32_t)p->spp_done, (hipStream_t) nullptr);
    if (st != RTX_OK) return st;
    HIP_TRY(hipMemcpy(out->rgb8, d_rgb, (size_t)p->npix_all * 3, hipMemcpyDeviceToHost));
  }
  return RTX_OK;
}

rtx_status rtx_progressive_stats(rtx_progressive* p, double target_rel_err, RtxNoiseStats* out) {
  if (!progressive_usable(p, "rtx_progressive_stats")) return RTX_EINVAL;
  if (!out) { set_error("rtx_progressive_stats: NULL out"); return RTX_EINVAL; }
  if (!(target_rel_err >= 0.0)) { set_error("rtx_progressive_stats: target_rel_err must be >= 0"); return RTX_EINVAL; }
  if (p->spp_done < 2) { set_error("rtx_progressive_stats: the variance needs at least 2 samples"); return RTX_EINVAL; }
  return progressive_stats(p, target_rel_err, out);
}

rtx_status rtx_progressive_until(rtx_progressive* p, int32_t batch, double target_rel_err, RtxNoiseStats* out) {
  if (!progressive_usable(p, "rtx_progressive_until") || !uniform_allowed(p, "rtx_progressive_until")) return RTX_EINVAL;
  if (!out) { set_error("rtx_progressive_until: NULL out"); return RTX_EINVAL; }
  if (batch <= 0) { set_error("rtx_progressive_until: batch must be > 0"); return RTX_EINVAL; }
  if (!(target_rel_err >= 0.0)) { set_error("rtx_progressive_until: target_rel_err must be >= 0"); return RTX_EINVAL; }
  noise_stats_head(p, target_rel_err, out);
  out->pixels_above = (int32_t)p->npix;
  const int32_t budget = p->cfg.samples_per_pixel;
  if (p->spp_done >= 2) {
    rtx_status st = progressive_stats(p, target_rel_err, out);
    if (st != RTX_OK || out->pixels_above == 0) return st;
  }
  while (p->spp_done < budget) {
    const int32_t n = budget - p->spp_done < batch ? budget - p->spp_done : batch;
    rtx_status st = progressive_add(p, n, (hipStream_t) nullptr, nullptr);
    if (st != RTX_OK) return st;
    out->spp_done = p->spp_done;
    if (p->spp_done < 2) continue;
    st = progressive_stats(p, target_rel_err, out);
    if (st != RTX_OK || out->pixels_above == 0) return st;
  }
  return RTX_OK;
}

rtx_status rtx_progressive_add_adaptive(rtx_progressive* p, int32_t n_samples, int32_t min_spp, double target_rel_err,
                                        void* hip_stream, RtxRenderStats* stats) {
  if (!progressive_usable(p, "rtx_progressive_add_adaptive")) return RTX_EINVAL;
  if (!n_samples_ok(p, "rtx_progressive_add_adaptive", n_samples)) return RTX_EINVAL;
  if (!adaptive_args_ok(p, "rtx_progressive_add_adaptive", min_spp, target_rel_err)) return RTX_EINVAL;
  rtx_status st = adaptive_init(p);
  if (st == RTX_OK && check_due(p, min_spp)) st = adaptive_retire(p, target_rel_err, (hipStream_t)hip_stream);
  if (st != RTX_OK) return st;
  return progressive_add(p, n_samples, (hipStream_t)hip_stream, stats);
}

rtx_status rtx_progressive_until_adaptive(rtx_progressive* p, int32_t batch, int32_t min_spp, double target_rel_err,
                                          RtxAdaptiveStats* out) {
  if (!progressive_usable(p, "rtx_progressive_until_adaptive")) return RTX_EINVAL;
  if (!out) { set_error("rtx_progressive_until_adaptive: NULL out"); return RTX_EINVAL; }
  if (batch <= 0) { set_error("rtx_progressive_until_adaptive: batch must be > 0"); return RTX_EINVAL; }
  if (!adaptive_args_ok(p, "rtx_progressive_until_adaptive", min_spp, target_rel_err)) return RTX_EINVAL;
  HIP_TRY(hipDeviceSynchronize());  // earlier rounds may have run on the caller's stream; this loop runs on the default one
  rtx_status st = adaptive_init(p);
  if (st != RTX_OK) return st;
  const int32_t budget = p->cfg.samples_per_pixel;
  for (;;) {
    if (check_due(p, min_spp)) {  // every batch boundary, and the budget's
      st = adaptive_retire(p, target_rel_err, (hipStream_t) nullptr);
      if (st != RTX_OK) return st;
    }
    if (p->n_active == 0 || p->spp_done >= budget) break;
    const int32_t n = budget - p->spp_done < batch ? budget - p->spp_done : batch;
    st = progressive_add(p, n, (hipStream_t) nullptr, nullptr);
    if (st != RTX_OK) return st;
  }
  return adaptive_stats(p, min_spp, target_rel_err, out);
}

rtx_status rtx_progressive_pixel_spp(const rtx_progressive* p, int32_t* spp) {
  if (!progressive_usable(p, "rtx_progressive_pixel_spp")) return RTX_EINVAL;
  if (!spp) { set_error("rtx_progressive_pixel_spp: NULL out"); return RTX_EINVAL; }
  if (p->adaptive && p->npix_all) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(spp, p->counts, (size_t)p->npix_all * 4, hipMemcpyDeviceToHost));
  } else {
    memset(spp, 0, (size_t)p->npix_all * 4);
  }
  for (uint32_t lp = 0; lp < p->npix; ++lp)
    if (spp[lp] == 0) spp[lp] = p->spp_done;  // still active
  return RTX_OK;
}

rtx_status rtx_device_retire(const double* S, const double* Q, uint32_t npix, const uint32_t* active, uint32_t n,
                             uint32_t spp, double target, int32_t* counts, uint32_t* next, uint32_t* kept) {
  const char* fn = "rtx_device_retire";
  if (!self_test_args_ok(fn, S && Q && active && counts && next && kept, npix, spp, target)) return RTX_EINVAL;
  *kept = 0;
  if (n == 0 || npix == 0) return RTX_OK;
  for (uint32_t k = 0; k < n; ++k)
    if (active[k] >= npix || (k && active[k] <= active[k - 1])) {
      set_error(std::string(fn) + ": active must ascend strictly and stay below npix");
      return RTX_EINVAL;
    }
  DeviceBuffer<double> dS, dQ;
  DeviceBuffer<uint32_t> d_active, d_next;
  DeviceBuffer<int32_t> d_counts;
  RetireScratch scratch;
  const size_t plane = (size_t)npix * 3;
  HIP_TRY(dS.upload(S, plane, SELF_TEST_SPARE));
  HIP_TRY(dQ.upload(Q, plane, SELF_TEST_SPARE));
  HIP_TRY(d_active.upload(active, n, SELF_TEST_SPARE));
  HIP_TRY(d_counts.upload(counts, npix, SELF_TEST_SPARE));
  HIP_TRY(d_next.alloc((size_t)n * 4 + SELF_TEST_SPARE));
  HIP_TRY(retire_scratch_alloc(n, &scratch));
  uint32_t got = 0;
  const rtx_status st = retire_launch(dS, dQ, d_active, n, spp, target, d_counts, scratch, d_next, (hipStream_t) nullptr, &got);
  if (st != RTX_OK) return st;
  if (got) HIP_TRY(hipMemcpy(next, d_next, (size_t)got * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(counts, d_counts, (size_t)npix * 4, hipMemcpyDeviceToHost));
  *kept = got;
  return RTX_OK;
}

rtx_status rtx_device_noise_reduce(const double* S, const double* Q, const int32_t* counts, uint32_t npix, uint32_t spp,
                                   double target, double* max_r, double* sum_r, uint64_t* above) {
  const char* fn = "rtx_device_noise_reduce";
  if (!self_test_args_ok(fn, S && Q && max_r && sum_r && above, npix, spp, target)) return RTX_EINVAL;
  *max_r = 0.0;
  *sum_r = 0.0;
  *above = 0;
  if (npix == 0) return RTX_OK;
  DeviceBuffer<double> dS, dQ;
  DeviceBuffer<int32_t> d_counts;
  DeviceBuffer<NoisePartial> partials;
  const size_t plane = (size_t)npix * 3;
  HIP_TRY(dS.upload(S, plane, SELF_TEST_SPARE));
  HIP_TRY(dQ.upload(Q, plane, SELF_TEST_SPARE));
  if (counts) HIP_TRY(d_counts.upload(counts, npix, SELF_TEST_SPARE));
  HIP_TRY(noise_partials_alloc(npix, &partials));
  NoisePartial r;
  const rtx_status st = noise_reduce_launch(dS, dQ, d_counts, npix, spp, target, partials, &r);
  if (st != RTX_OK) return st;
  *max_r = r.max_r;
  *sum_r = r.sum_r;
  *above = r.above;
  return RTX_OK;
}

rtx_status rtx_progressive_features(rtx_progressive* p, int32_t feature_spp, float* albedo_rgb, float* normal_xyz) {
  const char* fn = "rtx_progressive_features";
  if (!progressive_usable(p, fn)) return RTX_EINVAL;
  if (feature_spp < 1 || feature_spp > 64) { set_error(std::string(fn) + ": feature_spp must be in [1, 64]"); return RTX_EINVAL; }
  if (!denoise_supported(p, fn)) return RTX_EUNSUPPORTED;
  const rtx_status st = ensure_features(p, feature_spp);
  if (st != RTX_OK) return st;
  if (albedo_rgb && download_xyz(p->albedo, p->npix_all, albedo_rgb) != RTX_OK) return RTX_EHIP;
  if (normal_xyz && download_xyz(p->normal, p->npix_all, normal_xyz) != RTX_OK) return RTX_EHIP;
  return RTX_OK;
}

rtx_status rtx_progressive_denoise(rtx_progressive* p, const RtxDenoiseParams* params, double* mean_rgb, uint8_t* rgb8) {
  const char* fn = "rtx_progressive_denoise";
  if (!progressive_usable(p, fn)) return RTX_EINVAL;
  DenoiseRule r;
  int32_t feature_spp = 0;
  if (!denoise_rule(params, fn, &r, &feature_spp)) return RTX_EINVAL;
  if (!denoise_supported(p, fn)) return RTX_EUNSUPPORTED;
  if (p->spp_done < 2) { set_error(std::string(fn) + ": the variance needs at least 2 samples"); return RTX_EINVAL; }
  rtx_status st = ensure_features(p, feature_spp);
  if (st != RTX_OK) return st;
  if (!p->denoise.rgb8) {  // all five buffers or none: rgb8 is the last one allocated
    DenoiseBuffers b;
    const hipError_t e = denoise_buffers_alloc(p->npix_all, &b);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      set_error(std::string(fn) + ": " + hipGetErrorString(e));
      return e == hipErrorOutOfMemory ? RTX_ENOMEM : RTX_EHIP;
    }
    p->denoise = std::move(b);
  }
  const int32_t w = p->cfg.image_width, h = (int32_t)(p->npix_all / (uint32_t)w);
  HIP_TRY(hipDeviceSynchronize());  // the adds ran on the caller's stream: S, Q and the counts must be complete
  st = denoise_launch(w, h, r, p->S, p->Q, any_retired(p) ? p->counts : nullptr, (uint32_t)p->spp_done, 1, p->albedo,
                      p->normal, p->denoise, mean_rgb != nullptr, rgb8 != nullptr);
  if (st != RTX_OK) return st;
  if (mean_rgb) HIP_TRY(hipMemcpy(mean_rgb, p->denoise.mean, (size_t)p->npix_all * 24, hipMemcpyDeviceToHost));
  if (rgb8) HIP_TRY(hipMemcpy(rgb8, p->denoise.rgb8, (size_t)p->npix_all * 3, hipMemcpyDeviceToHost));
  return RTX_OK;
}

rtx_status rtx_device_denoise(const double* mean_rgb, const double* var_rgb, const float* albedo_rgb, const float* normal_xyz,
                              int32_t width, int32_t height, const RtxDenoiseParams* params, double* out_mean_rgb,
                              uint8_t* out_rgb8) {
  const char* fn = "rtx_device_denoise";
  if (!mean_rgb || !var_rgb || !albedo_rgb || !normal_xyz) { set_error(std::string(fn) + ": NULL argument"); return RTX_EINVAL; }
  if (width < 1 || height < 1 || (uint64_t)width * (uint64_t)height >= (1ull << 31)) {
    set_error(std::string(fn) + ": width and height must be >= 1, with fewer than 2^31 pixels");
    return RTX_EINVAL;
  }
  DenoiseRule r;
  if (!denoise_rule(params, fn, &r, nullptr)) return RTX_EINVAL;
  const size_t npix = (size_t)width * (size_t)height;
  std::vector<float4> a4(npix), n4(npix);
  for (size_t k = 0; k < npix; ++k) {
    a4[k] = make_float4(albedo_rgb[3 * k], albedo_rgb[3 * k + 1], albedo_rgb[3 * k + 2], 0.f);
    n4[k] = make_float4(normal_xyz[3 * k], normal_xyz[3 * k + 1], normal_xyz[3 * k + 2], 0.f);
  }
  DeviceBuffer<double> dm, dv;
  DeviceBuffer<float4> da, dn;
  DenoiseBuffers b;
  HIP_TRY(dm.upload(mean_rgb, npix * 3, SELF_TEST_SPARE));
  HIP_TRY(dv.upload(var_rgb, npix * 3, SELF_TEST_SPARE));
  HIP_TRY(da.upload(a4.data(), npix, SELF_TEST_SPARE));
  HIP_TRY(dn.upload(n4.data(), npix, SELF_TEST_SPARE));
  HIP_TRY(denoise_buffers_alloc(npix, &b));
  const rtx_status st = denoise_launch(width, height, r, dm, dv, nullptr, 0u, 0, da, dn, b, out_mean_rgb != nullptr,
                                       out_rgb8 != nullptr);
  if (st != RTX_OK) return st;
  if (out_mean_rgb) HIP_TRY(hipMemcpy(out_mean_rgb, b.mean, npix * 24, hipMemcpyDeviceToHost));
  if (out_rgb8) HIP_TRY(hipMemcpy(out_rgb8, b.rgb8, npix * 3, hipMemcpyDeviceToHost));
  return RTX_OK;
}

}  // extern "C"
