// Progressive rendering (rtx_progressive_*, included by render.hip's f64 compilation after the C ABI).
//
// A handle keeps one (scene, camera, config, shard)'s accumulators S (sum of radiances) and Q (sum of their squares) in
// device memory across calls.  rtx_progressive_add(n) traces the absolute samples [spp_done, spp_done + n) of every pixel
// through render_impl (SampleRange: same passes, pipelining and kernel choice as a one-shot render) and adds them onto S and
// Q in sample order.  Since every path's random stream is keyed by its absolute (pixel, sample) index, the frame after k
// samples -- however they were split across calls -- is bit-identical to a one-shot render at k spp.
//
// The handle borrows the scene's render workspace (sample buffer, work counters, pipelining stream): it must not run at the
// same time as another render of the same scene on another stream, and it must be destroyed before its scene.

struct rtx_progressive {
  const rtx_scene* scene;
  RtxCamera cam;
  RtxConfig cfg;
  RtxShard shard;
  int device;
  uint32_t npix_all;  // pixels of the shard
  uint32_t npix;      // of which active (row_chunk_compat leaves the rest zero)
  int32_t spp_done;
  bool broken;        // a failed add left S / Q partly updated
  double* S;
  double* Q;
  NoisePartial* partials;  // one per 256 active pixels, then the final result
  uint32_t n_partials;
};

namespace {

void progressive_free(rtx_progressive* p) {
  if (p->S) (void)hipFree(p->S);
  if (p->Q) (void)hipFree(p->Q);
  if (p->partials) (void)hipFree(p->partials);
  delete p;
}

rtx_status progressive_add(rtx_progressive* p, int32_t n_samples, hipStream_t stream, RtxRenderStats* stats) {
  const SampleRange range = {(uint32_t)p->spp_done, (uint32_t)n_samples, p->spp_done > 0 ? 1 : 0, p->Q};
  rtx_status st;
  if (p->scene->f32)
    st = rtx_f32_render_range(p->scene->device_scene, &p->cam, &p->cfg, &p->shard, p->S, p->Q, range.first, range.count,
                              range.cont, (void*)stream, stats);
  else
    st = render_impl<false>(scene_device(p->scene), &p->cam, &p->cfg, &p->shard, p->S, nullptr, stream, stats, &range);
  if (st != RTX_OK) { p->broken = true; return st; }
  p->spp_done += n_samples;
  return RTX_OK;
}

rtx_status progressive_stats(rtx_progressive* p, double target, RtxNoiseStats* out) {
  memset(out, 0, sizeof(*out));
  out->spp_done = p->spp_done;
  out->pixels = (int32_t)p->npix;
  out->target_rel_err = target;
  if (p->npix == 0) return RTX_OK;
  HIP_TRY(hipDeviceSynchronize());  // the adds ran on the caller's stream
  hipLaunchKernelGGL(k_noise_stats, dim3(p->n_partials), dim3(256), 0, (hipStream_t) nullptr, p->S, p->Q, p->npix,
                     (uint32_t)p->spp_done, target, p->partials);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_noise_stats_final, dim3(1), dim3(256), 0, (hipStream_t) nullptr, p->partials, p->n_partials,
                     p->partials + p->n_partials);
  HIP_TRY(hipGetLastError());
  NoisePartial r;
  HIP_TRY(hipMemcpy(&r, p->partials + p->n_partials, sizeof(r), hipMemcpyDeviceToHost));
  out->pixels_above = (int32_t)r.above;
  out->max_rel_err = r.max_r;
  out->mean_rel_err = r.sum_r / (double)p->npix;
  return RTX_OK;
}

bool progressive_usable(const rtx_progressive* p, const char* fn) {
  if (!p) { set_error(std::string(fn) + ": NULL handle"); return false; }
  if (p->broken) { set_error(std::string(fn) + ": an earlier rtx_progressive_add failed; the accumulators are incomplete"); return false; }
  return true;
}

}  // namespace

extern "C" {

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
  p->n_partials = (uint32_t)((npix + 255) / 256);
  hipError_t e = hipGetDevice(&p->device);
  const size_t plane = (size_t)npix_all * 24;
  if (e == hipSuccess && plane) e = hipMalloc((void**)&p->S, plane);
  if (e == hipSuccess && plane) e = hipMalloc((void**)&p->Q, plane);
  if (e == hipSuccess) e = hipMalloc((void**)&p->partials, (p->n_partials + 1) * sizeof(NoisePartial));
  if (e == hipSuccess && plane) e = hipMemset(p->S, 0, plane);  // rows beyond row_chunk_compat's limit stay zero
  if (e == hipSuccess && plane) e = hipMemset(p->Q, 0, plane);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error(std::string("rtx_progressive_create: ") + hipGetErrorString(e));
    progressive_free(p);
    return e == hipErrorOutOfMemory ? RTX_ENOMEM : RTX_EHIP;
  }
  *out = p;
  return RTX_OK;
}

void rtx_progressive_destroy(rtx_progressive* p) {
  if (!p) return;
  (void)hipDeviceSynchronize();  // an add may still be running on the caller's stream
  progressive_free(p);
}

int32_t rtx_progressive_spp(const rtx_progressive* p) { return p ? p->spp_done : -1; }

rtx_status rtx_progressive_add(rtx_progressive* p, int32_t n_samples, void* hip_stream, RtxRenderStats* stats) {
  if (!progressive_usable(p, "rtx_progressive_add")) return RTX_EINVAL;
  if (n_samples <= 0 || n_samples > p->cfg.samples_per_pixel - p->spp_done) {
    set_error("rtx_progressive_add: n_samples must be in [1, samples_per_pixel - spp_done] = [1, " +
              std::to_string(p->cfg.samples_per_pixel - p->spp_done) + "]");
    return RTX_EINVAL;
  }
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
    uint8_t* d_rgb = nullptr;
    HIP_TRY(hipMalloc((void**)&d_rgb, (size_t)p->npix_all * 3));
    rtx_status st = RTX_OK;
    hipError_t e = hipMemset(d_rgb, 0, (size_t)p->npix_all * 3);
    if (e == hipSuccess) {
      st = p->scene->f32 ? rtx_f32_tonemap(p->S, d_rgb, p->npix, (uint32_t)p->spp_done, nullptr)
                         : tonemap_impl(p->S, d_rgb, p->npix, (uint32_t)p->spp_done, (hipStream_t) nullptr);
      if (st == RTX_OK) e = hipMemcpy(out->rgb8, d_rgb, (size_t)p->npix_all * 3, hipMemcpyDeviceToHost);
    }
    (void)hipFree(d_rgb);
    if (st != RTX_OK) return st;
    if (e != hipSuccess) { set_error(std::string("rtx_progressive_read: ") + hipGetErrorString(e)); return RTX_EHIP; }
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
  if (!progressive_usable(p, "rtx_progressive_until")) return RTX_EINVAL;
  if (!out) { set_error("rtx_progressive_until: NULL out"); return RTX_EINVAL; }
  if (batch <= 0) { set_error("rtx_progressive_until: batch must be > 0"); return RTX_EINVAL; }
  if (!(target_rel_err >= 0.0)) { set_error("rtx_progressive_until: target_rel_err must be >= 0"); return RTX_EINVAL; }
  memset(out, 0, sizeof(*out));
  out->spp_done = p->spp_done;
  out->pixels = (int32_t)p->npix;
  out->target_rel_err = target_rel_err;
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

}  // extern "C"
