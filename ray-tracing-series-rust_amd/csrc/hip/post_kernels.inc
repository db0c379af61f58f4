// Ordered sample reduction, tone map and the device self-test kernels (included by render.hip, namespace rtx).


// One lane per pixel; samples of the pass are added in ascending sample index.
__global__ __launch_bounds__(256) void k_reduce_samples(const double* __restrict__ samples,
                                                        double* __restrict__ accum, uint32_t npix,
                                                        uint32_t s_count, int first_pass) {
  uint32_t lp = blockIdx.x * 256u + threadIdx.x;
  if (lp >= npix) return;
  double r = 0.0, g = 0.0, b = 0.0;  // world.rs:1210: Vec3::new(0, 0, 0)
  if (!first_pass) { r = accum[3 * (size_t)lp]; g = accum[3 * (size_t)lp + 1]; b = accum[3 * (size_t)lp + 2]; }
  for (uint32_t s = 0; s < s_count; ++s) {
    const double* p = samples + 3 * ((size_t)s * npix + lp);
    r += p[0]; g += p[1]; b += p[2];  // world.rs:1215 (vec3.rs:223-229 AddAssign)
  }
  accum[3 * (size_t)lp] = r; accum[3 * (size_t)lp + 1] = g; accum[3 * (size_t)lp + 2] = b;
}

// k_reduce_samples that also keeps the per-pixel, per-channel sum of squares Q += x*x (progressive rendering,
// progressive.inc).  S gets exactly k_reduce_samples' adds; the square and its add are separately rounded, so a host
// restatement of the same in-order loop is bit-equal.
__global__ __launch_bounds__(256) void k_reduce_samples_moments(const double* __restrict__ samples,
                                                                double* __restrict__ accum, double* __restrict__ sumsq,
                                                                uint32_t npix, uint32_t s_count, int first_pass) {
#pragma clang fp contract(off)
  uint32_t lp = blockIdx.x * 256u + threadIdx.x;
  if (lp >= npix) return;
  double r = 0.0, g = 0.0, b = 0.0, qr = 0.0, qg = 0.0, qb = 0.0;
  if (!first_pass) {
    r = accum[3 * (size_t)lp]; g = accum[3 * (size_t)lp + 1]; b = accum[3 * (size_t)lp + 2];
    qr = sumsq[3 * (size_t)lp]; qg = sumsq[3 * (size_t)lp + 1]; qb = sumsq[3 * (size_t)lp + 2];
  }
  for (uint32_t s = 0; s < s_count; ++s) {
    const double* p = samples + 3 * ((size_t)s * npix + lp);
    const double x0 = p[0], x1 = p[1], x2 = p[2];
    r += x0; g += x1; b += x2;
    qr = __dadd_rn(qr, __dmul_rn(x0, x0));
    qg = __dadd_rn(qg, __dmul_rn(x1, x1));
    qb = __dadd_rn(qb, __dmul_rn(x2, x2));
  }
  accum[3 * (size_t)lp] = r; accum[3 * (size_t)lp + 1] = g; accum[3 * (size_t)lp + 2] = b;
  sumsq[3 * (size_t)lp] = qr; sumsq[3 * (size_t)lp + 1] = qg; sumsq[3 * (size_t)lp + 2] = qb;
}

// k_reduce_samples_moments for an adaptive pass (pass_items.inc): the pass's items are the pixels of the active list, so lane
// k adds its samples onto local pixel active[k]'s S and Q with the same in-order, non-contracted arithmetic.  Adaptive passes
// always continue sums already there (a pixel can retire only after 2 samples, progressive.inc).
__global__ __launch_bounds__(256) void k_reduce_samples_moments_active(const double* __restrict__ samples,
                                                                       double* __restrict__ accum, double* __restrict__ sumsq,
                                                                       const uint32_t* __restrict__ active, uint32_t n_active,
                                                                       uint32_t s_count) {
#pragma clang fp contract(off)
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n_active) return;
  const size_t lp = active[k];
  double r = accum[3 * lp], g = accum[3 * lp + 1], b = accum[3 * lp + 2];
  double qr = sumsq[3 * lp], qg = sumsq[3 * lp + 1], qb = sumsq[3 * lp + 2];
  for (uint32_t s = 0; s < s_count; ++s) {
    const double* p = samples + 3 * ((size_t)s * n_active + k);
    const double x0 = p[0], x1 = p[1], x2 = p[2];
    r += x0; g += x1; b += x2;
    qr = __dadd_rn(qr, __dmul_rn(x0, x0));
    qg = __dadd_rn(qg, __dmul_rn(x1, x1));
    qb = __dadd_rn(qb, __dmul_rn(x2, x2));
  }
  accum[3 * lp] = r; accum[3 * lp + 1] = g; accum[3 * lp + 2] = b;
  sumsq[3 * lp] = qr; sumsq[3 * lp + 1] = qg; sumsq[3 * lp + 2] = qb;
}

// Noise estimate of a progressive frame after n >= 2 samples, per pixel and channel:
//   m = S/n,  var = max(0, (Q - S*S/n) / (n - 1)),  se = sqrt(var / n),  r_c = se / (m + 1/256)
// and the pixel's error r = max_c r_c.  Every operation is correctly rounded and none is contracted, so r equals a
// numpy restatement bit for bit.  Reduced over the active pixels to (max r, sum r, count r > target) in a fixed order:
//   stage 1 (k_noise_stats): one partial per 256-pixel block -- xor-shuffle butterfly inside each wave64, then wave 0
//            combines the block's four waves from LDS in wave order;
//   stage 2 (k_noise_stats_final): one block folds the partials -- thread t takes partials t, t + 256, ... in
//            ascending order, then the same wave / LDS tree.
// No atomics: the result depends on npix alone, never on scheduling.
struct NoisePartial {
  double max_r, sum_r;
  unsigned long long above;
};

__device__ __forceinline__ double pixel_rel_err(const double* __restrict__ S, const double* __restrict__ Q, size_t lp,
                                                double n) {
#pragma clang fp contract(off)
  double r = 0.0;
  for (int c = 0; c < 3; ++c) {
    const double s = S[3 * lp + c], q = Q[3 * lp + c];
    const double m = __ddiv_rn(s, n);
    double var = __ddiv_rn(__dsub_rn(q, __ddiv_rn(__dmul_rn(s, s), n)), __dsub_rn(n, 1.0));
    var = var > 0.0 ? var : 0.0;
    const double se = __dsqrt_rn(__ddiv_rn(var, n));
    const double rc = __ddiv_rn(se, __dadd_rn(m, 1.0 / 256.0));
    r = rc > r ? rc : r;  // a NaN rc is ignored
  }
  return r;
}

// Block-wide (256 lanes, four waves) reduction in a fixed pattern; the result is valid in thread 0.
__device__ __forceinline__ NoisePartial noise_block_reduce(NoisePartial v) {
  for (int off = 32; off >= 1; off >>= 1) {
    const double om = __shfl_xor(v.max_r, off, 64);
    const double os = __shfl_xor(v.sum_r, off, 64);
    const unsigned long long oa = __shfl_xor(v.above, off, 64);
    v.max_r = om > v.max_r ? om : v.max_r;
    v.sum_r = v.sum_r + os;
    v.above += oa;
  }
  __shared__ NoisePartial wave_part[4];
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) wave_part[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    v = wave_part[0];
    for (int k = 1; k < 4; ++k) {
      v.max_r = wave_part[k].max_r > v.max_r ? wave_part[k].max_r : v.max_r;
      v.sum_r = v.sum_r + wave_part[k].sum_r;
      v.above += wave_part[k].above;
    }
  }
  return v;
}

__global__ __launch_bounds__(256) void k_noise_stats(const double* __restrict__ S, const double* __restrict__ Q,
                                                     uint32_t npix, uint32_t spp, double target,
                                                     NoisePartial* __restrict__ partials) {
  const uint32_t lp = blockIdx.x * 256u + threadIdx.x;
  NoisePartial v = {0.0, 0.0, 0ull};
  if (lp < npix) {
    const double r = pixel_rel_err(S, Q, lp, (double)spp);
    v.max_r = r;
    v.sum_r = r;
    v.above = r > target ? 1ull : 0ull;
  }
  v = noise_block_reduce(v);
  if (threadIdx.x == 0) partials[blockIdx.x] = v;
}

__global__ __launch_bounds__(256) void k_noise_stats_final(const NoisePartial* __restrict__ partials, uint32_t n_partials,
                                                           NoisePartial* __restrict__ out) {
  NoisePartial v = {0.0, 0.0, 0ull};
  for (uint32_t k = threadIdx.x; k < n_partials; k += 256u) {
    const NoisePartial p = partials[k];
    v.max_r = p.max_r > v.max_r ? p.max_r : v.max_r;
    v.sum_r = v.sum_r + p.sum_r;
    v.above += p.above;
  }
  v = noise_block_reduce(v);
  if (threadIdx.x == 0) *out = v;
}

// k_noise_stats for a frame whose pixels hold different sample counts (adaptive progressive rendering): pixel lp's n is
// counts[lp], or spp where counts[lp] == 0 (a pixel still active).  The same pixel_rel_err and the same reduction tree.
__global__ __launch_bounds__(256) void k_noise_stats_counts(const double* __restrict__ S, const double* __restrict__ Q,
                                                            const int32_t* __restrict__ counts, uint32_t npix, uint32_t spp,
                                                            double target, NoisePartial* __restrict__ partials) {
  const uint32_t lp = blockIdx.x * 256u + threadIdx.x;
  NoisePartial v = {0.0, 0.0, 0ull};
  if (lp < npix) {
    const int32_t c = counts[lp];
    const double r = pixel_rel_err(S, Q, lp, (double)(c != 0 ? (uint32_t)c : spp));
    v.max_r = r;
    v.sum_r = r;
    v.above = r > target ? 1ull : 0ull;
  }
  v = noise_block_reduce(v);
  if (threadIdx.x == 0) partials[blockIdx.x] = v;
}

// Adaptive retirement (progressive.inc) over the n pixels of the ascending active list, in three launches:
//   k_retire_flag:    lane k computes pixel active[k]'s r at n = spp; the pixel retires when r <= target (counts[lp] = spp,
//                     its sample count from now on).  Each wave's ballot of the survivors goes to keep_mask[k / 64], the
//                     block's survivor count to block_count[blockIdx.x].
//   k_retire_scan:    one block turns the block counts into exclusive offsets, block_offset[n_blocks] = the survivors.
//   k_retire_scatter: a survivor's slot in the next list is its block's offset + the survivors of the block's earlier waves
//                     (scanned through LDS) + those of the lower lanes of its wave (mbcnt on the ballot).
// A stable compaction: the next list is ascending again, and it depends on the data alone, never on scheduling.
__global__ __launch_bounds__(256) void k_retire_flag(const double* __restrict__ S, const double* __restrict__ Q,
                                                     const uint32_t* __restrict__ active, uint32_t n, uint32_t spp,
                                                     double target, int32_t* __restrict__ counts,
                                                     unsigned long long* __restrict__ keep_mask,
                                                     uint32_t* __restrict__ block_count) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  bool keep = false;
  if (k < n) {
    const uint32_t lp = active[k];
    const double r = pixel_rel_err(S, Q, lp, (double)spp);
    keep = !(r <= target);  // (r is never NaN: pixel_rel_err ignores a NaN channel, so an all-NaN pixel has r = 0)
    if (!keep) counts[lp] = (int32_t)spp;
  }
  const unsigned long long m = __ballot(keep);
  __shared__ uint32_t wave_n[4];
  if ((threadIdx.x & 63u) == 0) {
    keep_mask[k >> 6] = m;
    wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) block_count[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

__global__ __launch_bounds__(256) void k_retire_scan(const uint32_t* __restrict__ block_count, uint32_t n_blocks,
                                                     uint32_t* __restrict__ block_offset) {
  // thread t owns the contiguous blocks [t * per, (t + 1) * per): its sum, an exclusive scan of the 256 sums, then its offsets
  const uint32_t per = (n_blocks + 255u) / 256u, lo = threadIdx.x * per;
  const uint32_t hi = lo + per < n_blocks ? lo + per : n_blocks;
  uint32_t sum = 0;
  for (uint32_t b = lo; b < hi; ++b) sum += block_count[b];
  __shared__ uint32_t part[256];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int t = 0; t < 256; ++t) { const uint32_t c = part[t]; part[t] = run; run += c; }
    block_offset[n_blocks] = run;
  }
  __syncthreads();
  uint32_t run = part[threadIdx.x];
  for (uint32_t b = lo; b < hi; ++b) { block_offset[b] = run; run += block_count[b]; }
}

__global__ __launch_bounds__(256) void k_retire_scatter(const uint32_t* __restrict__ active, uint32_t n,
                                                        const unsigned long long* __restrict__ keep_mask,
                                                        const uint32_t* __restrict__ block_offset,
                                                        uint32_t* __restrict__ next) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  __shared__ uint32_t wave_base[4];
  if (threadIdx.x == 0) {
    uint32_t b = block_offset[blockIdx.x];
    for (int w = 0; w < 4; ++w) { wave_base[w] = b; b += (uint32_t)__popcll(keep_mask[4 * blockIdx.x + w]); }
  }
  __syncthreads();
  if (k >= n) return;
  const unsigned long long m = keep_mask[k >> 6];
  if (!((m >> (threadIdx.x & 63u)) & 1ull)) return;
  const uint32_t rank = lane_rank(m);
  next[wave_base[threadIdx.x >> 6] + rank] = active[k];
}

__global__ __launch_bounds__(256) void k_iota(uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k < n) out[k] = k;
}

__global__ __launch_bounds__(256) void k_tonemap(const double* __restrict__ accum,
                                                 uint8_t* __restrict__ rgb8, uint32_t npix,
                                                 uint32_t spp) {
  uint32_t lp = blockIdx.x * 256u + threadIdx.x;
  if (lp >= npix) return;
  int32_t c[3];
  rt::tone_map(rt::v3(accum[3 * (size_t)lp], accum[3 * (size_t)lp + 1], accum[3 * (size_t)lp + 2]), spp, c);
  rgb8[3 * (size_t)lp] = (uint8_t)c[0];
  rgb8[3 * (size_t)lp + 1] = (uint8_t)c[1];
  rgb8[3 * (size_t)lp + 2] = (uint8_t)c[2];
}

// k_tonemap for a frame whose pixels hold different sample counts: pixel lp's is counts[lp], or spp where that is 0.
__global__ __launch_bounds__(256) void k_tonemap_counts(const double* __restrict__ accum, uint8_t* __restrict__ rgb8,
                                                        const int32_t* __restrict__ counts, uint32_t npix, uint32_t spp) {
  uint32_t lp = blockIdx.x * 256u + threadIdx.x;
  if (lp >= npix) return;
  const int32_t n = counts[lp];
  int32_t c[3];
  rt::tone_map(rt::v3(accum[3 * (size_t)lp], accum[3 * (size_t)lp + 1], accum[3 * (size_t)lp + 2]), n != 0 ? (uint32_t)n : spp, c);
  rgb8[3 * (size_t)lp] = (uint8_t)c[0];
  rgb8[3 * (size_t)lp + 1] = (uint8_t)c[1];
  rgb8[3 * (size_t)lp + 2] = (uint8_t)c[2];
}

// Device self-test kernels (rtx_device_math / rtx_device_stream; rtx_device_retire and rtx_device_noise_reduce run the
// kernels above through progressive.inc's launch helpers).
__global__ void k_device_math(int fn, const double* x, const double* y, long long n, double* out) {
  long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  double a = x[k], b = y[k], r;
  switch (fn) {
    case 0: r = rt::rt_sin(a); break;
    case 1: r = rt::rt_cos(a); break;
    case 2: r = rt::rt_log(a); break;
    case 3: r = rt::rt_acos(a); break;
    case 4: r = rt::rt_atan2(a, b); break;
    case 5: r = rt::rt_tan(a); break;
    case 6: r = rt::rt_sqrt(a); break;
    case 7: r = a / b; break;
    case 8: r = a * b + a; break;
    case 10: r = (double)wide_key((float)a, (float)b); break;  // the clamp walk_node_step4 sorts children by (NaN -> t_min, +inf -> finite)
    default: r = rt::rt_floor(a); break;
  }
  out[k] = r;
}
#ifdef RTX_F32_TU
// rtx_device_math's float entries (fn >= 32): the building blocks as THIS compilation evaluates them -- the five platform
// functions behind rt_sin ..., the correctly rounded sqrt and division, and the three float RNG forms fed one raw 64-bit
// draw (the bits of x[k]; for rng_range the bits of y[k] hold lo (low word) and hi (high word) as floats).  The float result
// is handed back widened, which is exact.
__global__ void k_device_math_f32(int fn, const double* x, const double* y, long long n, double* out) {
  long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const float a = (float)x[k], b = (float)y[k];
  const uint64_t raw = rt::f64_bits(x[k]), yb = rt::f64_bits(y[k]);
  rt::Rng g;
  g.s0 = raw; g.s1 = 0;  // rng_next_u64 returns s0 + s1: the next draw IS raw
  union { uint32_t u; float f; } lo, hi;
  lo.u = (uint32_t)yb; hi.u = (uint32_t)(yb >> 32);
  float r;
  switch (fn) {
    case 32: r = rt::rt_sin(a); break;
    case 33: r = rt::rt_cos(a); break;
    case 34: r = rt::rt_log(a); break;
    case 35: r = rt::rt_acos(a); break;
    case 36: r = rt::rt_atan2(a, b); break;
    case 37: r = rt::rt_sqrt(a); break;
    case 38: r = a / b; break;
    case 39: r = (float)rt::rt_sin_sign(a); break;
    case 40: r = rt::rng_f64(g); break;
    case 41: r = rt::rng_range(g, lo.f, hi.f); break;
    case 43: r = rt::make_ray32(rt::make_ray(rt::v3(0, 0, 0), rt::v3(a, 1, 1), 0), rt::real(0.001)).ix; break;  // the slope cap (v_med3_f32) on 1 / a
    case 42: r = rt::rng_range_pm1(g); break;
    default: r = 0.0f; break;
  }
  out[k] = (double)r;
}
#endif
__global__ void k_device_stream(unsigned long long seed, unsigned long long pixel, unsigned int sample, int n, double* out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  rt::Rng g = rt::rng_for_sample(seed, pixel, sample);
  for (int k = 0; k < n; ++k) out[k] = rt::rng_f64(g);
}

