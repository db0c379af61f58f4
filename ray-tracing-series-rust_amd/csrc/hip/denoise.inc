// Denoising a progressive frame (included by render.hip, namespace rtx; progressive.inc drives it).
//
// Two parts, both new outputs next to S and Q; nothing here writes S, Q, the counts or a trace kernel's buffers:
//
// 1. Feature pass (k_features, both compilations).  One thread per pixel, grid-stride.  For each feature sample s in
//    [0, feature_spp) it begins path sample s exactly as a trace kernel does (rt::path_begin: the same jitter, lens sample
//    and shutter time) and makes that path's first rt::world_hit call on the same stream (so a medium's distance draw matches
//    the path's first hit).  It averages, in registers, what the ray hit:
//      albedo  Lambertian / Isotropic: the texture value scatter would attenuate by; Metal: its albedo; Dielectric and
//              DiffuseLight: (1, 1, 1); a miss: the background;
//      normal  rec.normal (face-forwarded, as the hit record holds it); (0, 0, 0) for an Isotropic hit and for a miss.
//    Output: one float4 per pixel for each (w = 0), in the shard layout.  No atomics.
//
// 2. The filter (f64 compilation only): an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) steered by the
//    per-pixel variance of the mean, as in the spatial part of SVGF (Schied et al. 2017).
//      k_denoise_prepare   f64 in, f32 out, per pixel p at its own count n:  m = S/n, v_c = max(0, (Q - S*S/n)/(n - 1))/n
//                          (pixel_rel_err's operations, in its order), or m and v as given (the self-test entry); with
//                          demodulation a = max(A, 1e-3), c0 = m/a, v_c = v_c/a^2 (in f64, rounded once to f32);
//                          sigma2 = 0.2126^2 v_r + 0.7152^2 v_g + 0.0722^2 v_b (channel covariances are ignored);
//                          n^ = N/|N| if |N| >= 1e-3, else 0.
//      k_denoise_level     one launch per level k, step t = 2^k, f32: taps q = p + t (dx, dy), dx, dy in -2..2 inside the
//                          image, h = (1, 4, 6, 4, 1)/16,
//                            w = h_dx h_dy exp(-|l(c_p) - l(c_q)| / (sigma_l sqrt(sigma2_p) + 1e-4) - |A_p - A_q|^2 / sigma_a^2) W_n
//                          with l the Rec. 709 luminance, W_n = 1 if both n^ are 0, 0 if exactly one is, else
//                          max(0, min(1, n^_p . n^_q))^sigma_n;  c' = sum w c_q / sum w,  sigma2' = sum w^2 sigma2_q / (sum w)^2.
//                          Taps are summed dy outer, dx inner, each ascending; the centre tap's weight is (3/8)^2.
//                          The last level also finishes: mean = c_K a (demodulated) or c_K, to f64 and / or to rgb8
//                          through rt::tone_map(mean, 1).
//    Colour and variance travel together as one float4 (c, sigma2) per pixel, ping-ponged between two buffers; the guides
//    are one float4 each (albedo A; n^ with w = 1 where it is not 0).  A block is 64 x 4 pixels: each wave covers 64
//    consecutive pixels of one row, so every tap row of a wave is one coalesced 1 KiB load per buffer.  Every operation is
//    fixed per pixel (no atomics, no reduction across lanes): the same inputs give the same bits on every call.

// A feature sample's first hit (a world_hit of path sample s; rt::path_begin gives the path's own primary ray).
template <uint32_t F>
__global__ __launch_bounds__(TRACE_BLOCK) void k_features(rt::SceneView sv, rt::RenderParams rp, uint32_t npix,
                                                          uint32_t feature_spp, float4* __restrict__ albedo,
                                                          float4* __restrict__ normal) {
  extern __shared__ int32_t lds_stack[];
  LdsStack stack;
  stack.base = lds_stack + threadIdx.x;
  stack.n = 0;
  const uint32_t w = (uint32_t)rp.image_width;
  for (uint32_t lp = blockIdx.x * TRACE_BLOCK + threadIdx.x; lp < npix; lp += gridDim.x * TRACE_BLOCK) {
    const uint32_t j = lp / w, i = lp - j * w;  // the whole image: local pixel lp is row j from the bottom
    rt::Color a = rt::v3(0, 0, 0);
    rt::Vec3 n = rt::v3(0, 0, 0);
    for (uint32_t s = 0; s < feature_spp; ++s) {
      rt::PathState ps;
      rt::path_begin(rp, i, j, s, &ps);
      rt::HitRecord rec;
      bool hit = false;
      if (!rt::path_bounce_begin(&ps)) {  // (max_depth >= 1: only the f32 mode's non-finite ray ends here)
        stack.reset();
        hit = rt::world_hit<F, false>(sv, ps.ray, rt::ray_t_min(ps.ray), RT_INFINITY, &rec, ps.rng, stack, nullptr);
      }
      if (!hit) {
        a += rp.background;
        continue;
      }
      const rt::FlatMaterial& m = sv.materials[rec.mat];
      if (m.kind == rt::MAT_LAMBERTIAN || m.kind == rt::MAT_ISOTROPIC) a += rt::material_texture_value<F, false>(sv, m, rec, nullptr);
      else if (m.kind == rt::MAT_METAL) a += rt::load_v3(m.albedo);
      else a += rt::v3(1, 1, 1);  // Dielectric, DiffuseLight
      if (m.kind != rt::MAT_ISOTROPIC) n += rec.normal;
    }
    const rt::real inv = rt::real(1.0) / (rt::real)feature_spp;
    albedo[lp] = make_float4((float)(a.x * inv), (float)(a.y * inv), (float)(a.z * inv), 0.f);
    normal[lp] = make_float4((float)(n.x * inv), (float)(n.y * inv), (float)(n.z * inv), 0.f);
  }
}

#if !defined(RTX_F32_TU)
// The filter's parameters, already defaulted and checked (progressive.inc: denoise_rule).
struct DenoiseRule {
  int32_t iterations;  // K levels
  int32_t demodulate;  // 1 on, 0 off
  float sigma_l, sigma_n, inv_sigma_a2;
};

#define DENOISE_BX 64
#define DENOISE_BY 4

// Per pixel: (c0, sigma2) and n^ from m and v (moments = 0) or from S, Q at the pixel's count (moments = 1: counts[lp], or
// spp where counts is NULL or 0).
__global__ __launch_bounds__(256) void k_denoise_prepare(const double* __restrict__ s_or_m, const double* __restrict__ q_or_v,
                                                         const int32_t* __restrict__ counts, uint32_t spp, int moments,
                                                         uint32_t npix, int demodulate, const float4* __restrict__ albedo,
                                                         const float4* __restrict__ normal, float4* __restrict__ cv,
                                                         float4* __restrict__ nhat) {
#pragma clang fp contract(off)
  const uint32_t lp = blockIdx.x * 256u + threadIdx.x;
  if (lp >= npix) return;
  const float4 A = albedo[lp];
  const float Ac[3] = {A.x, A.y, A.z};
  const double lum[3] = {0.2126, 0.7152, 0.0722};
  double n = 0.0;
  if (moments) {
    const int32_t c = counts ? counts[lp] : 0;
    n = (double)(c != 0 ? (uint32_t)c : spp);
  }
  float c0[3];
  double s2 = 0.0;
  for (int c = 0; c < 3; ++c) {
    double m, v;
    if (moments) {  // pixel_rel_err's operations, in its order
      const double s = s_or_m[3 * (size_t)lp + c], q = q_or_v[3 * (size_t)lp + c];
      m = __ddiv_rn(s, n);
      double var = __ddiv_rn(__dsub_rn(q, __ddiv_rn(__dmul_rn(s, s), n)), __dsub_rn(n, 1.0));
      var = var > 0.0 ? var : 0.0;
      v = __ddiv_rn(var, n);
    } else {
      m = s_or_m[3 * (size_t)lp + c];
      v = q_or_v[3 * (size_t)lp + c];
    }
    if (demodulate) {
      const double a = Ac[c] > 1e-3f ? (double)Ac[c] : (double)1e-3f;
      m = m / a;
      v = v / (a * a);
    }
    c0[c] = (float)m;
    s2 = s2 + (lum[c] * lum[c]) * v;
  }
  cv[lp] = make_float4(c0[0], c0[1], c0[2], (float)s2);
  const float4 N = normal[lp];
  const float len = sqrtf(N.x * N.x + N.y * N.y + N.z * N.z);
  nhat[lp] = len >= 1e-3f ? make_float4(N.x / len, N.y / len, N.z / len, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ float denoise_luminance(float4 c) { return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z; }

// One a-trous level at step t over a w x h image; LAST: finish into mean_rgb / rgb8 (each may be NULL) instead of cv_out.
template <bool LAST>
__global__ __launch_bounds__(DENOISE_BX * DENOISE_BY) void k_denoise_level(const float4* __restrict__ cv_in,
                                                                           const float4* __restrict__ albedo,
                                                                           const float4* __restrict__ nhat, int32_t w,
                                                                           int32_t h, int32_t t, uint32_t nbx, DenoiseRule r,
                                                                           float4* __restrict__ cv_out,
                                                                           double* __restrict__ mean_rgb,
                                                                           uint8_t* __restrict__ rgb8) {
#pragma clang fp contract(off)
  const uint32_t by = blockIdx.x / nbx, bx = blockIdx.x - by * nbx;  // a 1-D grid of nbx blocks per band of DENOISE_BY rows
  const int32_t x = (int32_t)(bx * DENOISE_BX + threadIdx.x), y = (int32_t)(by * DENOISE_BY + threadIdx.y);
  if (x >= w || y >= h) return;
  const size_t p = (size_t)y * (size_t)w + (size_t)x;
  const float hk[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
  const float4 cp = cv_in[p], Ap = albedo[p], np = nhat[p];
  const float lp = denoise_luminance(cp);
  const float inv_l = 1.f / (r.sigma_l * sqrtf(cp.w) + 1e-4f);
  float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f;
  for (int dy = -2; dy <= 2; ++dy) {
    const int32_t qy = y + t * dy;
    if (qy < 0 || qy >= h) continue;
    for (int dx = -2; dx <= 2; ++dx) {
      const int32_t qx = x + t * dx;
      if (qx < 0 || qx >= w) continue;
      const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
      const float4 cq = cv_in[q], Aq = albedo[q], nq = nhat[q];
      const float dr = Ap.x - Aq.x, dg = Ap.y - Aq.y, db = Ap.z - Aq.z;
      // exp(e) * W_n as ONE exp2 of log2(e) e + sigma_n log2(d) (hardware v_exp_f32 / v_log_f32, no libm range reduction):
      // e <= 0 and d <= 1, so the argument is <= 0 and the weight <= h_dx h_dy.  (d is clamped to 1 against the rounding of
      // two unit vectors' dot product; a d of 0 or below, or a normal on one side only, gives W_n = 0.)
      float x = (-fabsf(lp - denoise_luminance(cq)) * inv_l - (dr * dr + dg * dg + db * db) * r.inv_sigma_a2) * 1.44269504f;
      bool zero = np.w != nq.w;
      if (np.w != 0.f && nq.w != 0.f) {
        const float d = np.x * nq.x + np.y * nq.y + np.z * nq.z;
        zero = !(d > 0.f);
        x += r.sigma_n * __builtin_amdgcn_logf(d < 1.f ? d : 1.f);
      }
      // the centre tap is p itself: e = 0 and W_n = 1 exactly (n^ . n^ may round below 1, and a huge sigma_n would zero it)
      const float wt = dx == 0 && dy == 0 ? hk[2] * hk[2] : (zero ? 0.f : hk[dy + 2] * hk[dx + 2] * __builtin_amdgcn_exp2f(x));
      sw += wt;
      sr += wt * cq.x;
      sg += wt * cq.y;
      sb += wt * cq.z;
      sv += (wt * wt) * cq.w;
    }
  }
  const float inv = 1.f / sw;
  const float4 o = make_float4(sr * inv, sg * inv, sb * inv, sv * (inv * inv));
  if (!LAST) {
    cv_out[p] = o;
    return;
  }
  double c[3] = {(double)o.x, (double)o.y, (double)o.z};
  if (r.demodulate) {
    const float Ac[3] = {Ap.x, Ap.y, Ap.z};
    for (int k = 0; k < 3; ++k) c[k] = c[k] * (Ac[k] > 1e-3f ? (double)Ac[k] : (double)1e-3f);
  }
  if (mean_rgb) { mean_rgb[3 * p] = c[0]; mean_rgb[3 * p + 1] = c[1]; mean_rgb[3 * p + 2] = c[2]; }
  if (rgb8) {
    int32_t v[3];
    rt::tone_map(rt::v3(c[0], c[1], c[2]), 1u, v);
    rgb8[3 * p] = (uint8_t)v[0];
    rgb8[3 * p + 1] = (uint8_t)v[1];
    rgb8[3 * p + 2] = (uint8_t)v[2];
  }
}
#endif  // !RTX_F32_TU
