// Stand-in for the reference binary (/root/reference/src/main.rs:1-16): pick a scene from the
// catalogue, render it, print P3 PPM on stdout and "Time taken" on stderr.  The reference hard-codes
// THREADS = 11, SCENE_ID = 11 and Config::new(1.6, 600, 1000, 50, THREADS); here the same values are the
// defaults and every one of them can be overridden on the command line.
//
//   rtx_render [--scene ID] [--aspect A] [--width W] [--spp S] [--depth D] [--threads T] [--seed N]
//              [--scene-seed N] [--out FILE.ppm] [--camera-aspect A] [--ply FILE] [--earth FILE.ppm]
//              [--row-chunk-compat] [--batch N --target-error E [--snapshot-every K]]
//              [--batch N --target-error E --adaptive [--min-spp M] [--spp-map FILE.pgm]]
//              [--batch N --target-error E [--adaptive ...] --denoise [--noisy-out FILE.ppm] [--albedo-out FILE.ppm]
//               [--normal-out FILE.ppm]]
//              [--light-sampling]
//
// --batch / --target-error render progressively: N samples at a time until no pixel's relative error exceeds E or --spp
// samples are in (rtx_progressive_until); the spp reached and the final noise stats go to stderr.  --snapshot-every K
// also writes the frame after every K samples to <out>.<spp>.ppm (needs --out).
// --adaptive stops tracing each pixel once its relative error is at most E, checked at every batch boundary from M samples
// on (default 2; rtx_progressive_until_adaptive); stderr also gets the samples traced against a uniform render's.
// --spp-map writes each pixel's sample count as a plain PGM (top row first, maxval = --spp).
// --denoise (with --batch) writes the denoised frame (rtx_progressive_denoise, default parameters) where the frame would go;
// --noisy-out gets the frame as accumulated, --albedo-out and --normal-out the filter's first-hit guides (albedo clamped to
// [0, 1], normal mapped to 0.5 + 0.5 n; linear, not tone-mapped).
// --light-sampling traces with next-event estimation and MIS (rtx_render_ex / rtx_progressive_create_ex; statistical), in
// every mode above.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../csrc/host/world.hpp"

// A feature buffer (rows * w * 3 floats, row 0 = bottom) as a PPM: each value v -> 255.9 * clamp(offset + scale * v, 0, 1).
static void write_feature_ppm(const char* path, int w, int h, const std::vector<float>& v, double offset, double scale) {
  std::vector<uint8_t> rgb8(v.size());
  for (size_t k = 0; k < v.size(); ++k) {
    double x = offset + scale * (double)v[k];
    x = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
    rgb8[k] = (uint8_t)(int)(255.9 * x);
  }
  rtsr::check(rtx_write_ppm(path, w, h, rgb8.data()));
}

static const size_t THREADS = 11;  // main.rs:4
static const int SCENE_ID = 11;    // main.rs:5

int main(int argc, char** argv) {
  auto start = std::chrono::steady_clock::now();  // main.rs:8: the timer covers scene build + render + PPM
  int scene_id = SCENE_ID, width = 600, spp = 1000, depth = 50;
  size_t threads = THREADS;
  double aspect = 1.6, camera_aspect = 0.0;
  uint64_t seed = 1, scene_seed = 1;
  const char* out = nullptr;
  const char* ply = nullptr;
  const char* earth = nullptr;
  bool compat = false;
  int batch = 0, snapshot_every = 0, min_spp = 2;
  double target_error = -1.0;
  bool adaptive = false;
  const char* spp_map = nullptr;
  bool denoise = false;
  const char* noisy_out = nullptr;
  const char* albedo_out = nullptr;
  const char* normal_out = nullptr;
  bool light_sampling = false;
  for (int i = 1; i < argc; ++i) {
    auto need = [&](const char* flag) -> const char* {
      if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", flag); exit(2); }
      return argv[++i];
    };
    if (!strcmp(argv[i], "--scene")) scene_id = atoi(need("--scene"));
    else if (!strcmp(argv[i], "--aspect")) aspect = atof(need("--aspect"));
    else if (!strcmp(argv[i], "--camera-aspect")) camera_aspect = atof(need("--camera-aspect"));
    else if (!strcmp(argv[i], "--width")) width = atoi(need("--width"));
    else if (!strcmp(argv[i], "--spp")) spp = atoi(need("--spp"));
    else if (!strcmp(argv[i], "--depth")) depth = atoi(need("--depth"));
    else if (!strcmp(argv[i], "--threads")) threads = (size_t)atoi(need("--threads"));
    else if (!strcmp(argv[i], "--seed")) seed = strtoull(need("--seed"), nullptr, 10);
    else if (!strcmp(argv[i], "--scene-seed")) scene_seed = strtoull(need("--scene-seed"), nullptr, 10);
    else if (!strcmp(argv[i], "--out")) out = need("--out");
    else if (!strcmp(argv[i], "--ply")) ply = need("--ply");
    else if (!strcmp(argv[i], "--earth")) earth = need("--earth");
    else if (!strcmp(argv[i], "--row-chunk-compat")) compat = true;
    else if (!strcmp(argv[i], "--batch")) batch = atoi(need("--batch"));
    else if (!strcmp(argv[i], "--target-error")) target_error = atof(need("--target-error"));
    else if (!strcmp(argv[i], "--snapshot-every")) snapshot_every = atoi(need("--snapshot-every"));
    else if (!strcmp(argv[i], "--adaptive")) adaptive = true;
    else if (!strcmp(argv[i], "--min-spp")) min_spp = atoi(need("--min-spp"));
    else if (!strcmp(argv[i], "--spp-map")) spp_map = need("--spp-map");
    else if (!strcmp(argv[i], "--denoise")) denoise = true;
    else if (!strcmp(argv[i], "--noisy-out")) noisy_out = need("--noisy-out");
    else if (!strcmp(argv[i], "--albedo-out")) albedo_out = need("--albedo-out");
    else if (!strcmp(argv[i], "--normal-out")) normal_out = need("--normal-out");
    else if (!strcmp(argv[i], "--light-sampling")) light_sampling = true;
    else { fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
  }
  const bool progressive = batch > 0 || target_error >= 0.0;
  if (progressive && (batch <= 0 || !(target_error >= 0.0))) {
    fprintf(stderr, "--batch N (> 0) and --target-error E (>= 0) go together\n");
    return 2;
  }
  if (snapshot_every > 0 && (!progressive || !out)) {
    fprintf(stderr, "--snapshot-every needs --batch, --target-error and --out\n");
    return 2;
  }
  if (adaptive && !progressive) {
    fprintf(stderr, "--adaptive needs --batch N (> 0) and --target-error E (>= 0)\n");
    return 2;
  }
  if (!adaptive && (spp_map || min_spp != 2)) {
    fprintf(stderr, "--min-spp and --spp-map need --adaptive\n");
    return 2;
  }
  if (adaptive && (min_spp < 2 || min_spp > spp)) {
    fprintf(stderr, "--min-spp M must be in [2, --spp]\n");
    return 2;
  }
  if (adaptive && snapshot_every > 0) {
    fprintf(stderr, "--snapshot-every and --adaptive do not go together\n");
    return 2;
  }
  if (denoise && !progressive) {
    fprintf(stderr, "--denoise needs --batch N (> 0) and --target-error E (>= 0)\n");
    return 2;
  }
  if (denoise && (spp < 2 || compat)) {
    fprintf(stderr, "--denoise needs --spp >= 2 and every row (no --row-chunk-compat)\n");
    return 2;
  }
  if (!denoise && (noisy_out || albedo_out || normal_out)) {
    fprintf(stderr, "--noisy-out, --albedo-out and --normal-out need --denoise\n");
    return 2;
  }
  try {
    rtsr::Scene scene(scene_seed);
    RtxSceneOptions opt;
    memset(&opt, 0, sizeof(opt));
    opt.camera_aspect = camera_aspect;
    opt.dragon_ply = ply ? ply : "./models/dragon_recon/dragon_vrip_res2.ply";  // world.rs:684
    opt.earth_ppm = earth ? earth : "earthshit.ppm";                              // world.rs:290,580
    rtsr::WorldCam wc = rtsr::get_world_cam(scene, scene_id, &opt);               // main.rs:10
    rtsr::Config config = rtsr::Config::new_(aspect, width, spp, depth, threads);  // main.rs:11
    config.c.seed = seed;
    config.c.row_chunk_compat = compat ? 1 : 0;
    rtsr::Screen screen;
    rtsr::DenoiseOutputs dn;
    rtsr::DenoiseOutputs* dnp = denoise ? &dn : nullptr;
    RtxIntegratorOptions iopt;
    memset(&iopt, 0, sizeof(iopt));
    iopt.light_sampling = 1;
    const RtxIntegratorOptions* integrator = light_sampling ? &iopt : nullptr;
    if (adaptive) {
      RtxAdaptiveStats as = {};
      screen = rtsr::render_scene_adaptive(scene, wc.world, wc.cam, wc.background, config, batch, min_spp, target_error, &as, dnp,
                                           integrator);
      const double uniform = (double)as.spp_done * (double)as.pixels;
      fprintf(stderr, "spp reached: %d of %d; pixels above %g: %d of %d; max rel err %.6g, mean rel err %.6g\n", as.spp_done,
              spp, target_error, as.pixels_above, as.pixels, as.max_rel_err, as.mean_rel_err);
      fprintf(stderr, "adaptive: %llu samples traced, %.4g of a uniform render's %d spp x %d pixels; %d pixels still active\n",
              (unsigned long long)as.samples, uniform > 0 ? (double)as.samples / uniform : 0.0, as.spp_done, as.pixels,
              as.pixels_active);
      if (spp_map) screen.write_spp_pgm_file(spp_map, spp);
    } else if (progressive) {
      RtxNoiseStats ns = {};
      auto snap = [&](const rtsr::Screen& s, int spp_now) {
        std::string path = std::string(out) + "." + std::to_string(spp_now) + ".ppm";
        s.write_to_ppm_file(path.c_str());
      };
      screen = rtsr::render_scene_progressive(scene, wc.world, wc.cam, wc.background, config, batch, target_error, &ns,
                                              snapshot_every, snap, dnp, integrator);
      fprintf(stderr, "spp reached: %d of %d; pixels above %g: %d of %d; max rel err %.6g, mean rel err %.6g\n", ns.spp_done,
              spp, target_error, ns.pixels_above, ns.pixels, ns.max_rel_err, ns.mean_rel_err);
    } else {
      screen = rtsr::render_scene(scene, wc.world, wc.cam, wc.background, config, nullptr, integrator);  // main.rs:13
    }
    if (noisy_out) dn.noisy.write_to_ppm_file(noisy_out);
    if (albedo_out) write_feature_ppm(albedo_out, screen.width, screen.height, dn.albedo, 0.0, 1.0);
    if (normal_out) write_feature_ppm(normal_out, screen.width, screen.height, dn.normal, 0.5, 0.5);
    if (out) screen.write_to_ppm_file(out);
    else screen.write_to_ppm();
  } catch (const rtsr::Error& e) {
    fprintf(stderr, "rtx_render: %s (status %d)\n", e.what(), (int)e.status);
    return 1;
  }
  double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
  fprintf(stderr, "Time taken: %.3fs\n", secs);  // main.rs:15
  return 0;
}
