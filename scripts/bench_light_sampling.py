"""Light sampling against the reference's estimator on the Cornell box (scene 4) and the Book-2 final scene (scene 6).

    python scripts/bench_light_sampling.py [--width W] [--spp N] [--book2-full]

Prints one JSON line per (scene, estimator) and one summary line per scene:
  msamples_s        paths per second of the trace kernel at --spp samples per pixel (HIP events: RtxRenderStats.trace_ms of
                    a progressive add, after a warm-up add on another handle);
  mean_pixel_var    the mean over pixels and channels of the per-sample variance (Q - S^2/n) / (n - 1) at equal spp;
  var_ratio         light sampling's mean_pixel_var over the default's;
  adaptive          rtx_progressive_until_adaptive(batch 16, min_spp 16, target 0.05) with a budget of 4096 spp: the paths it
                    traced (RtxAdaptiveStats.samples), its spp reached and its wall time in ms (trace + retirement checks).
Scene 6 is the reduced Book-2 world (4 boxes per side, 50 spheres) unless --book2-full.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--book2-full", action="store_true")
    args = ap.parse_args()
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")

    for scene_id in (4, 6):
        kw = {"book2_boxes_per_side": 4, "book2_spheres": 50} if scene_id == 6 and not args.book2_full else {}
        b = rtsr.Builder(1)
        world, cam, bg = b.get_world_cam(scene_id, **kw)
        scene = b.flatten(world).upload()
        rows = {}
        for ls in (False, True):
            cfg = rtsr.Config.new(1.0, args.width, args.spp, 50, 4, seed=13, background=bg)
            warm = scene.progressive(cam, cfg, light_sampling=ls)
            warm.add(min(4, args.spp))
            del warm
            p = scene.progressive(cam, cfg, light_sampling=ls)
            st = p.add(args.spp, want_stats=True)
            S, Q = p.moments()
            n = args.spp
            var = np.maximum(Q - S * S / n, 0.0) / (n - 1)
            del p
            acfg = rtsr.Config.new(1.0, args.width, 4096, 50, 4, seed=17, background=bg)
            pa = scene.progressive(cam, acfg, light_sampling=ls)
            t0 = time.perf_counter()
            ast = pa.until_adaptive(16, 16, 0.05)
            ms = (time.perf_counter() - t0) * 1e3
            del pa
            row = {"scene": scene_id, "light_sampling": ls, "kernel": rtsr.trace_kernel_name(st.trace_kernel),
                   "width": args.width, "height": rtsr.image_height(cfg), "spp": n,
                   "msamples_s": round(st.samples / (st.trace_ms * 1e3), 2) if st.trace_ms > 0 else None,
                   "mean_pixel_var": float(var.mean()),
                   "adaptive": {"paths": int(ast.samples), "spp_reached": int(ast.spp_done), "pixels_above": int(ast.pixels_above),
                                "ms": round(ms, 2)}}
            rows[ls] = row
            print(json.dumps(row), flush=True)
        print(json.dumps({"scene": scene_id, "var_ratio": rows[True]["mean_pixel_var"] / rows[False]["mean_pixel_var"],
                          "paths_ratio": rows[True]["adaptive"]["paths"] / max(1, rows[False]["adaptive"]["paths"]),
                          "ms_ratio": rows[True]["adaptive"]["ms"] / max(1e-9, rows[False]["adaptive"]["ms"])}), flush=True)


if __name__ == "__main__":
    main()
