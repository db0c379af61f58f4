"""A field of N individually rotated boxes in its two spellings: every box a slot of the world list ("hoisted": the scan is
O(N) per ray) against the boxes as members of one instance tree ("instanced", rtx_instance_bvh_from_list).

    python scripts/bench_instances.py [--sizes 64,1024,4096] [--width W] [--spp N] [--steps K] [--warmup W] [--spellings hoisted,instanced]

Prints one JSON line per (N, spelling):
  msamples_s, trace_ms   paths per second and trace time of k_trace_world (HIP events: RtxRenderStats.trace_ms), the median
                         of --steps renders after --warmup renders, with the min and max beside it;
  *_tests_per_ray        the counting kernel's work counters (rtx_render_count) over its rays, at a quarter of the width;
and one summary line per N with the ratio of the two trace times.  Both spellings give the same frame (checked here too).
The field is that of tests/instance_scenes.py: a ground sphere, a lamp, the boxes and a BvhNode of 12 spheres.
--spellings hoisted alone also runs on a build without the constructor (the parent's figures are taken that way).
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spellings", default="hoisted,instanced")
    args = ap.parse_args()
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")
    from instance_scenes import box_field, field_cam_cfg

    for n in [int(x) for x in args.sizes.split(",")]:
        rows, frames = {}, {}
        for spelling in args.spellings.split(","):
            cam, cfg, h = field_cam_cfg(rtsr, n=n, width=args.width, spp=args.spp, depth=30)
            b, world = box_field(rtsr, spelling, n=n)
            flat = b.flatten(world)
            scene = flat.upload()
            for _ in range(args.warmup):
                scene.render(cam, cfg)
            runs = [scene.render(cam, cfg, want_stats=True) for _ in range(args.steps)]
            ms = sorted(r.stats.trace_ms for r in runs)
            med = ms[len(ms) // 2]
            samples = runs[0].stats.samples
            ccfg = rtsr.Config.new(1.5, max(16, args.width // 4), 2, 30, 4, seed=11, background=(0.35, 0.4, 0.55))
            c = scene.render_count(cam, ccfg)
            row = {"n": n, "spelling": spelling, "kernel": rtsr.trace_kernel_name(runs[0].stats.trace_kernel),
                   "width": args.width, "height": h, "spp": args.spp, "slots": flat.info()["n_top_level"],
                   "instance_trees": flat.instances() if hasattr(flat, "instances") else None,
                   "trace_ms": round(med, 3), "trace_ms_min": round(ms[0], 3), "trace_ms_max": round(ms[-1], 3),
                   "msamples_s": round(samples / (med * 1e3), 2) if med > 0 else None,
                   "rect_tests_per_ray": round(c.rect_tests / c.rays, 2), "box_tests_per_ray": round(c.box_tests / c.rays, 2),
                   "sphere_tests_per_ray": round(c.sphere_tests / c.rays, 2)}
            rows[spelling], frames[spelling] = row, runs[0].accum
            print(json.dumps(row), flush=True)
        if len(rows) == 2:
            print(json.dumps({"n": n, "same_frame": bool(np.array_equal(frames["hoisted"], frames["instanced"])),
                              "trace_ms_ratio_hoisted_over_instanced": round(rows["hoisted"]["trace_ms"] / max(1e-9, rows["instanced"]["trace_ms"]), 2)}),
                  flush=True)


if __name__ == "__main__":
    main()
