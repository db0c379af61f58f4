"""What rebuilding an instance tree costs on a resident scene (rtx_scene_rebuild_instance_trees), and what the rebuilt tree
saves a render.

    python scripts/bench_rebuild_instances.py [--sizes 64,1024,4096] [--out profiles/animate/bench_rebuild_instances.json]

The field is tests/instance_scenes.py: box_field with N boxes, in the SCRAMBLE pose of tests/rebuild_cases.py (box i stands in
the grid cell of box pi(i), pi a fixed multiplicative permutation): every member has travelled far from where the flattener's
tree saw it.  Device work is timed with HIP events (torch events on the stream the work is enqueued on; RtxRenderStats.trace_ms
for a render), host work with the wall clock.  Every figure is the median of 7 timed runs after 2 warm-up runs, with the min and
max beside it.

Measurement 1, per N: the scene is at the scramble pose (one set_transforms of every member) and then
  rebuild_device_ms   the kernels, the sort and the commit copies of one rebuild, between two events on the stream;
  rebuild_call_ms     wall time of the rtx_scene_rebuild_instance_trees call (it waits once, for the depths);
  refit_device_ms     the set_transforms of every member alone (copy, k_set_slot_ops, k_refit_instance_tree), for scale;
beside the only other way to a tree built for the pose --
  reflatten_ms, reupload_ms   rtx_flatten of the re-posed graph (a host SAH build) and rtx_scene_upload of the result, wall
                              time, the device idle before and after.  flatten.cpp and the upload are the parent commit's code.
Measurement 2, per N: one render at 256 x 256 x 16 spp of the scramble pose on
  render_refit_ms     the tree refitted to the pose (the flattener's topology of the first pose);
  render_rebuilt_ms   the tree rebuilt on the device (Morton);
  render_sah_ms       the tree of a fresh flatten at the pose (host SAH);
and whether the three frames are the same bits (they must be).
Measurement 3: the three costs (rtx_scene_instance_tree_cost; the fresh flat's for SAH) and depths.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WARMUP, RUNS = 2, 7


def stat(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")
    api = importlib.import_module("ray-tracing-series-rust_amd.api")
    from instance_scenes import box_field
    from rebuild_cases import scramble_values
    from set_transforms_cases import build, updates_for

    rows = []
    stream = torch.cuda.Stream()
    raw = C.c_void_p(stream.cuda_stream)
    for n in [int(x) for x in args.sizes.split(",")]:
        scene_fn = lambda r: box_field(r, "instanced", n=n)
        b, w, calls = build(rtsr, scene_fn)
        flat = b.flatten(w)
        scrambled = scramble_values(calls, n)
        arr_pose = api._slot_ops(flat, updates_for(flat, calls, scrambled))
        refit_only = flat.upload()   # stays refitted
        assert rtsr.lib.rtx_scene_set_transforms(refit_only.ptr, arr_pose, len(arr_pose), None) == rtsr.RTX_OK
        s = n ** 0.5
        cam = rtsr.Camera.new((0.1 * s, 0.55 * s, 1.05 * s), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0), 42.0, 1.0, 0.0, 1.0 * s, 0.0, 1.0)
        cfg = rtsr.Config.new(1.0, 256, 16, 30, 4, seed=11, background=(0.35, 0.4, 0.55))
        assert rtsr.image_height(cfg) == 256
        dev, call, refit, fl, up = [], [], [], [], []
        stats = api.RtxRebuildStats()
        for k in range(WARMUP + RUNS):
            scene = flat.upload()  # the flattener's tree of the first pose, every run; refitted, then rebuilt
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize()
            ev[0].record(stream)
            assert rtsr.lib.rtx_scene_set_transforms(scene.ptr, arr_pose, len(arr_pose), raw) == rtsr.RTX_OK
            ev[1].record(stream)
            t0 = time.perf_counter()
            st = rtsr.lib.rtx_scene_rebuild_instance_trees(scene.ptr, None, 0, raw, C.byref(stats))
            t1 = time.perf_counter()
            ev[2].record(stream)
            assert st == rtsr.RTX_OK, rtsr.last_error()
            stream.synchronize()
            bf, wf, _ = build(rtsr, scene_fn, scrambled)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            fresh_flat = bf.flatten(wf)
            t3 = time.perf_counter()
            fresh = fresh_flat.upload()
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            if k >= WARMUP:
                refit.append(ev[0].elapsed_time(ev[1])); dev.append(ev[1].elapsed_time(ev[2])); call.append(1e3 * (t1 - t0))
                fl.append(1e3 * (t3 - t2)); up.append(1e3 * (t4 - t3))
        r_refit, r_rebuilt, r_sah = [], [], []
        for k in range(WARMUP + RUNS):
            a = refit_only.render(cam, cfg, want_stats=True)
            m = scene.render(cam, cfg, want_stats=True)
            f = fresh.render(cam, cfg, want_stats=True)
            if k >= WARMUP:
                r_refit.append(a.stats.trace_ms); r_rebuilt.append(m.stats.trace_ms); r_sah.append(f.stats.trace_ms)
        row = {"n": n, "members": flat.instance_tree(0)["n_slots"], "pose": "scramble",
               "rebuild_device_ms": stat(dev), "rebuild_call_ms": stat(call), "refit_device_ms": stat(refit),
               "reflatten_ms": stat(fl), "reupload_ms": stat(up),
               "render": "256x256x16spp", "kernel": rtsr.trace_kernel_name(m.stats.trace_kernel),
               "render_refit_ms": stat(r_refit), "render_rebuilt_ms": stat(r_rebuilt), "render_sah_ms": stat(r_sah),
               "same_frame": bool(np.array_equal(a.accum, m.accum) and np.array_equal(m.accum, f.accum)),
               "cost_refit": refit_only.instance_tree_cost(0), "cost_rebuilt": scene.instance_tree_cost(0), "cost_sah": fresh_flat.instance_tree_cost(0),
               "depth_refit": flat.instance_tree(0)["depth"], "depth_rebuilt": stats.max_depth, "depth_sah": fresh_flat.instance_tree(0)["depth"],
               "max_stack_refit": refit_only.max_stack(), "max_stack_rebuilt": scene.max_stack()}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump({"warmup": WARMUP, "runs": RUNS, "rows": rows}, fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main()
