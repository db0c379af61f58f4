"""What moving the members of an instance tree costs on a resident scene (rtx_scene_set_transforms), and what the refitted tree
costs a render.

    python scripts/bench_set_transforms.py [--sizes 64,1024,4096] [--out profiles/animate/bench_set_transforms.json]

The field is tests/instance_scenes.py: box_field (a ground sphere, a lamp, N Translate(RotateY(RectPrism)) boxes and a BvhNode
of 12 spheres, the boxes and the BvhNode members of ONE instance tree).  Device work is timed with HIP events (torch events on
the stream the update is enqueued on; RtxRenderStats.trace_ms for a render), host work with the wall clock.  Every figure is
the median of 7 timed runs after 2 warm-up runs, with the min and max beside it.

Measurement 1, per N: one update of EVERY member --
  update_device_ms   the copy, k_set_slot_ops and k_refit_instance_tree, between two events on the stream;
  update_call_ms     wall time of the rtx_scene_set_transforms call itself (checks, staging, enqueue; it does not wait);
  update_python_ms   wall time of turning the {slot: ops} dict into the C array (api.py: _slot_ops), paid before the call;
beside what the same change costs without the feature --
  rebuild_flatten_ms, rebuild_upload_ms   rtx_flatten of the re-posed graph (a host SAH build) and rtx_scene_upload of the
                                          result, wall time, the device idle before and after.
Measurement 2, per N: one render at 256 x 256 x 16 spp after every member got a new random pose (a new angle, an offset moved
by up to 0.4) --
  render_refit_ms    trace time on the tree REFITTED to that pose;
  render_fresh_ms    trace time on the tree BUILT for that pose (the same world flattened from scratch);
and whether the two frames are the same bits (they must be).
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
    from set_transforms_cases import build, random_values, updates_for

    rows = []
    stream = torch.cuda.Stream()
    for n in [int(x) for x in args.sizes.split(",")]:
        scene_fn = lambda r: box_field(r, "instanced", n=n)
        b, w, calls = build(rtsr, scene_fn)
        flat = b.flatten(w)
        scene = flat.upload()
        s = n ** 0.5
        cam = rtsr.Camera.new((0.1 * s, 0.55 * s, 1.05 * s), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0), 42.0, 1.0, 0.0, 1.0 * s, 0.0, 1.0)
        cfg = rtsr.Config.new(1.0, 256, 16, 30, 4, seed=11, background=(0.35, 0.4, 0.55))
        assert rtsr.image_height(cfg) == 256
        dev, call, py, fl, up = [], [], [], [], []
        for k in range(WARMUP + RUNS):
            values = random_values(calls, seed=100 + k)
            upd = updates_for(flat, calls, values)
            t0 = time.perf_counter()
            arr = api._slot_ops(flat, upd)
            t1 = time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            t2 = time.perf_counter()
            st = rtsr.lib.rtx_scene_set_transforms(scene.ptr, arr, len(arr), C.c_void_p(stream.cuda_stream))
            t3 = time.perf_counter()
            e1.record(stream)
            assert st == rtsr.RTX_OK, rtsr.last_error()
            stream.synchronize()
            # the parent's way to the same scene: the graph built at the new pose, flattened and uploaded
            bf, wf, _ = build(rtsr, scene_fn, values)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            fresh_flat = bf.flatten(wf)
            t5 = time.perf_counter()
            fresh = fresh_flat.upload()
            torch.cuda.synchronize()
            t6 = time.perf_counter()
            if k >= WARMUP:
                dev.append(e0.elapsed_time(e1)); call.append(1e3 * (t3 - t2)); py.append(1e3 * (t1 - t0))
                fl.append(1e3 * (t5 - t4)); up.append(1e3 * (t6 - t5))
        # measurement 2, at the last pose: `scene` holds the refitted tree, `fresh` the tree built for the pose
        refit, built = [], []
        for k in range(WARMUP + RUNS):
            a = scene.render(cam, cfg, want_stats=True)
            f = fresh.render(cam, cfg, want_stats=True)
            if k >= WARMUP:
                refit.append(a.stats.trace_ms); built.append(f.stats.trace_ms)
        row = {"n": n, "members": flat.instance_tree(0)["n_slots"], "tree_depth": flat.instance_tree(0)["depth"],
               "update_device_ms": stat(dev), "update_call_ms": stat(call), "update_python_ms": stat(py),
               "rebuild_flatten_ms": stat(fl), "rebuild_upload_ms": stat(up),
               "render": "256x256x16spp", "kernel": rtsr.trace_kernel_name(a.stats.trace_kernel),
               "render_refit_ms": stat(refit), "render_fresh_ms": stat(built),
               "fresh_tree_depth": fresh_flat.instance_tree(0)["depth"], "same_frame": bool(np.array_equal(a.accum, f.accum))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            json.dump({"warmup": WARMUP, "runs": RUNS, "rows": rows}, fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main()
