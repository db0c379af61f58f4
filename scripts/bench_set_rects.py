"""What moving and resizing rectangles costs on a resident scene (rtx_scene_set_rects*), against today's only other route -- the
builder calls, a flatten and an upload -- and what the refitted trees cost a render.

    python scripts/bench_set_rects.py [--sizes 64,1024,4096] [--out profiles/rects/bench_set_rects.json]

Scenes: the Cornell box of scripts/swing_light.py, its ceiling light alone updated (1 rectangle: the record, the slot box, the
light table), and a box field -- a ground sphere, a sphere lamp and ONE instance tree of N Translate(RotateY(RectPrism))
members on a square grid, all 6 N rectangles updated (every box gets a new width and height through api.prism_rects: the
records, N member boxes, the instance tree above them).  Device work is timed with torch events on the stream the update is
enqueued on (RtxRenderStats.trace_ms for a render), host work with the wall clock.  Every figure is the median of 7 timed runs
after 2 warm-up runs, with the min and max beside it; everything runs in one process.  No threshold: these are the first
numbers.

Per scene --
  update_device_ms          rtx_scene_set_rects_device (values already on the device) between two events;
  update_call_ms            wall time of that call itself (checks, plan, staging, enqueue; it does not wait);
  update_host_device_ms     the same between events for rtx_scene_set_rects (values staged from the host: 40 B a rectangle);
  update_host_call_ms       wall time of that call;
  rebuild_graph_ms / rebuild_flatten_ms / rebuild_upload_ms
                            the same change without the feature, wall time: the world built anew, flattened, uploaded (which
                            also throws away the render workspace and any progressive handle);
  render_updated_ms         trace time of a 256 x 256 x 16 spp frame on the scene UPDATED to the last values;
  render_fresh_ms           on the scene BUILT for them;
  same_frame                the two frames: the same bits, or the run is void.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
WARMUP, RUNS = 2, 7


def stat(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def box_sizes(n, seed):
    """(n, 2): half width and height of every box, seeded."""
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(0.15, 0.4, n), rng.uniform(0.2, 0.7, n)])


def box_corners(size):
    w, h = float(size[0]), float(size[1])
    return (-w, 0.0, -w), (w, h, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from swing_light import LIGHT_REST, cornell
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")

    def field_world(sizes):
        n = len(sizes)
        b = rtsr.Builder(7)
        m = [b.lambertian((0.8, 0.3, 0.3)), b.metal((0.8, 0.8, 0.9), 0.3), b.lambertian((0.2, 0.7, 0.3)), b.lambertian((0.3, 0.3, 0.8))]
        cols = int(np.ceil(np.sqrt(n)))
        boxes, members = [], []
        for k in range(n):
            boxes.append(b.rect_prism(*box_corners(sizes[k]), m[k % 4]))
            x, z = -0.5 * cols + 1.0 * (k % cols) + 0.0137 * (k % 7), -0.5 * cols + 1.0 * (k // cols) + 0.0071 * (k % 5)
            members.append(b.translate((x, 0.0, z), b.rotate_y(7.0 + 5.3 * k, boxes[-1])))
        ground = b.sphere((0.0, -500.0, 0.0), 500.0, m[2])
        lamp = b.sphere((0.0, 0.6 * cols + 4.0, 1.0), 1.0 + 0.05 * cols, b.diffuse_light((4.0, 4.0, 4.0)))
        return b, b.hittable_list([ground, lamp, b.instance_bvh(b.hittable_list(members))]), boxes

    def light_values(k):
        rng = np.random.default_rng(500 + k)
        cx, cz, hx, hz = 278.0 + rng.uniform(-150.0, 150.0), 279.5 + rng.uniform(-100.0, 100.0), rng.uniform(30.0, 65.0), rng.uniform(25.0, 52.0)
        return np.array([[cx - hx, cx + hx, cz - hz, cz + hz, 554.0 - rng.uniform(0.0, 40.0)]])

    rows = []
    stream = torch.cuda.Stream()
    names = ["cornell_light"] + ["box_field_%d" % int(s) for s in args.sizes.split(",") if s]
    for name in names:
        if name == "cornell_light":
            b, world, light = cornell(rtsr, LIGHT_REST)
            flat = b.flatten(world)
            ids = flat.rect_ids(b, light)
            values_of = light_values
            rebuild = lambda vals: cornell(rtsr, vals[0])[:2]
            cam = rtsr.Camera.new((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0)
            bg, ls = (0.0, 0.0, 0.0), True
        else:
            n = int(name.rsplit("_", 1)[1])
            b, world, boxes = field_world(box_sizes(n, 3))
            flat = b.flatten(world)
            ids = np.concatenate([flat.rect_ids(b, h) for h in boxes])
            sizes_of = lambda k: box_sizes(n, 100 + k)
            values_of = lambda k: np.concatenate([rtsr.prism_rects(*box_corners(s)) for s in sizes_of(k)])
            rebuild = None
            cols = float(np.ceil(np.sqrt(n)))
            cam = rtsr.Camera.new((0.1 * cols, 0.55 * cols + 2.0, 1.05 * cols + 3.0), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0), 42.0, 1.0, 0.0, 10.0, 0.0, 1.0)
            bg, ls = (0.35, 0.4, 0.55), False
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        assert len(set(ids.tolist())) == len(ids)
        scene = flat.upload()
        ids_p = ids.ctypes.data_as(C.POINTER(C.c_int32))
        cfg = rtsr.Config.new(1.0, 256, 16, 30, 4, seed=11, background=bg)
        dev, call, hostdev, hostcall, graph, flatten, up = [], [], [], [], [], [], []
        fresh = None
        for k in range(WARMUP + RUNS):
            vals = np.ascontiguousarray(values_of(k), dtype=np.float64)
            assert vals.shape == (len(ids), 5)
            d_v = torch.from_numpy(vals).cuda()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            torch.cuda.synchronize()
            e[0].record(stream)
            t0 = time.perf_counter()
            st = rtsr.lib.rtx_scene_set_rects_device(scene.ptr, ids_p, len(ids), C.c_void_p(d_v.data_ptr()), C.c_void_p(stream.cuda_stream))
            t1 = time.perf_counter()
            e[1].record(stream)
            assert st == rtsr.RTX_OK, rtsr.last_error()
            stream.synchronize()
            e[2].record(stream)
            t6 = time.perf_counter()
            st = rtsr.lib.rtx_scene_set_rects(scene.ptr, ids_p, len(ids), vals.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(stream.cuda_stream))
            t7 = time.perf_counter()
            e[3].record(stream)
            assert st == rtsr.RTX_OK, rtsr.last_error()
            stream.synchronize()
            # the way to the same scene without the feature: the world built anew, flattened and uploaded
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            bf, wf = rebuild(vals) if name == "cornell_light" else field_world(sizes_of(k))[:2]
            t3 = time.perf_counter()
            fresh_flat = bf.flatten(wf)
            t4 = time.perf_counter()
            fresh = fresh_flat.upload()
            torch.cuda.synchronize()
            t5 = time.perf_counter()
            if k >= WARMUP:
                dev.append(e[0].elapsed_time(e[1])); call.append(1e3 * (t1 - t0)); hostdev.append(e[2].elapsed_time(e[3])); hostcall.append(1e3 * (t7 - t6))
                graph.append(1e3 * (t3 - t2)); flatten.append(1e3 * (t4 - t3)); up.append(1e3 * (t5 - t4))
        updated, built = [], []
        a = f = None
        for k in range(WARMUP + RUNS):
            a = scene.render(cam, cfg, want_stats=True, light_sampling=ls)
            f = fresh.render(cam, cfg, want_stats=True, light_sampling=ls)
            if k >= WARMUP:
                updated.append(a.stats.trace_ms); built.append(f.stats.trace_ms)
        row = {"scene": name, "rects_updated": len(ids), "nodes": flat.info()["n_nodes"],
               "update_device_ms": stat(dev), "update_call_ms": stat(call), "update_host_device_ms": stat(hostdev), "update_host_call_ms": stat(hostcall),
               "rebuild_graph_ms": stat(graph), "rebuild_flatten_ms": stat(flatten), "rebuild_upload_ms": stat(up),
               "render": "256x256x16spp" + (" light_sampling" if ls else ""), "kernel": rtsr.trace_kernel_name(a.stats.trace_kernel),
               "render_updated_ms": stat(updated), "render_fresh_ms": stat(built),
               "same_frame": bool(np.array_equal(a.accum, f.accum) and np.array_equal(a.rgb8, f.rgb8))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del scene, fresh
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            json.dump({"warmup": WARMUP, "runs": RUNS, "rows": rows}, fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main()
