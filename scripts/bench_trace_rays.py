"""Throughput of radiance queries (Scene.trace_rays, device pointers) on primary rays at 1920 x 1080, 16 spp, depth 50.

    python scripts/bench_trace_rays.py [--out profiles/trace_rays/bench_trace_rays.json] [--scenes 100,6,11]
    python scripts/bench_trace_rays.py --yardstick [--out FILE]     # runs from a checkout of an earlier commit too

Scenes: 100 (Book-1 final), 6 (Book-2 final) and 11 (the mesh room).  The rays are the camera's pinhole rays through the pixel
centres, built with torch on the device (scripts/bench_cast_rays.py: primary_rays), in scanline order and in one fixed random
permutation of it (torch.randperm, seed 1), every ray at time 0.  Cases: f64 scenes with both estimators, f32 scenes with the
reference's.  Method: 2 warm-up calls, then 7 timed ones, each rtx_scene_trace_rays_device alone (sums allocated beforehand, no
stats) between two HIP events on torch's current stream: the interval holds the trace kernel and the reduction.  Median, min and
max.  Output: one JSON document on stdout and, with --out, in a file.

--yardstick times rtx_render_ex with light_sampling = 1 at the same size, spp and depth through the scene's own camera: its
RtxRenderStats.trace_ms (k_trace_nee alone: the same scheduling, two walks per vertex), 2 warm-up + 7 renders, median.  The mode
uses nothing newer than rtx_render_ex, so this file runs unchanged from a checkout of the parent commit to time that build.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, SPP, DEPTH = 1920, 1080, 16, 50
WARMUP, STEPS = 2, 7
NAMES = {100: "book1_final", 6: "book2_final", 11: "mesh_room"}


def primary_rays(torch, cam, dev):
    """(origins, directions) of the W x H pinhole rays through the pixel centres, scanline order (row 0 = bottom)."""
    v = lambda a: torch.tensor(list(a), dtype=torch.float64, device=dev)
    s = (torch.arange(W, dtype=torch.float64, device=dev) + 0.5) / W
    t = (torch.arange(H, dtype=torch.float64, device=dev) + 0.5) / H
    d = v(cam.lower_left_corner) + s[None, :, None] * v(cam.horizontal) + t[:, None, None] * v(cam.vertical) - v(cam.origin)
    d = d.reshape(-1, 3).contiguous()
    return v(cam.origin).expand(W * H, 3).contiguous(), d


def summary(ms):
    med = statistics.median(ms)
    return {"ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "msamples_per_s": round(W * H * SPP / med / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", default="100,6,11")
    ap.add_argument("--yardstick", action="store_true")
    args = ap.parse_args()
    import torch  # first: the library then shares torch's HIP runtime (tests/conftest.py)
    torch.cuda.init()
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")
    dev = torch.device("cuda", 0)
    result = {"size": [W, H], "spp": SPP, "max_depth": DEPTH, "warmup": WARMUP, "steps": STEPS,
              "device": torch.cuda.get_device_name(0), "library": os.path.relpath(rtsr.LIB_PATH, ROOT),
              "mode": "yardstick" if args.yardstick else "trace_rays", "cases": []}
    for scene_id in [int(x) for x in args.scenes.split(",")]:
        b = rtsr.Builder(1)
        world, cam, bg = b.get_world_cam(scene_id, camera_aspect=W / H)
        flat = b.flatten(world)
        if args.yardstick:
            cfg = rtsr.Config.new(W / H, W, SPP, DEPTH, 10, seed=1, background=bg)
            scene = flat.upload()
            ms = []
            for k in range(WARMUP + STEPS):
                screen = scene.render(cam, cfg, want_accum=False, light_sampling=True, want_stats=True)
                if k >= WARMUP:
                    ms.append(screen.stats.trace_ms)
            case = {"scene": scene_id, "name": NAMES.get(scene_id, str(scene_id)), "what": "rtx_render_ex light_sampling=1 trace_ms",
                    "kernel": rtsr.trace_kernel_name(screen.stats.trace_kernel), "image": [cfg.image_width, rtsr.image_height(cfg)]}
            case.update(summary(ms))
            result["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
            del scene
            continue
        o, d = primary_rays(torch, cam, dev)
        g = torch.Generator(device="cpu")
        g.manual_seed(1)
        perm = torch.randperm(W * H, generator=g).to(dev)
        orders = {"scanline": (o, d), "permuted": (o[perm].contiguous(), d[perm].contiguous())}
        for f32, nee in ((False, False), (False, True), (True, False)):
            scene = flat.upload(f32=f32)
            for order, (oo, dd) in orders.items():
                # the sums, the argument block and Scene.trace_rays' own checks stay outside the timed interval: one checked
                # call first (it also gives the mean radiance), then the entry point alone between the events
                r = scene.trace_rays(oo, dd, spp=SPP, max_depth=DEPTH, background=tuple(bg), seed=1, light_sampling=nee)
                q = rtsr.RtxRadianceRays()
                rtsr.lib.rtx_radiance_rays_defaults(C.byref(q))
                q.n, q.origin, q.direction, q.samples, q.max_depth = W * H, oo.data_ptr(), dd.data_ptr(), SPP, DEPTH
                q.background[:] = tuple(bg)
                q.light_sampling = 1 if nee else 0
                stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream or None)
                ms = []
                for k in range(WARMUP + STEPS):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    status = rtsr.lib.rtx_scene_trace_rays_device(scene.ptr, C.byref(q), r.sum.data_ptr(), None, stream, None)
                    e1.record()
                    e1.synchronize()
                    if status != rtsr.RTX_OK:
                        raise rtsr.RtxError(status, rtsr.last_error())
                    if k >= WARMUP:
                        ms.append(e0.elapsed_time(e1))
                case = {"scene": scene_id, "name": NAMES.get(scene_id, str(scene_id)), "precision": "f32" if f32 else "f64",
                        "estimator": "light_sampling" if nee else "reference", "order": order,
                        "mean_radiance": round(float(r.mean.mean()), 6)}
                case.update(summary(ms))
                result["cases"].append(case)
                print(json.dumps(case), file=sys.stderr, flush=True)
            del scene
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
