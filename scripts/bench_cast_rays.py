"""Throughput of ray queries (Scene.cast_rays, device pointers) on primary rays at 1920 x 1080.

    python scripts/bench_cast_rays.py [--out profiles/raycast/bench_cast_rays.json] [--scenes 100,6,11,12]
    python scripts/bench_cast_rays.py --features-yardstick      # k_features at feature_spp = 1, for a kernel trace

Scenes: 100 (Book-1 final), 6 (Book-2 final), 11 (the mesh room: the dragon-class mesh of 871 200 triangles in its room of
rectangles) and 12 (the triangular prism in the Cornell room).  The rays are the camera's pinhole rays through the pixel
centres, built with torch on the device: origin = camera origin, direction = lower_left + s horizontal + t vertical - origin,
in scanline order and in one fixed random permutation of it (torch.randperm, seed 1).  Cases: every column against t + ids
only, f64 and f32 scenes.  Method: 2 warm-up casts, then 7 timed ones, each rtx_scene_cast_rays_device alone (columns allocated
beforehand) between two HIP events on torch's current stream; median, min and max.  Output: one JSON document (Mrays/s, bytes read and written per ray) on stdout and, with --out, in a file.

--features-yardstick runs rtx_progressive_features with feature_spp = 1 three times on each scene at the same size and
prints nothing to time: it exists to be run under `rocprofv3 --kernel-trace --stats`, where k_features -- the same first hits
from the camera's own rays, 32 B written per pixel -- is the yardstick for the walk.  The mode uses nothing newer than rtx_progressive_features, so the same file runs
unchanged from a checkout of an earlier commit to time that commit's build.
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
W, H = 1920, 1080
WARMUP, STEPS = 2, 7
NAMES = {100: "book1_final", 6: "book2_final", 11: "mesh_room", 12: "triangular_prism"}
BYTES = {"t": 8, "p": 24, "normal": 24, "uv": 16, "ids": 16}


def primary_rays(torch, cam, dev):
    """(origins, directions) of the W x H pinhole rays through the pixel centres, scanline order (row 0 = bottom)."""
    v = lambda a: torch.tensor(list(a), dtype=torch.float64, device=dev)
    s = (torch.arange(W, dtype=torch.float64, device=dev) + 0.5) / W
    t = (torch.arange(H, dtype=torch.float64, device=dev) + 0.5) / H
    d = v(cam.lower_left_corner) + s[None, :, None] * v(cam.horizontal) + t[:, None, None] * v(cam.vertical) - v(cam.origin)
    d = d.reshape(-1, 3).contiguous()
    return v(cam.origin).expand(W * H, 3).contiguous(), d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", default="100,6,11,12")
    ap.add_argument("--features-yardstick", action="store_true")
    args = ap.parse_args()
    import torch  # first: the library then shares torch's HIP runtime (tests/conftest.py)
    torch.cuda.init()
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")
    dev = torch.device("cuda", 0)
    result = {"size": [W, H], "rays": W * H, "warmup": WARMUP, "steps": STEPS, "device": torch.cuda.get_device_name(0),
              "library": rtsr.LIB_PATH, "cases": []}
    for scene_id in [int(x) for x in args.scenes.split(",")]:
        b = rtsr.Builder(1)
        world, cam, bg = b.get_world_cam(scene_id, camera_aspect=W / H)
        flat = b.flatten(world)
        if args.features_yardstick:
            cfg = rtsr.Config.new(W / H, W, 2, 50, 10, seed=1, background=bg)
            prog = flat.upload().progressive(cam, cfg)
            for _ in range(3):
                for spp in (2, 1):  # never the feature_spp the handle holds: the pass runs every call; the trace names both
                    status = rtsr.lib.rtx_progressive_features(prog._p, spp, None, None)
                    if status != rtsr.RTX_OK:
                        raise rtsr.RtxError(status, rtsr.last_error())
            torch.cuda.synchronize()
            print("features: scene %d done (3 x feature_spp 2 then 1: the feature_spp = 1 calls are the 2nd, 4th and 6th k_features)" % scene_id)
            del prog
            continue
        o, d = primary_rays(torch, cam, dev)
        g = torch.Generator(device="cpu")
        g.manual_seed(1)
        perm = torch.randperm(W * H, generator=g).to(dev)
        orders = {"scanline": (o, d), "permuted": (o[perm].contiguous(), d[perm].contiguous())}
        for f32 in (False, True):
            scene = flat.upload(f32=f32)
            for order, (oo, dd) in orders.items():
                for want in (rtsr.RAY_COLUMNS, ("t", "ids")):
                    # the result columns, the argument blocks and Scene.cast_rays' own checks stay outside the timed interval:
                    # one checked call first (it also gives the hit fraction), then the entry point alone between the events
                    h = scene.cast_rays(oo, dd, want=want)
                    batch = rtsr.RtxRayBatch()
                    rtsr.lib.rtx_ray_batch_defaults(C.byref(batch))
                    batch.n, batch.origin, batch.direction = W * H, oo.data_ptr(), dd.data_ptr()
                    hits = rtsr.RtxRayHits(*[getattr(h, c).data_ptr() if c in want else None for c in rtsr.RAY_COLUMNS])
                    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream or None)
                    ms = []
                    for k in range(WARMUP + STEPS):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        status = rtsr.lib.rtx_scene_cast_rays_device(scene.ptr, C.byref(batch), C.byref(hits), stream)
                        e1.record()
                        e1.synchronize()
                        if status != rtsr.RTX_OK:
                            raise rtsr.RtxError(status, rtsr.last_error())
                        if k >= WARMUP:
                            ms.append(e0.elapsed_time(e1))
                    med = statistics.median(ms)
                    case = {"scene": scene_id, "name": NAMES.get(scene_id, str(scene_id)), "precision": "f32" if f32 else "f64",
                            "order": order, "columns": list(want), "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
                            "ms_max": round(max(ms), 4), "mrays_per_s": round(W * H / med / 1e3, 1),
                            "bytes_read_per_ray": 48, "bytes_written_per_ray": sum(BYTES[c] for c in want),
                            "hit_fraction": round(float((h.ids[:, 0] == 1).double().mean()), 4)}
                    result["cases"].append(case)
                    print(json.dumps(case), file=sys.stderr, flush=True)
            del scene
    if not args.features_yardstick:
        text = json.dumps(result, indent=1)
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
