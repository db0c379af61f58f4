"""Occlusion queries (rtx_scene_occlusion_device) beside the ids-only closest-hit cast (rtx_scene_cast_rays_device) on the same rays.

    python scripts/bench_occlusion.py [--out profiles/occlusion/bench_occlusion.json] [--batches primary,ao,shadow] [--scenes 100,6,11,12]

Batches:
  primary  the 1920 x 1080 pinhole rays of scripts/bench_cast_rays.py, in scanline order and in its fixed
           permutation, on scenes 100, 6, 11 and 12, f64 and f32, unbounded;
  ao       on scenes 100 and 11: 4 hemisphere directions (unit vectors from torch's generator, seed 2, flipped to the normal's
           side) per first hit of the primary rays, t_max a tenth of the diagonal of the first hits' bounding box;
  shadow   on scene 4 (the Cornell box): segments from the first hits to the centre of the ceiling light (278, 554, 279.5),
           direction = light - p on [0.001, 1 - 1e-6] (Scene.occlusion_between's interval).
Method, for both entries in the same process: result buffers and argument blocks set up beforehand, 2 warm-up calls, then 7 timed
ones, each the device entry alone between two HIP events on torch's current stream; median, min and max.  Output: one JSON
document on stdout and, with --out, in a file (cases of earlier runs with other --batches / --scenes in that file are kept).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_cast_rays import NAMES, STEPS, WARMUP, H, W, primary_rays  # noqa: E402

NAMES = dict(NAMES)
NAMES[4] = "cornell_box"
LIGHT_CENTRE = (278.0, 554.0, 279.5)


def timed(torch, call):
    ms = []
    for k in range(WARMUP + STEPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        status = call()
        e1.record()
        e1.synchronize()
        if status != 0:
            raise RuntimeError("status %d" % status)
        if k >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def run_case(torch, rtsr, scene, dev, o, d, t_max_all, label):
    n = o.shape[0]
    occ = scene.occlusion(o, d, t_max_all=t_max_all)            # one checked call of each first: the answers' agreement
    ids = scene.cast_rays(o, d, t_max_all=t_max_all, want=("ids",)).ids
    batch = rtsr.RtxRayBatch()
    rtsr.lib.rtx_ray_batch_defaults(C.byref(batch))
    batch.n, batch.origin, batch.direction, batch.t_max_all = n, o.data_ptr(), d.data_ptr(), t_max_all
    hits = rtsr.RtxRayHits(None, None, None, None, ids.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream or None)
    tau = occ.tau
    t_occ = timed(torch, lambda: rtsr.lib.rtx_scene_occlusion_device(scene.ptr, C.byref(batch), C.c_void_p(tau.data_ptr()), stream))
    t_cast = timed(torch, lambda: rtsr.lib.rtx_scene_cast_rays_device(scene.ptr, C.byref(batch), C.byref(hits), stream))
    case = dict(label)
    case.update({"rays": n, "occlusion": t_occ, "cast_ids_only": t_cast,
                 "cast_over_occlusion": round(t_cast["ms_median"] / t_occ["ms_median"], 3),
                 "blocked_fraction": round(float(occ.blocked.double().mean()), 4),
                 "cast_hit_fraction": round(float((ids[:, 0] == 1).double().mean()), 4)})
    print(json.dumps(case), file=sys.stderr, flush=True)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="primary,ao,shadow")
    ap.add_argument("--scenes", default="100,6,11,12")
    args = ap.parse_args()
    import torch  # first: the library then shares torch's HIP runtime (tests/conftest.py)
    torch.cuda.init()
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")
    dev = torch.device("cuda", 0)
    inf = float("inf")
    batches = args.batches.split(",")
    scenes = [int(x) for x in args.scenes.split(",")]
    cases = []
    todo = [(s, "primary") for s in scenes if "primary" in batches]
    todo += [(s, "ao") for s in scenes if "ao" in batches and s in (100, 11)]
    todo += [(4, "shadow")] if "shadow" in batches else []
    for scene_id, kind in todo:
        b = rtsr.Builder(1)
        world, cam, _ = b.get_world_cam(scene_id, camera_aspect=W / H)
        flat = b.flatten(world)
        o, d = primary_rays(torch, cam, dev)
        for f32 in (False, True):
            scene = flat.upload(f32=f32)
            label = {"scene": scene_id, "name": NAMES.get(scene_id, str(scene_id)), "precision": "f32" if f32 else "f64", "batch": kind}
            if kind == "primary":
                g = torch.Generator(device="cpu")
                g.manual_seed(1)
                perm = torch.randperm(W * H, generator=g).to(dev)
                for order, (oo, dd) in (("scanline", (o, d)), ("permuted", (o[perm].contiguous(), d[perm].contiguous()))):
                    cases.append(run_case(torch, rtsr, scene, dev, oo, dd, inf, dict(label, order=order)))
                continue
            first = scene.cast_rays(o, d, want=("p", "normal", "ids"))
            hit = first.ids[:, 0] == 1
            p, normal = first.p[hit], first.normal[hit]
            if kind == "ao":
                g = torch.Generator(device="cpu")
                g.manual_seed(2)
                v = torch.randn((p.shape[0] * 4, 3), generator=g, dtype=torch.float64).to(dev)
                v = v / v.norm(dim=1, keepdim=True)
                nn = normal.repeat_interleave(4, dim=0)
                v = torch.where(((v * nn).sum(dim=1, keepdim=True) < 0), -v, v).contiguous()
                reach = 0.1 * float((p.max(dim=0).values - p.min(dim=0).values).norm())
                cases.append(run_case(torch, rtsr, scene, dev, p.repeat_interleave(4, dim=0).contiguous(), v, reach, dict(label, t_max=reach)))
            else:
                light = torch.tensor(LIGHT_CENTRE, dtype=torch.float64, device=dev)
                cases.append(run_case(torch, rtsr, scene, dev, p.contiguous(), (light - p).contiguous(), 1.0 - 1e-6, dict(label, t_max=1.0 - 1e-6)))
            del scene
    result = {"size": [W, H], "warmup": WARMUP, "steps": STEPS, "device": torch.cuda.get_device_name(0), "cases": cases}
    if args.out and os.path.exists(args.out):
        key = lambda c: (c["scene"], c["precision"], c["batch"], c.get("order"))
        mine = {key(c) for c in cases}
        result["cases"] = [c for c in json.load(open(args.out))["cases"] if key(c) not in mine] + cases
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
