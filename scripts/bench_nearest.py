"""Nearest-point queries (rtx_scene_nearest_device) at 2^22 points, beside the ids-only closest-hit cast of as many rays.

    python scripts/bench_nearest.py [--out profiles/nearest/bench_nearest.json] [--cases book1,mesh_inside,mesh_far,zoo] [--points 4194304]

Cases:
  book1        scene 100 (Book-1 final: a BVH of spheres on a ground sphere), points uniform in the box of the small spheres;
  mesh_inside  scene 11 (the mesh room, 871 200 triangles), points uniform in the box of the mesh's vertices;
  mesh_far     the same scene, the same points carried 10 diagonals of that box away along (1, 1, 1);
  zoo          the instance zoo of tests/instance_scenes.py (box_field, 1024 members in one instance tree), points uniform over it.
In the same run, as context: k_cast_rays (ids only) of as many rays from the same points, directions uniform on the sphere
(torch's generator, seed 2).  f64 and f32 scenes.  Method as scripts/bench_occlusion.py: columns allocated beforehand, 2 warm-up
calls, then 7 timed ones, each the device entry alone between two HIP events on torch's current stream; median, min and max.
Output: one JSON document on stdout and, with --out, in a file."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_cast_rays import STEPS, WARMUP  # noqa: E402
from bench_occlusion import timed  # noqa: E402


def mesh_box(flat):
    v = np.frombuffer(flat.array("triangles"), dtype=np.float64).reshape(-1, 13)[:, :9].reshape(-1, 3)
    return v.min(axis=0), v.max(axis=0)


def build_case(rtsr, name):
    """-> (flat, lo, hi, shift): points are uniform in [lo, hi], then moved by shift."""
    if name == "book1":
        b = rtsr.Builder(1)
        world, _, _ = b.get_world_cam(100)
        return b.flatten(world), np.array([-11.0, 0.0, -11.0]), np.array([11.0, 3.0, 11.0]), np.zeros(3)
    if name in ("mesh_inside", "mesh_far"):
        b = rtsr.Builder(1)
        world, _, _ = b.get_world_cam(11)
        flat = b.flatten(world)
        lo, hi = mesh_box(flat)
        far = 10.0 * np.linalg.norm(hi - lo) / np.sqrt(3.0) if name == "mesh_far" else 0.0
        return flat, lo, hi, np.full(3, far)
    from instance_scenes import box_field
    b, world = box_field(rtsr, "instanced", n=1024)
    return b.flatten(world), np.array([-17.0, 0.0, -17.0]), np.array([17.0, 2.0, 17.0]), np.zeros(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="book1,mesh_inside,mesh_far,zoo")
    ap.add_argument("--points", type=int, default=1 << 22)
    args = ap.parse_args()
    import torch  # first: the library then shares torch's HIP runtime (tests/conftest.py)
    torch.cuda.init()
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")
    dev = torch.device("cuda", 0)
    n = args.points
    g = torch.Generator(device="cpu")
    g.manual_seed(2)
    unit = torch.rand((n, 3), generator=g, dtype=torch.float64)
    dirs = torch.randn((n, 3), generator=g, dtype=torch.float64)
    dirs = (dirs / dirs.norm(dim=1, keepdim=True)).to(dev).contiguous()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream or None)
    cases = []
    for name in args.cases.split(","):
        flat, lo, hi, shift = build_case(rtsr, name)
        pts = (torch.from_numpy(lo) + unit * torch.from_numpy(hi - lo) + torch.from_numpy(shift)).to(dev).contiguous()
        info = flat.info()
        for f32 in (False, True):
            scene = flat.upload(f32=f32)
            ans = scene.nearest(pts)  # one checked call first
            ids = scene.cast_rays(pts, dirs, want=("ids",)).ids
            batch = rtsr.RtxPointBatch()
            rtsr.lib.rtx_point_batch_defaults(C.byref(batch))
            batch.n, batch.points = n, pts.data_ptr()
            out = rtsr.RtxNearest(ans.d.data_ptr(), ans.q.data_ptr(), ans.ids.data_ptr())
            rays = rtsr.RtxRayBatch()
            rtsr.lib.rtx_ray_batch_defaults(C.byref(rays))
            rays.n, rays.origin, rays.direction = n, pts.data_ptr(), dirs.data_ptr()
            hits = rtsr.RtxRayHits(None, None, None, None, ids.data_ptr())
            t_near = timed(torch, lambda: rtsr.lib.rtx_scene_nearest_device(scene.ptr, C.byref(batch), C.byref(out), stream))
            t_cast = timed(torch, lambda: rtsr.lib.rtx_scene_cast_rays_device(scene.ptr, C.byref(rays), C.byref(hits), stream))
            case = {"case": name, "precision": "f32" if f32 else "f64", "points": n,
                    "primitives": info["n_spheres"] + info["n_moving_spheres"] + info["n_rects"] + info["n_triangles"],
                    "nearest": t_near, "nearest_mqueries_per_s": round(n / t_near["ms_median"] / 1e3, 2),
                    "cast_ids_only": t_cast, "cast_mrays_per_s": round(n / t_cast["ms_median"] / 1e3, 2),
                    "found_fraction": round(float(ans.found.double().mean()), 4), "mean_distance": round(float(ans.d.mean()), 4),
                    "cast_hit_fraction": round(float((ids[:, 0] == 1).double().mean()), 4)}
            print(json.dumps(case), file=sys.stderr, flush=True)
            cases.append(case)
            del scene
    result = {"warmup": WARMUP, "steps": STEPS, "device": torch.cuda.get_device_name(0), "cases": cases}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
