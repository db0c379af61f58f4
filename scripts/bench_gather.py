"""Time of gather queries (rtx_scene_gather_device) against what a caller had to do before them: the same directions sent as
explicit rays through rtx_scene_trace_rays_device.

    python scripts/bench_gather.py [--out profiles/gather/bench_gather.json] [--scenes 100,6,5] [--parent-root DIR]
                                   [--compare-item-group P]

Workloads: scenes 100 (Book-1 final), 6 (Book-2 final) and 5 (Cornell smoke); 2^20 points taken from a cast of the camera's
1024 x 1024 pinhole rays through the pixel centres (the hit point and its normal; where a ray misses, the point one direction
vector along it, and where it misses or ends in a medium -- whose hit has no normal -- the reversed unit direction); 64 spp,
depth 50; both forms; f64 scenes with both estimators, f32 scenes with the reference's.  Method: 2 warm-up calls, then 7 timed ones, each entry point alone (sums allocated beforehand, no stats,
no sumsq) between two HIP events on torch's current stream: the interval holds the trace kernel and the reduction.  Median, min,
max.

The yardstick: the n x spp start directions of the same query from rtx_gather_directions (probe form: computed on the host
once per scene and precision; surface form: normal + that unit vector, added on the device -- the same bits), every one an
explicit ray of rtx_scene_trace_rays_device with one sample.  Its ray index is r * spp + s, so its paths are other draws of
the same distribution; the per-point sums the caller would still have to add up are not timed.  --parent-root DIR imports the
package (and its built library) for the yardstick from a checkout of the parent commit at DIR, in a child process of its own;
without it the yardstick runs on this build, whose k_trace_rays is instruction-identical (profiles/gather/isa_identity.txt).

One invocation times, in this order: the gather with the library's own item order; with --compare-item-group P the gather
again on scenes uploaded under RTX_ITEM_GROUP=P (k_gather's pass in groups of P points, core/item_order.hpp; 2^30 is one group,
item g = s_local * n + r); the yardstick; and the first gather once more.  The two runs of the same gather bracket the
yardstick in time, so their difference bounds what drift between the parts of one invocation can be; a ratio that differs
from 1 by less than that shows nothing.

Reported per case: every median, ratio = gather / yardstick for the first and for the repeated gather, and the device bytes of
the inputs and sums either way.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE, SPP, DEPTH = 1024, 64, 50
WARMUP, STEPS = 2, 7
NAMES = {100: "book1_final", 6: "book2_final", 5: "cornell_smoke"}
# (precision is f32?, light sampling)
MODES = ((False, False), (False, True), (True, False))
DEFAULT_ITEM_GROUP = 4  # GATHER_ITEM_GROUP of csrc/hip/queries.inc, for the record only: the library's order is what runs


def load(root):
    sys.path.insert(0, root)
    return importlib.import_module("ray-tracing-series-rust_amd")


def timed(torch, call):
    ms = []
    for k in range(WARMUP + STEPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        if k >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def points_of(torch, rtsr, scene, cam, dev):
    """(p, normal) (n, 3) on the device from a cast of the pinhole rays through the pixel centres."""
    v = lambda a: torch.tensor(list(a), dtype=torch.float64, device=dev)
    s = (torch.arange(SIDE, dtype=torch.float64, device=dev) + 0.5) / SIDE
    d = v(cam.lower_left_corner) + s[None, :, None] * v(cam.horizontal) + s[:, None, None] * v(cam.vertical) - v(cam.origin)
    d = d.reshape(-1, 3).contiguous()
    o = v(cam.origin).expand(SIDE * SIDE, 3).contiguous()
    hits = scene.cast_rays(o, d, want=("p", "normal", "ids"))
    hit = (hits.ids[:, 0] == 1)[:, None]
    p = torch.where(hit, hits.p, o + d).contiguous()
    has_normal = hit & (hits.normal.abs().sum(dim=1, keepdim=True) > 0)  # (a medium's hit carries the normal (0, 0, 0))
    nrm = torch.where(has_normal, hits.normal, -d / d.norm(dim=1, keepdim=True)).contiguous()
    return p, nrm, float(hit.double().mean())


def check(rtsr, status):
    if status != rtsr.RTX_OK:
        raise rtsr.RtxError(status, rtsr.last_error())


def run(args, rtsr, directions, want):
    """want: "gather" or "yardstick" -> the cases of that side, keyed (scene, precision, estimator, form)."""
    import torch
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream or None)
    cases = {}
    n = SIDE * SIDE
    for scene_id in [int(x) for x in args.scenes.split(",")]:
        b = rtsr.Builder(1)
        world, cam, bg = b.get_world_cam(scene_id, camera_aspect=1.0)
        flat = b.flatten(world)
        for f32, nee in MODES:
            scene = flat.upload(f32=f32)
            p, nrm, hit_share = points_of(torch, rtsr, scene, cam, dev)
            u = None
            if want == "yardstick":
                u = torch.from_numpy(directions(n, SPP, f32)).to(dev)  # (n, spp, 3)
                o_all = p[:, None, :].expand(n, SPP, 3).reshape(-1, 3).contiguous()
                sums = torch.empty((n * SPP, 3), dtype=torch.float64, device=dev)
            else:
                sums = torch.empty((n, 3), dtype=torch.float64, device=dev)
            for surface in (True, False):
                key = "%d/%s/%s/%s" % (scene_id, "f32" if f32 else "f64", "light_sampling" if nee else "reference", "surface" if surface else "probe")
                case = {"scene": scene_id, "name": NAMES.get(scene_id, str(scene_id)), "precision": "f32" if f32 else "f64",
                        "estimator": "light_sampling" if nee else "reference", "form": "surface" if surface else "probe",
                        "hit_share": round(hit_share, 4)}
                if want == "gather":
                    q = rtsr.RtxGatherPoints()
                    rtsr.lib.rtx_gather_points_defaults(C.byref(q))
                    q.n, q.position, q.normal, q.samples, q.max_depth = n, p.data_ptr(), nrm.data_ptr() if surface else None, SPP, DEPTH
                    q.background[:] = tuple(bg)
                    q.light_sampling = 1 if nee else 0
                    case.update(timed(torch, lambda: check(rtsr, rtsr.lib.rtx_scene_gather_device(scene.ptr, C.byref(q), sums.data_ptr(), None, stream, None))))
                    case["device_bytes"] = n * (48 if surface else 24) + n * 24
                    case["mean"] = round(float(sums.mean()) / SPP, 6)
                else:
                    dirs = ((nrm[:, None, :] + u) if surface else u).reshape(-1, 3).contiguous()
                    q = rtsr.RtxRadianceRays()
                    rtsr.lib.rtx_radiance_rays_defaults(C.byref(q))
                    q.n, q.origin, q.direction, q.samples, q.max_depth = n * SPP, o_all.data_ptr(), dirs.data_ptr(), 1, DEPTH
                    q.background[:] = tuple(bg)
                    q.light_sampling = 1 if nee else 0
                    case.update(timed(torch, lambda: check(rtsr, rtsr.lib.rtx_scene_trace_rays_device(scene.ptr, C.byref(q), sums.data_ptr(), None, stream, None))))
                    case["device_bytes"] = n * SPP * 48 + n * SPP * 24
                    case["mean"] = round(float(sums.mean()), 6)
                    del dirs
                cases[key] = case
                print(json.dumps(case), file=sys.stderr, flush=True)
            del scene, sums, u
            torch.cuda.empty_cache()
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", default="100,6,5")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--compare-item-group", type=int, default=0)
    ap.add_argument("--yardstick-child", default=None, help=argparse.SUPPRESS)  # the library that has rtx_gather_directions
    args = ap.parse_args()
    import torch  # first: the library then shares torch's HIP runtime (tests/conftest.py)
    torch.cuda.init()
    import numpy as np

    def directions_through(lib, struct):
        def directions(n, spp, f32):
            q = struct()
            lib.rtx_gather_points_defaults(C.byref(q))
            q.n, q.samples = n, spp
            out = np.empty((n, spp, 3))
            if lib.rtx_gather_directions(C.byref(q), 1 if f32 else 0, C.c_void_p(out.ctypes.data)) != 0:
                raise RuntimeError("rtx_gather_directions failed")
            return out
        return directions

    if args.yardstick_child:
        # the parent's package for the rays; this build's library, loaded beside it, only for the host-only direction call
        rtsr = load(args.parent_root)
        new = C.CDLL(args.yardstick_child)
        # the struct's layout without importing a second copy of the package: the fields are fixed by include/rtx_abi.h
        class RtxGatherPoints(C.Structure):
            _fields_ = [("n", C.c_int64), ("position", C.c_void_p), ("normal", C.c_void_p), ("time", C.c_void_p),
                        ("first_point", C.c_uint64), ("first_sample", C.c_uint32), ("samples", C.c_int32), ("max_depth", C.c_int32),
                        ("accumulate", C.c_int32), ("seed", C.c_uint64), ("background", C.c_double * 3),
                        ("light_sampling", C.c_int32), ("sh_order", C.c_int32), ("sample_buffer_bytes", C.c_uint64),
                        ("reserved", C.c_int32 * 2)]
        new.rtx_gather_points_defaults.restype = None
        new.rtx_gather_points_defaults.argtypes = [C.POINTER(RtxGatherPoints)]
        new.rtx_gather_directions.restype = C.c_int32
        new.rtx_gather_directions.argtypes = [C.POINTER(RtxGatherPoints), C.c_int32, C.c_void_p]
        print(json.dumps(run(args, rtsr, directions_through(new, RtxGatherPoints), "yardstick")))
        return
    rtsr = load(ROOT)
    dev_name = torch.cuda.get_device_name(0)
    gathered = run(args, rtsr, None, "gather")
    other = None
    if args.compare_item_group:
        os.environ["RTX_ITEM_GROUP"] = str(args.compare_item_group)  # read at upload
        other = run(args, rtsr, None, "gather")
        del os.environ["RTX_ITEM_GROUP"]
    if args.parent_root:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--scenes", args.scenes, "--parent-root", args.parent_root,
                                "--yardstick-child", rtsr.LIB_PATH], stdout=subprocess.PIPE, check=True, text=True)
        yard = json.loads(child.stdout.strip().split("\n")[-1])
        yard_lib = "the parent commit's build"
    else:
        yard = run(args, rtsr, directions_through(rtsr.lib, rtsr.RtxGatherPoints), "yardstick")
        yard_lib = "this build (k_trace_rays instruction-identical to the parent's)"
    again = run(args, rtsr, None, "gather")
    result = {"points": SIDE * SIDE, "spp": SPP, "max_depth": DEPTH, "warmup": WARMUP, "steps": STEPS, "device": dev_name,
              "order_of_the_parts": ["gather"] + (["gather_item_group_%d" % args.compare_item_group] if other else []) + ["yardstick", "gather_again"],
              "item_group": "the library's default (GATHER_ITEM_GROUP, csrc/hip/queries.inc: %d points)" % DEFAULT_ITEM_GROUP,
              "yardstick_library": yard_lib, "cases": []}
    keys = ("ms_median", "ms_min", "ms_max", "device_bytes", "mean")
    for key, g in gathered.items():
        y, g2 = yard[key], again[key]
        case = {**{k: g[k] for k in ("scene", "name", "precision", "estimator", "form", "hit_share")},
                "gather": {k: g[k] for k in keys}, "gather_again": {k: g2[k] for k in keys}, "yardstick": {k: y[k] for k in keys},
                "ratio": round(g["ms_median"] / y["ms_median"], 4), "ratio_again": round(g2["ms_median"] / y["ms_median"], 4),
                "again_over_first": round(g2["ms_median"] / g["ms_median"], 4)}
        if other:
            case["gather_item_group_%d" % args.compare_item_group] = {k: other[key][k] for k in keys}
            case["ratio_item_group_%d" % args.compare_item_group] = round(other[key]["ms_median"] / y["ms_median"], 4)
        result["cases"].append(case)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
