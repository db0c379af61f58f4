"""Book-1 final with its small spheres bobbing: one resident scene, one Scene.set_spheres per frame, no re-flatten, no upload.

    python scripts/bounce.py [--frames 6] [--width 240] [--spp 8] [--out-dir DIR] [--check]

The scene is catalogue scene 100 (484 spheres and the ground in one BvhNode; k_trace_lds renders it).  Every frame the centres
of the small spheres are computed by torch ON THE GPU, on a side stream, and handed to rtx_scene_set_spheres_device on that
stream: each small sphere hops on the spot with a height and a phase of its own, and every 5th one breathes (its radius swings
by 30 %).  The BVH is refitted on the device; the frame is rendered after the stream has been waited for (Scene.render takes
no stream).

--check: the LAST frame is compared, bit for bit, with the same catalogue scene flattened again, given the last frame's values
on the host (rtx_flat_set_spheres, which the test suite holds to a flatten from scratch) and uploaded afresh.  The catalogue
draws the scene from its own random stream, so "from scratch with other values" cannot be spelled through the builder.
"""
import argparse
import importlib
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SPHERE = np.dtype([("c", np.float64, (3,)), ("radius", np.float64), ("mat", np.int32), ("pad", np.int32)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--width", type=int, default=240)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--out-dir", default=None, help="write frame_%%03d.ppm here")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import torch
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")

    def book1():
        b = rtsr.Builder(1)
        world, cam, bg = b.get_world_cam(rtsr.SCENE_BOOK1_CANONICAL)
        return b, world, cam, bg, b.flatten(world)

    b, world, cam, bg, flat = book1()
    cfg = rtsr.Config.new(3.0 / 2.0, args.width, args.spp, 50, 4, seed=1, background=bg)
    scene = flat.upload()
    sph = flat.array("spheres").view(SPHERE)
    ids = np.array([i for i in flat.sphere_ids(b, world) if abs(sph["radius"][i]) < 0.5], dtype=np.int32)
    rest = np.column_stack([sph["c"][ids], sph["radius"][ids]])
    rng = np.random.default_rng(7)
    side = torch.cuda.Stream()
    d_rest = torch.from_numpy(rest).cuda()
    d_height = torch.from_numpy(rng.uniform(0.15, 0.6, len(ids))).cuda()
    d_phase = torch.from_numpy(rng.uniform(0.0, math.pi, len(ids))).cuda()
    d_breathes = torch.from_numpy((np.arange(len(ids)) % 5 == 0).astype(np.float64)).cuda()
    torch.cuda.synchronize()
    print("bounce: %d of %d spheres move, %d frames of %d x %d at %d spp" % (len(ids), len(sph), args.frames, args.width, rtsr.image_height(cfg), args.spp))
    screen, d_vals = None, None
    for f in range(args.frames):
        t = (f + 1) / max(args.frames, 1)
        t0 = time.perf_counter()
        with torch.cuda.stream(side):
            d_vals = d_rest.clone()
            d_vals[:, 1] += d_height * torch.abs(torch.sin(d_phase + 2.0 * math.pi * t))
            d_vals[:, 3] *= 1.0 + 0.3 * d_breathes * math.sin(2.0 * math.pi * t + 0.4)
            scene.set_spheres(ids, d_vals, stream=side)
        t1 = time.perf_counter()
        side.synchronize()
        screen = scene.render(cam, cfg, want_stats=True)
        t2 = time.perf_counter()
        print("frame %d: update enqueued in %.3f ms, frame in %.1f ms (%s)" % (f, 1e3 * (t1 - t0), 1e3 * (t2 - t1), rtsr.trace_kernel_name(screen.stats.trace_kernel)))
        if args.out_dir:
            os.makedirs(args.out_dir, exist_ok=True)
            screen.write_to_ppm_file(os.path.join(args.out_dir, "frame_%03d.ppm" % f))
    if args.check:
        if screen is None:
            print("check: no frame was rendered")
            return 1
        b2, world2, cam2, bg2, flat2 = book1()
        flat2.set_spheres(ids, d_vals.cpu().numpy())
        want = flat2.upload().render(cam2, cfg)
        same = bool(np.array_equal(screen.accum, want.accum) and np.array_equal(screen.rgb8, want.rgb8))
        print("check: last frame %s the scene flattened again with the last values" % ("EQUALS, bit for bit," if same else "DIFFERS from"))
        return 0 if same else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
