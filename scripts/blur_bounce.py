"""Book-1 at HEAD with its movers hopping, motion-blurred: one resident scene, one Scene.set_moving_spheres per frame, no
re-flatten, no upload.

    python scripts/blur_bounce.py [--frames 6] [--width 240] [--spp 8] [--out-dir DIR] [--check]

The scene is catalogue scene 13 (its small spheres are MovingSpheres that rise during the shutter, in one BvhNode with the
ground; k_trace_lds renders it through its time-aware boxes).  A MovingSphere's c0 / c1 are its centre at time0 / time1, here
the shutter's open and close: every frame torch computes, ON THE GPU and on a side stream, where every mover is when the
shutter of that frame opens and where it is when it closes -- each hops on the spot with a height and a phase of its own, and
every 7th drifts sideways as well, which takes the scene out of k_trace_lds's y-only instantiation -- and hands both poses to
rtx_scene_set_moving_spheres_device on that stream.  The BVH and its time-aware boxes are refitted on the device; the frame is
rendered after the stream has been waited for (Scene.render takes no stream).

--check: the LAST frame is compared, bit for bit, with the same catalogue scene flattened again, given the last frame's values
on the host (rtx_flat_set_moving_spheres, which the test suite holds to a flatten from scratch) and uploaded afresh.  The
catalogue draws the scene from its own random stream, so "from scratch with other values" cannot be spelled through the builder.
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
MOVER = np.dtype([("c0", np.float64, (3,)), ("c1", np.float64, (3,)), ("time0", np.float64), ("time1", np.float64), ("radius", np.float64),
                  ("mat", np.int32), ("pad", np.int32)])
SHUTTER = 0.35  # of a frame's time the shutter stays open


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

    def book1_head():
        b = rtsr.Builder(1)
        world, cam, bg = b.get_world_cam(rtsr.SCENE_BOOK1_HEAD)
        return b, world, cam, bg, b.flatten(world)

    b, world, cam, bg, flat = book1_head()
    cfg = rtsr.Config.new(16.0 / 9.0, args.width, args.spp, 50, 4, seed=1, background=bg)
    scene = flat.upload()
    mov = flat.array("moving_spheres").view(MOVER)
    ids = flat.moving_sphere_ids(b, world)
    rng = np.random.default_rng(7)
    side = torch.cuda.Stream()
    d_ground = torch.from_numpy(np.ascontiguousarray(mov["c0"][ids])).cuda()   # where each mover stands
    d_radius = torch.from_numpy(np.ascontiguousarray(mov["radius"][ids])).cuda()
    d_height = torch.from_numpy(rng.uniform(0.15, 0.6, len(ids))).cuda()
    d_phase = torch.from_numpy(rng.uniform(0.0, math.pi, len(ids))).cuda()
    d_drift = torch.from_numpy(0.25 * (np.arange(len(ids)) % 7 == 0).astype(np.float64)).cuda()
    torch.cuda.synchronize()
    print("blur_bounce: %d movers, %d frames of %d x %d at %d spp" % (len(ids), args.frames, args.width, rtsr.image_height(cfg), args.spp))

    def pose(t):
        c = d_ground.clone()
        c[:, 1] += d_height * torch.abs(torch.sin(d_phase + 2.0 * math.pi * t))
        c[:, 0] += d_drift * math.sin(2.0 * math.pi * t)
        return c

    screen, d_vals = None, None
    for f in range(args.frames):
        t_open = (f + 1) / max(args.frames, 1)
        t_close = t_open + SHUTTER / max(args.frames, 1)
        t0 = time.perf_counter()
        with torch.cuda.stream(side):
            d_vals = torch.cat([pose(t_open), pose(t_close), d_radius[:, None]], dim=1).contiguous()
            scene.set_moving_spheres(ids, d_vals, stream=side)
        t1 = time.perf_counter()
        side.synchronize()
        screen = scene.render(cam, cfg, want_stats=True)
        t2 = time.perf_counter()
        print("frame %d: update enqueued in %.3f ms, frame in %.1f ms (%s, variant %d)" % (
            f, 1e3 * (t1 - t0), 1e3 * (t2 - t1), rtsr.trace_kernel_name(screen.stats.trace_kernel), screen.stats.trace_variant))
        if args.out_dir:
            os.makedirs(args.out_dir, exist_ok=True)
            screen.write_to_ppm_file(os.path.join(args.out_dir, "frame_%03d.ppm" % f))
    if args.check:
        if screen is None:
            print("check: no frame was rendered")
            return 1
        b2, world2, cam2, bg2, flat2 = book1_head()
        flat2.set_moving_spheres(ids, d_vals.cpu().numpy())
        want = flat2.upload().render(cam2, cfg, want_stats=True)
        same = bool(np.array_equal(screen.accum, want.accum) and np.array_equal(screen.rgb8, want.rgb8) and screen.stats.trace_variant == want.stats.trace_variant)
        print("check: last frame %s the scene flattened again with the last values" % ("EQUALS, bit for bit," if same else "DIFFERS from"))
        return 0 if same else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
