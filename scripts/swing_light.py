"""The Cornell box with its ceiling light sliding and shrinking: one resident scene, one Scene.set_rects per frame, no re-flatten,
no upload, the render workspace kept.

    python scripts/swing_light.py [--frames 6] [--width 240] [--spp 8] [--out-dir DIR] [--check]

The scene is the Cornell box built by hand (five walls, the XZ ceiling light, two boxes under Translate(RotateY(..))), rendered
with next-event estimation (light_sampling): the light is a sampled light, so every update refreshes the light table on the
device -- its area and pick probability -- beside the record and the slot box.  Every frame the light's a0 a1 b0 b1 k are
computed by torch ON THE GPU, on a side stream, and handed to rtx_scene_set_rects_device on that stream: the light slides
along x on a sine, shrinks to 55 % of its size and comes down from the ceiling a little.  The frame is rendered after the
stream has been waited for (Scene.render takes no stream).

--check: the LAST frame is compared, bit for bit, with the same box built from scratch with the last frame's values for its
light, flattened and uploaded afresh.
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
LIGHT_REST = (213.0, 343.0, 227.0, 332.0, 554.0)  # x0 x1 z0 z1 y


def cornell(rtsr, light_values):
    """-> (builder, world, the light's handle)."""
    b = rtsr.Builder(1)
    red, white, green = b.lambertian((0.65, 0.05, 0.05)), b.lambertian((0.73, 0.73, 0.73)), b.lambertian((0.12, 0.45, 0.15))
    light = b.xz_rect(*[float(v) for v in light_values], b.diffuse_light((15.0, 15.0, 15.0)))
    tall = b.translate((265.0, 0.0, 295.0), b.rotate_y(15.0, b.rect_prism((0.0, 0.0, 0.0), (165.0, 330.0, 165.0), white)))
    short = b.translate((130.0, 0.0, 65.0), b.rotate_y(-18.0, b.rect_prism((0.0, 0.0, 0.0), (165.0, 165.0, 165.0), white)))
    world = b.hittable_list([b.yz_rect(0.0, 555.0, 0.0, 555.0, 555.0, green), b.yz_rect(0.0, 555.0, 0.0, 555.0, 0.0, red), light,
                             b.xz_rect(0.0, 555.0, 0.0, 555.0, 0.0, white), b.xz_rect(0.0, 555.0, 0.0, 555.0, 555.0, white),
                             b.xy_rect(0.0, 555.0, 0.0, 555.0, 555.0, white), tall, short])
    return b, world, light


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

    b, world, light = cornell(rtsr, LIGHT_REST)
    flat = b.flatten(world)
    cam = rtsr.Camera.new((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    cfg = rtsr.Config.new(1.0, args.width, args.spp, 50, 4, seed=1, background=(0.0, 0.0, 0.0))
    scene = flat.upload()
    ids = flat.rect_ids(b, light)
    assert len(ids) == 1 and flat.lights()["n_lights"] == 1
    side = torch.cuda.Stream()
    d_rest = torch.tensor([LIGHT_REST], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    print("swing_light: %d frames of %d x %d at %d spp, next-event estimation" % (args.frames, args.width, rtsr.image_height(cfg), args.spp))
    screen, d_vals = None, None
    for f in range(args.frames):
        t = (f + 1) / max(args.frames, 1)
        t0 = time.perf_counter()
        with torch.cuda.stream(side):
            cx, cz = 0.5 * (d_rest[:, 0] + d_rest[:, 1]), 0.5 * (d_rest[:, 2] + d_rest[:, 3])
            hx, hz = 0.5 * (d_rest[:, 1] - d_rest[:, 0]), 0.5 * (d_rest[:, 3] - d_rest[:, 2])
            shrink = 1.0 - 0.45 * t
            cx = cx + 150.0 * math.sin(2.0 * math.pi * t + 0.5)
            d_vals = torch.stack([cx - shrink * hx, cx + shrink * hx, cz - shrink * hz, cz + shrink * hz, d_rest[:, 4] - 40.0 * t], dim=1).contiguous()
            scene.set_rects(ids, d_vals, stream=side)
        t1 = time.perf_counter()
        side.synchronize()
        screen = scene.render(cam, cfg, want_stats=True, light_sampling=True)
        t2 = time.perf_counter()
        print("frame %d: update enqueued in %.3f ms, frame in %.1f ms (%s)" % (f, 1e3 * (t1 - t0), 1e3 * (t2 - t1), rtsr.trace_kernel_name(screen.stats.trace_kernel)))
        if args.out_dir:
            os.makedirs(args.out_dir, exist_ok=True)
            screen.write_to_ppm_file(os.path.join(args.out_dir, "frame_%03d.ppm" % f))
    if args.check:
        if screen is None:
            print("check: no frame was rendered")
            return 1
        last = d_vals.cpu().numpy()[0]
        b2, world2, _ = cornell(rtsr, last)
        want = b2.flatten(world2).upload().render(cam, cfg, light_sampling=True)
        same = bool(np.array_equal(screen.accum, want.accum) and np.array_equal(screen.rgb8, want.rgb8))
        print("check: last frame %s the box built from scratch with the last values" % ("EQUALS, bit for bit," if same else "DIFFERS from"))
        return 0 if same else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
