"""Relighting on ONE upload: a Cornell room whose light changes colour while the fog in it thins, frame by frame.

    python scripts/relight.py [--frames N] [--width W] [--spp S] [--out-dir DIR] [--check]

The room -- five walls, a rectangle light, a glass ball and a block of fog -- is built, flattened and uploaded once.  Every
frame hands Scene.set_shading the light's new colour and the fog's new density (one small copy and one small kernel; the light
table of next-event estimation follows on the device) and renders a short progressive frame with light sampling, denoised.
Nothing else crosses to the GPU.  A progressive handle holds the samples and features of the look it was made under, so every
frame makes a new one.  Writes frame_000.ppm ... into --out-dir (default: a temporary directory, printed) and one line per
frame with the edit's and the frame's wall time.

--check: the last frame (its samples AND its denoised image) is compared, bit for bit, with the same frame on a room built
from scratch with the last values; exit status 1 when they differ.
"""
import argparse
import importlib
import math
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def room(rtsr, light_rgb, density):
    """-> (builder, world, the light's texture, the fog's slot)."""
    b = rtsr.Builder(1)
    white, red, green = b.lambertian((0.73, 0.73, 0.73)), b.lambertian((0.65, 0.05, 0.05)), b.lambertian((0.12, 0.45, 0.15))
    emit = b.solid_color(light_rgb)
    objs = [b.yz_rect(0.0, 555.0, 0.0, 555.0, 555.0, green), b.yz_rect(0.0, 555.0, 0.0, 555.0, 0.0, red),
            b.xz_rect(163.0, 393.0, 177.0, 382.0, 554.0, b.diffuse_light(emit)), b.xz_rect(0.0, 555.0, 0.0, 555.0, 0.0, white),
            b.xz_rect(0.0, 555.0, 0.0, 555.0, 555.0, white), b.xy_rect(0.0, 555.0, 0.0, 555.0, 555.0, white),
            b.sphere((190.0, 90.0, 190.0), 90.0, b.dielectric(1.5))]
    block = b.translate((265.0, 0.0, 295.0), b.rotate_y(15.0, b.rect_prism((0.0, 0.0, 0.0), (165.0, 330.0, 165.0), white)))
    fog_slot = len(objs)
    objs.append(b.constant_medium((0.9, 0.9, 0.95), density, block))
    return b, b.hittable_list(objs), emit, fog_slot


def look(f, frames):
    """The light's colour and the fog's density at frame f: warm and thick to cool and thin."""
    s = f / max(frames - 1, 1)
    warm, cool = np.array([17.0, 12.0, 6.0]), np.array([6.0, 10.0, 17.0])
    return tuple(float(x) for x in (1.0 - s) * warm + s * cool), 0.012 * math.exp(-2.5 * s)


def frame(scene, cam, cfg, spp):
    """A short progressive frame with light sampling, then the denoiser -> (the samples' screen, the denoised screen)."""
    p = scene.progressive(cam, cfg, light_sampling=True)
    p.add(spp)
    return p.screen(), p.denoise()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--width", type=int, default=240)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--check", action="store_true", help="compare the last frame with a room built from scratch with the last values")
    args = ap.parse_args()
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")

    rgb0, d0 = look(0, args.frames)
    b, world, emit, fog_slot = room(rtsr, rgb0, d0)
    flat = b.flatten(world)
    scene = flat.upload()
    cam = rtsr.Camera.new((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    cfg = rtsr.Config.new(1.0, args.width, args.spp, 30, 4, seed=7, background=(0.0, 0.0, 0.0))
    out_dir = args.out_dir or tempfile.mkdtemp(prefix="relight_")
    os.makedirs(out_dir, exist_ok=True)
    raw = den = None
    rgb, density = rgb0, d0
    for f in range(args.frames):
        rgb, density = look(f, args.frames)
        t0 = time.perf_counter()
        scene.set_shading([("solid_color", emit, rgb), ("medium_density", fog_slot, density)])
        t1 = time.perf_counter()
        raw, den = frame(scene, cam, cfg, args.spp)
        t2 = time.perf_counter()
        path = os.path.join(out_dir, "frame_%03d.ppm" % f)
        den.write_to_ppm_file(path)
        print("frame %d: light (%.1f, %.1f, %.1f), density %.4f set in %.2f ms (call), frame in %.1f ms -> %s" % (
            f, rgb[0], rgb[1], rgb[2], density, 1e3 * (t1 - t0), 1e3 * (t2 - t1), path), flush=True)
    if args.check:
        fb, fworld, _, _ = room(rtsr, rgb, density)
        fresh = fb.flatten(fworld).upload()
        fraw, fden = frame(fresh, cam, cfg, args.spp)
        same = (np.array_equal(raw.accum, fraw.accum) and np.array_equal(raw.rgb8, fraw.rgb8) and np.array_equal(den.accum, fden.accum) and
                np.array_equal(den.rgb8, fden.rgb8))
        print("check: the last frame %s the frame of a room built from scratch with the last values" % ("equals, bit for bit," if same else "DIFFERS from"), flush=True)
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
