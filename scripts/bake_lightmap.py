"""A light map of the Cornell box's floor with gather queries: an example of Scene.gather's surface form.

    python scripts/bake_lightmap.py [--texels 128] [--spp 256] [--depth 8] [--albedo 0.73] [--out lightmap.ppm]

One texel centre per cell of the floor y = 0, 0 <= x, z <= 555, the normal (0, 1, 0).  A gather returns sum / spp = E / pi, the
radiosity of a WHITE diffuse texel; the floor's own albedo is the caller's multiplication.  The map is baked twice -- with the
reference's estimator and with light sampling -- and both halves are written side by side (reference left) as one binary PPM,
gamma 2 as the renderer's tone map, x to the right and z upwards.  Prints each half's mean irradiance and mean relative
standard error from the returned sumsq: with light sampling the same spp resolves the map about an order of magnitude better.
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texels", type=int, default=128)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--albedo", type=float, default=0.73)
    ap.add_argument("--out", default="lightmap.ppm")
    args = ap.parse_args()
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")
    t, spp = args.texels, args.spp
    b = rtsr.Builder(1)
    world, cam, _ = b.get_world_cam(rtsr.SCENE_CORNELL_BOX)
    scene = b.flatten(world).upload()
    c = (np.arange(t) + 0.5) * (555.0 / t)
    p = np.ascontiguousarray(np.stack([np.tile(c, t), np.zeros(t * t), np.repeat(c, t)], axis=1))  # row = z, column = x
    n = np.ascontiguousarray(np.tile([0.0, 1.0, 0.0], (t * t, 1)))
    halves = []
    for light_sampling in (False, True):
        g = scene.gather(p, n, spp=spp, max_depth=args.depth, background=(0.0, 0.0, 0.0), light_sampling=light_sampling)
        var_of_mean = np.maximum(g.sumsq - g.sum * g.sum / spp, 0.0) / max(spp - 1, 1) / spp
        rel = np.sqrt(var_of_mean).mean() / max(g.mean.mean(), 1e-300)
        print("light sampling %d: mean irradiance %.4f, mean relative standard error %.4f" % (light_sampling, g.irradiance.mean(), rel))
        halves.append((args.albedo * g.mean).reshape(t, t, 3)[::-1])
    image = np.concatenate(halves, axis=1)
    rgb = (255.9 * np.clip(np.sqrt(image), 0.0, 1.0)).astype(np.uint8)
    with open(args.out, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (2 * t, t))
        f.write(rgb.tobytes())
    print("wrote", args.out)


if __name__ == "__main__":
    main()
