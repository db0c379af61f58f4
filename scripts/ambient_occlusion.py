"""Ambient occlusion of a catalogue scene with ray queries: an example of Scene.cast_rays + Scene.occlusion.

    python scripts/ambient_occlusion.py [--scene 4] [--width 320] [--height 240] [--k 16] [--reach 0.1] [--out ao.pgm]

First hits of the camera's pinhole rays (cast_rays: p, normal, ids), then k directions per hit on the normal's side (unit vectors
from numpy's generator, seed 1) tested with occlusion over a short reach (a fraction of the diagonal of the first hits' bounding
box).  A pixel's value is the mean transmittance exp(-tau) of its k segments: 1 in the open, 0 in a crease, in between through
fog.  Pixels whose primary ray hits nothing are white.  Writes a binary PGM, top row first.
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
    ap.add_argument("--scene", type=int, default=4)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reach", type=float, default=0.1)
    ap.add_argument("--out", default="ao.pgm")
    args = ap.parse_args()
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")
    w, h, k = args.width, args.height, args.k
    b = rtsr.Builder(1)
    world, cam, _ = b.get_world_cam(args.scene, camera_aspect=w / h)
    scene = b.flatten(world).upload()
    v = lambda a: np.array(list(a), dtype=np.float64)
    s, t = (np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h
    d = v(cam.lower_left_corner) + s[None, :, None] * v(cam.horizontal) + t[:, None, None] * v(cam.vertical) - v(cam.origin)
    d = np.ascontiguousarray(d.reshape(-1, 3))
    o = np.ascontiguousarray(np.broadcast_to(v(cam.origin), d.shape))
    first = scene.cast_rays(o, d, want=("p", "normal", "ids"))
    hit = first.ids[:, 0] == 1
    p, n = first.p[hit], first.normal[hit]
    image = np.ones(w * h)
    if len(p):
        rng = np.random.default_rng(1)
        u = rng.normal(size=(len(p) * k, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        nn = np.repeat(n, k, axis=0)
        u = np.ascontiguousarray(np.where((u * nn).sum(axis=1, keepdims=True) < 0, -u, u))
        reach = args.reach * float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
        occ = scene.occlusion(np.ascontiguousarray(np.repeat(p, k, axis=0)), u, t_max_all=reach)
        image[hit] = np.nan_to_num(occ.transmittance, nan=1.0).reshape(-1, k).mean(axis=1)
        print("%d first hits, %d segments of reach %.4g: %.1f %% blocked, mean transmittance %.4f" %
              (len(p), len(u), reach, 100.0 * occ.blocked.mean(), image[hit].mean()))
    grey = np.clip(np.rint(255.0 * image), 0, 255).astype(np.uint8).reshape(h, w)[::-1]
    with open(args.out, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (w, h))
        f.write(grey.tobytes())
    print("wrote", args.out)


if __name__ == "__main__":
    main()
