"""A flag waving over N frames on ONE resident scene (Scene.set_triangles), written as PPMs.

    python scripts/flag.py [--frames 24] [--cells 48] [--width 480] [--spp 32] [--out-dir flag_frames]

The flag is a sheet of 2 x cells x (cells * 2 / 3) triangles in a BvhNode, on a pole beside a ground sphere.  It is flattened
and uploaded once; every frame computes new vertices on the GPU (a travelling wave that grows away from the pole, a torch
expression on the stream) and hands the tensor to rtx_scene_set_triangles_device: no re-flatten, no re-upload, the BVH refitted
in place with its topology kept.  --check renders the last frame once more on a scene built from scratch with the same
vertices and compares the bits.
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sheet(cells):
    nx, ny = cells, max(cells * 2 // 3, 1)
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    v = np.stack([0.05 + 3.0 * gx / nx, 2.0 + 2.0 * gy / ny, np.full(gx.shape, 0.01)], axis=-1).reshape(-1, 3)
    idx = lambda i, j: i * (ny + 1) + j
    faces = []
    for i in range(nx):
        for j in range(ny):
            faces += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return v, np.array(faces, dtype=np.int64)


def build(rtsr, tris):
    b = rtsr.Builder(1)
    cloth, grey, steel = b.lambertian((0.8, 0.15, 0.12)), b.lambertian((0.45, 0.5, 0.45)), b.metal((0.8, 0.8, 0.85), 0.1)
    mesh = b.triangle_mesh(tris.reshape(-1, 3), np.arange(3 * len(tris), dtype=np.int64).reshape(-1, 3), cloth)
    pole = b.rect_prism((-0.05, 0.0, -0.05), (0.05, 4.2, 0.05), steel)
    world = b.hittable_list([b.sphere((0.0, -1000.0, 0.0), 1000.0, grey), pole, b.bvh_from_list(mesh, 0.0, 1.0)])
    return b, world, mesh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--cells", type=int, default=48)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--out-dir", default="flag_frames")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import torch
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")

    v, faces = sheet(args.cells)
    rest = v[faces]
    b, world, mesh = build(rtsr, rest)
    flat = b.flatten(world)
    scene = flat.upload()
    ids = flat.triangle_ids(b, mesh)  # face k of the mesh is triangle ids[k]: asked once, kept
    cam = rtsr.Camera.new((1.2, 2.6, 8.5), (1.5, 2.6, 0.0), (0.0, 1.0, 0.0), 38.0, 1.5, 0.0, 8.5, 0.0, 1.0)
    cfg = rtsr.Config.new(1.5, args.width, args.spp, 20, 4, seed=7)
    os.makedirs(args.out_dir, exist_ok=True)
    stream = torch.cuda.Stream()
    d_rest = torch.from_numpy(rest).cuda()
    torch.cuda.synchronize()
    for f in range(args.frames):
        phase = 2.0 * np.pi * f / args.frames
        with torch.cuda.stream(stream):
            x = d_rest[..., 0]
            d_new = d_rest.clone()
            d_new[..., 2] = d_rest[..., 2] + 0.12 * x * torch.sin(3.0 * x - phase) + 0.03 * x * torch.sin(5.0 * d_rest[..., 1] + 2.0 * phase)
            d_new[..., 1] = d_rest[..., 1] - 0.02 * x * x
            scene.set_triangles(ids, d_new.reshape(-1, 9).contiguous(), stream=stream)
        stream.synchronize()  # Scene.render works on the default stream: ordering between streams is the caller's
        screen = scene.render(cam, cfg)
        path = os.path.join(args.out_dir, "flag_%03d.ppm" % f)
        screen.write_to_ppm_file(path)
        print(path, flush=True)
    if args.check:
        bf, wf, _ = build(rtsr, d_new.cpu().numpy())
        fresh = bf.flatten(wf).upload().render(cam, cfg)
        same = bool(np.array_equal(fresh.accum, screen.accum))
        print("last frame against a scene built from scratch: same bits: %s" % str(same).lower())
        sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
