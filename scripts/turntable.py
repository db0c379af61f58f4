"""A turntable on ONE upload: K poses of a box field, each box turning about its own axis while the field breathes in and out.

    python scripts/turntable.py [--frames K] [--n N] [--width W] [--spp S] [--out-dir DIR] [--rebuild-every R [--rebuild-growth G]]

The scene (tests/instance_scenes.py: box_field, N boxes in one instance tree) is flattened and uploaded once.  Every frame
hands Scene.set_transforms the new offset and angle of every box -- one small copy, a scatter and a refit of the tree on the
device -- and renders; nothing else crosses to the GPU.  With --rebuild-every R, every R-th frame asks the resident tree
for its cost (Scene.instance_tree_cost) and, when it has grown by more than the factor --rebuild-growth over the cost right
after the last build, rebuilds the tree on the device for the current pose (Scene.rebuild_instance_trees).  Writes frame_000.ppm ... into --out-dir (default: a temporary
directory, printed) and one line per frame with the update's and the render's wall time.
"""
import argparse
import importlib
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--n", type=int, default=60)
    ap.add_argument("--width", type=int, default=240)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--rebuild-every", type=int, default=0, help="check the tree's cost every R frames and rebuild when it has grown (0: never)")
    ap.add_argument("--rebuild-growth", type=float, default=1.2, help="rebuild when cost > growth x the cost after the last build")
    args = ap.parse_args()
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")
    from instance_scenes import box_field, field_cam_cfg

    b, world = box_field(rtsr, "instanced", n=args.n)
    flat = b.flatten(world)
    scene = flat.upload()
    cam, cfg, _ = field_cam_cfg(rtsr, n=args.n, width=args.width, spp=args.spp)
    tree = flat.instance_tree(0)
    boxes = [s for s in range(tree["first_slot"], tree["first_slot"] + tree["n_slots"]) if flat.slot_chain(s) == ["translate", "rotate_y"]]
    cols = 10 if args.n <= 60 else int(round(args.n ** 0.5))
    out_dir = args.out_dir or tempfile.mkdtemp(prefix="turntable_")
    os.makedirs(out_dir, exist_ok=True)
    built_cost = scene.instance_tree_cost(0) if args.rebuild_every > 0 else 0.0
    for f in range(args.frames):
        phase = 2.0 * math.pi * f / args.frames
        spread = 1.0 + 0.15 * math.sin(phase)
        updates = {}
        for k, slot in enumerate(boxes):
            x = (-4.5 + 1.0 * (k % 10) if args.n <= 60 else -0.5 * cols + 1.0 * (k % cols)) * spread
            z = (-3.0 + 1.0 * (k // 10) if args.n <= 60 else -0.5 * cols + 1.0 * (k // cols)) * spread
            updates[slot] = [("translate", (x, 0.0, z)), ("rotate_y", 7.0 + 5.3 * k + 360.0 * f / args.frames)]
        t0 = time.perf_counter()
        scene.set_transforms(updates)
        note = ""
        if args.rebuild_every > 0 and f % args.rebuild_every == args.rebuild_every - 1:
            cost = scene.instance_tree_cost(0)
            if cost > args.rebuild_growth * built_cost:
                stats = scene.rebuild_instance_trees()
                built_cost = scene.instance_tree_cost(0)
                note = ", tree rebuilt (cost %.2f -> %.2f, depth %d)" % (cost, built_cost, stats["max_depth"])
            else:
                note = ", tree kept (cost %.2f, %.2f after the last build)" % (cost, built_cost)
        t1 = time.perf_counter()
        screen = scene.render(cam, cfg, want_accum=False)
        t2 = time.perf_counter()
        path = os.path.join(out_dir, "frame_%03d.ppm" % f)
        screen.write_to_ppm_file(path)
        print("frame %d: %d boxes moved in %.2f ms (call)%s, rendered in %.1f ms -> %s" % (f, len(boxes), 1e3 * (t1 - t0), note, 1e3 * (t2 - t1), path), flush=True)


if __name__ == "__main__":
    main()
