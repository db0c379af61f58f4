"""Clearance of one moving box against the rest of a box field, on ONE upload: set_transforms moves the members, nearest measures.

    python scripts/clearance.py [--steps K] [--n N] [--probe P] [--samples S]

The scene (tests/instance_scenes.py: box_field, N boxes in one instance tree) is flattened and uploaded once.  Every step turns
every box about its own axis and lets the field breathe, as scripts/turntable.py does.  The probe -- box P -- is parked far below
the field in the resident scene, so that "the scene" is everything else; its surface is sampled on the host from the pose it
would have (S points a face, through the same Translate(RotateY(.)) the flattener applies), and Scene.nearest answers how far
each sample is from the rest.  One line per step: the smallest distance, the sample and the slot, kind and primitive that
limit it.  No render."""
import argparse
import importlib
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
KINDS = ("sphere", "moving sphere", "rectangle", "triangle")


def box_samples(lo, hi, per_face, rng):
    """per_face uniform points on the top and the four sides of the box [lo, hi] (its own frame; it stands on the ground), the
    sides from a third of its height up."""
    out = []
    lo = lo + np.array([0.0, (hi[1] - lo[1]) / 3.0, 0.0])
    for axis in range(3):
        for plane in ((hi[axis],) if axis == 1 else (lo[axis], hi[axis])):
            p = lo + rng.uniform(size=(per_face, 3)) * (hi - lo)
            p[:, axis] = plane
            out.append(p)
    return np.concatenate(out)


def to_world(local, offset, degrees):
    """Translate(offset, RotateY(degrees, .)) of points of the inner frame: rotate back, then move (xform_record's p arithmetic)."""
    s, c = math.sin(math.radians(degrees)), math.cos(math.radians(degrees))
    x, z = c * local[:, 0] + s * local[:, 2], -s * local[:, 0] + c * local[:, 2]
    return np.ascontiguousarray(np.column_stack([x, local[:, 1], z]) + np.asarray(offset))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--n", type=int, default=60)
    ap.add_argument("--probe", type=int, default=23)
    ap.add_argument("--samples", type=int, default=64, help="sample points per face of the probe")
    args = ap.parse_args()
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")
    from instance_scenes import box_field

    b, world = box_field(rtsr, "instanced", n=args.n)
    flat = b.flatten(world)
    scene = flat.upload()
    tree = flat.instance_tree(0)
    boxes = [s for s in range(tree["first_slot"], tree["first_slot"] + tree["n_slots"]) if flat.slot_chain(s) == ["translate", "rotate_y"]]
    k_probe = args.probe % len(boxes)
    w = 0.25 + 0.013 * (k_probe % 7)  # box_field's extents of box k
    lo, hi = np.array([-w, 0.0, -w]), np.array([w, 0.3 + 0.05 * (k_probe % 5), w])
    local = box_samples(lo, hi, args.samples, np.random.default_rng(1))
    cols = 10 if args.n <= 60 else int(round(args.n ** 0.5))
    for f in range(args.steps):
        phase = 2.0 * math.pi * f / args.steps
        spread = 1.0 - 0.45 * (0.5 - 0.5 * math.cos(phase))  # the field closes up, then opens again
        updates, pose = {}, None
        for k, slot in enumerate(boxes):
            x = (-4.5 + 1.0 * (k % 10) if args.n <= 60 else -0.5 * cols + 1.0 * (k % cols)) * spread
            z = (-3.0 + 1.0 * (k // 10) if args.n <= 60 else -0.5 * cols + 1.0 * (k // cols)) * spread
            angle = 7.0 + 5.3 * k + 360.0 * f / args.steps
            if k == k_probe:
                pose = ((x, 0.0, z), angle)
            # the probe is parked 2000 units below: not part of what it is measured against
            updates[slot] = [("translate", (x, -2000.0 if k == k_probe else 0.0, z)), ("rotate_y", angle)]
        t0 = time.perf_counter()
        scene.set_transforms(updates)
        near = scene.nearest(to_world(local, *pose), r_max_all=5.0)
        t1 = time.perf_counter()
        if not near.found.any():
            print("step %2d: nothing within 5 units of box %d" % (f, k_probe), flush=True)
            continue
        i = int(np.argmin(near.d))
        print("step %2d: box %d clears the rest by %.6f at sample %d, limited by slot %d (%s %d) at (%.4f, %.4f, %.4f); %d boxes moved and %d "
              "points asked in %.2f ms" % (f, k_probe, near.d[i], i, near.slot[i], KINDS[near.prim_type[i]], near.prim_index[i], *near.q[i],
                                           len(boxes), near.n, 1e3 * (t1 - t0)), flush=True)


if __name__ == "__main__":
    main()
