"""Scenes and poses for tests/test_rebuild_instances_host.py and tests/test_gpu_rebuild_instances.py (a helper module, not a
test file).

A case is (scene function, pose, trees to rebuild).  The scene is built at the pose its function writes, moved to `pose` with
set_transforms and then rebuilt; the judge is the FRESH scene: the same function run with the pose's values
(tests/set_transforms_cases.py: build).  Sizes count MEMBERS of the tree: box_field(n) has n boxes and one BvhNode of spheres
in its tree, so a tree of m members is box_field(n = m - 1).  Everything here runs on the CPU.
"""
import math
import sys

import numpy as np

from instance_scenes import box_field, member_zoo
from set_transforms_cases import NODE, NODE32, MOTION32, build, narrow, random_values, two_trees, updates_for

SIZES = (2, 3, 64, 65, 257, 1024)


def field(m):
    return lambda r: box_field(r, "instanced", n=m - 1)


def uniform_field(rtsr, n):
    """A ground sphere and ONE tree of n IDENTICAL prisms, symmetric about their own origin in all three axes, each under
    Translate(RotateY(.)): a member's world box is then symmetric about its offset, so the centroid of the box is a function
    of the offset alone (and exactly 0 on an axis where the offset is 0)."""
    b = rtsr.Builder(5)
    m = [b.lambertian((0.8, 0.3, 0.3)), b.metal((0.8, 0.8, 0.9), 0.3), b.lambertian((0.2, 0.7, 0.3))]
    cols = max(int(round(n ** 0.5)), 1)
    members = [b.translate((-0.5 * cols + 1.0 * (k % cols), 0.0, -0.5 * cols + 1.0 * (k // cols)), b.rotate_y(20.0, b.rect_prism((-0.25, -0.25, -0.25), (0.25, 0.25, 0.25), m[k % 3])))
               for k in range(n)]
    return b, b.hittable_list([b.sphere((0.0, -500.5, 0.0), 500.0, m[2]), b.instance_bvh(b.hittable_list(members))])


def _uniform_pose(calls, offset):
    """Every angle stays; member k's offset becomes offset(k)."""
    out, k = [], 0
    for kind, v, _, _ in calls:
        if kind == "translate":
            out.append(tuple(float(x) for x in offset(k)))
            k += 1
        else:
            out.append(v)
    return out


def pose_point(calls):
    """Every member on one point: all Morton codes are equal, the whole tree comes from the index tie-break."""
    return _uniform_pose(calls, lambda k: (1.0, 0.0, 2.0))


def pose_line(calls):
    """Members on a line along x with y = z = 0: two axes have no centroid extent."""
    return _uniform_pose(calls, lambda k: (0.37 * k - 3.0, 0.0, 0.0))


def pose_diagonal(calls):
    """Geometrically shrinking spacing along the x = z diagonal: every Morton bit peels one member off, so the Morton tree is a
    chain where the binned SAH tree takes several members per level."""
    return _uniform_pose(calls, lambda k: (8.0 * 0.5 ** k, 0.0, 8.0 * 0.5 ** k))


def pose_chain63(calls):
    """64 members whose Morton codes have their highest set bit at 63 different places (member 3j + a sits at 2^-j on axis a,
    member 63 at the origin): a chain of 63 nodes, one more than the launchers' stacks hold."""
    def at(k):
        p = [0.0, 0.0, 0.0]
        if k < 63:
            p[k % 3] = 16.0 * 0.5 ** (k // 3)
        return p
    return _uniform_pose(calls, at)


def scramble_values(calls, n_boxes):
    """box_field's scramble pose: box i moves to the grid cell of box pi(i), pi(i) = a i mod n_boxes with a the smallest
    number >= 0.38 n_boxes that is coprime to n_boxes; angles stay."""
    a = max(int(0.38 * n_boxes), 1)
    while math.gcd(a, n_boxes) != 1:
        a += 1
    offsets = [c[1] for c in calls if c[0] == "translate"]
    assert len(offsets) == n_boxes
    out, k = [], 0
    for kind, v, _, _ in calls:
        if kind == "translate":
            out.append(offsets[(a * k) % n_boxes])
            k += 1
        else:
            out.append(v)
    return out


# name -> (scene function, pose(calls) -> values, trees to rebuild or None for all)
CASES = {("size_%d" % m): (field(m), (lambda m: lambda calls: random_values(calls, seed=m, shift=2.5))(m), None) for m in SIZES}
CASES.update({
    "point": (lambda r: uniform_field(r, 33), pose_point, None),
    "line": (lambda r: uniform_field(r, 33), pose_line, None),
    "diagonal": (lambda r: uniform_field(r, 48), pose_diagonal, None),
    "two_trees": (two_trees, lambda calls: random_values(calls, seed=6, shift=1.5), [1]),
    "zoo": (lambda r: member_zoo(r, "instanced", "middle"), lambda calls: random_values(calls, seed=4, shift=2.0), None),
    "scramble": (lambda r: box_field(r, "instanced", n=256), lambda calls: scramble_values(calls, 256), None),
})


# a pose the Morton builder must refuse (64 members; the SAH builder takes it)
REFUSED = {"chain63": (lambda r: uniform_field(r, 64), pose_chain63, None)}


def posed(rtsr, name):
    """-> (flat moved to the case's pose with set_transforms, calls, values, trees, fresh flat at that pose)."""
    fn, pose, trees = CASES[name] if name in CASES else REFUSED[name]
    b, w, calls = build(rtsr, fn)
    flat = b.flatten(w)
    values = pose(calls)
    flat.set_transforms(updates_for(flat, calls, values))
    bf, wf, _ = build(rtsr, fn, values)
    flat._keep = (b, bf)
    return flat, calls, values, trees, bf.flatten(wf)


def camera(rtsr, name):
    """A camera that sees the case's members, and the box its test rays start from."""
    if name in ("point", "line", "diagonal"):
        cam = rtsr.Camera.new((2.0, 5.0, 12.0), (1.0, 0.0, 1.0), (0.0, 1.0, 0.0), 50.0, 1.5, 0.0, 10.0, 0.0, 1.0)
        lo, hi = (-5.0, -1.0, -3.0), (10.0, 4.0, 10.0)
    elif name == "two_trees":
        cam = rtsr.Camera.new((0.5, 3.0, 9.0), (0.0, 0.6, 0.0), (0.0, 1.0, 0.0), 42.0, 1.5, 0.0, 9.0, 0.0, 1.0)
        lo, hi = (-6.0, -0.5, -4.0), (6.0, 4.0, 5.0)
    else:
        m = {"zoo": 60, "scramble": 256}.get(name) or int(name.split("_")[1])
        s = max(m, 60) ** 0.5
        cam = rtsr.Camera.new((0.1 * s, 0.55 * s, 1.05 * s), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0), 42.0, 1.5, 0.0, 1.0 * s, 0.0, 1.0)
        lo, hi = (-0.6 * s - 2.0, -0.5, -0.6 * s - 2.0), (0.6 * s + 2.0, 6.0, 0.6 * s + 2.0)
    cfg = rtsr.Config.new(1.5, 48, 8, 12, 4, seed=11, background=(0.35, 0.4, 0.55))
    return cam, cfg, rtsr.image_height(cfg), lo, hi


# ---- the audit of a tree, in numpy
def instance_records(flat):
    """[(root, first_slot, n_slots)] from the ENTRY_INSTANCE records that close the entry array."""
    e = flat.array("entries").view(np.int32).reshape(-1, 40)
    return [(int(r[1]), int(r[2]), int(r[3])) for r in e if r[0] == 5 and r[1] >= 0]


def member_box(local, ops):
    """core/member_box.hpp: member_box_through_ops restated: local (6,), ops [(op, v[3])] outermost first."""
    b = np.array(local, dtype=np.float64)
    mag = np.abs(b).max()
    for op, v in reversed(ops):
        if op == 0:
            b[:3] += v
            b[3:] += v
            mag = max(mag, np.abs(v).max())
        else:
            s, c = v[0], v[1]
            xs, zs = [], []
            for x in (b[0], b[3]):
                for z in (b[2], b[5]):
                    xs.append(c * x + s * z)
                    zs.append(-s * x + c * z)
            b = np.array([min(xs), b[1], min(zs), max(xs), b[4], max(zs)])
        mag = max(mag, np.abs(b).max())
    pad = mag * 2.0 ** -22
    b[:3] -= pad
    b[3:] += pad
    return b


def member_boxes(flat, tree_index):
    """The world box of every member of tree `tree_index` from member_local_box and the ops now in `entries`."""
    e = flat.array("entries")
    ints, dbl = e.view(np.int32).reshape(-1, 40), e.view(np.float64).reshape(-1, 20)
    top = flat.array("top_level").view(np.int32)
    local = flat.array("member_local_box").view(np.float64).reshape(-1, 6)
    recs = instance_records(flat)
    first = sum(r[2] for r in recs[:tree_index])
    _, first_slot, n_slots = recs[tree_index]
    out = {}
    for m in range(n_slots):
        k = int(top[first_slot + m])
        ops = []
        if ints[k][0] == 3:  # ENTRY_XFORM: kind, a, b, c, then f[2], then 4 ops of {op, pad, v[3]} from byte 32
            for i in range(int(ints[k][2])):
                ops.append((int(ints[k][8 + 8 * i]), dbl[k][5 + 4 * i: 8 + 4 * i].copy()))
        out[first_slot + m] = member_box(local[first + m], ops)
    return out


def audit_tree(flat, tree_index, max_stack_rule=True):
    """Every property a rebuilt tree must have, from the arrays alone.  -> depth."""
    nodes, n32 = flat.array("nodes").view(NODE), flat.array("nodes32").view(NODE32)
    root, first_slot, n_slots = instance_records(flat)[tree_index]
    boxes = member_boxes(flat, tree_index)
    seen_nodes, seen_slots = [], []

    def walk(n, level):
        seen_nodes.append(n)
        lo, hi, depth = [], [], level
        for c in range(2):
            code = int(nodes["child"][n][c])
            if code < 0:
                assert (code & 7) == 0, "a leaf of more than one slot"
                slot = (code & 0x7fffffff) >> 3
                seen_slots.append(slot)
                clo, chi = boxes[slot][:3], boxes[slot][3:]
            else:
                clo, chi, d = walk(code, level + 1)
                depth = max(depth, d)
            assert nodes["bmin"][n][c].tobytes() == np.asarray(clo).tobytes(), (n, c)
            assert nodes["bmax"][n][c].tobytes() == np.asarray(chi).tobytes(), (n, c)
            lo.append(clo)
            hi.append(chi)
        return np.minimum(lo[0], lo[1]), np.maximum(hi[0], hi[1]), depth

    sys.setrecursionlimit(max(sys.getrecursionlimit(), 3000))
    _, _, depth = walk(root, 1)
    assert sorted(seen_slots) == list(range(first_slot, first_slot + n_slots)), "every member in exactly one leaf"
    assert len(seen_nodes) == n_slots - 1 and max(seen_nodes) - min(seen_nodes) + 1 == n_slots - 1, "the nodes are one piece"
    piece = slice(min(seen_nodes), max(seen_nodes) + 1)
    assert np.array_equal(n32["lo"][piece], narrow(nodes["bmin"][piece], up=False)) and np.array_equal(n32["hi"][piece], narrow(nodes["bmax"][piece], up=True))
    assert np.array_equal(n32["child"][piece], nodes["child"][piece]) and np.array_equal(n32["axis"][piece], nodes["pad"][piece][:, 0])
    assert (nodes["pad"][piece][:, 1] == 0).all() and (n32["pad"][piece] == 0).all()
    mo = flat.array("motion32")
    if mo.size:
        mo = mo.view(MOTION32)
        assert np.array_equal(mo["lo0"][piece], n32["lo"][piece]) and np.array_equal(mo["hi0"][piece], n32["hi"][piece])
        assert not mo["dlo"][piece].any() and not mo["dhi"][piece].any()
    return depth


NODE_F32 = np.dtype([("bmin", np.float32, (2, 3)), ("bmax", np.float32, (2, 3)), ("child", np.int32, (2,)), ("pad", np.int32, (2,))])  # FlatNode of an f32 scene


def tree_cost(flat, tree_index):
    """rtx_flat_instance_tree_cost restated (see tree_cost_of)."""
    return tree_cost_of(flat.array("nodes").view(NODE), instance_records(flat)[tree_index][0])


def tree_cost_of(nodes, root):
    """Per node of the tree (ascending index) the two child areas added, summed in that order, over the area of the union of
    the root's two child boxes; areas in f64 from the planes widened, 2 (dx dy + dy dz + dz dx)."""
    todo, members = [root], [root]
    while todo:
        n = todo.pop()
        for c in range(2):
            if nodes["child"][n][c] >= 0:
                todo.append(int(nodes["child"][n][c]))
                members.append(int(nodes["child"][n][c]))

    def area(lo, hi):
        dx, dy, dz = (np.float64(hi[a]) - np.float64(lo[a]) for a in range(3))
        return np.float64(2.0) * (dx * dy + dy * dz + dz * dx)

    total = np.float64(0.0)
    for n in sorted(members):
        total = total + (area(nodes["bmin"][n][0], nodes["bmax"][n][0]) + area(nodes["bmin"][n][1], nodes["bmax"][n][1]))
    lo, hi = np.minimum(nodes["bmin"][root][0], nodes["bmin"][root][1]), np.maximum(nodes["bmax"][root][0], nodes["bmax"][root][1])
    return float(total / area(lo, hi))
