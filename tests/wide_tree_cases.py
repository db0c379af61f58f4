"""Trees for the audit of the 4-wide collapse (csrc/host/wide_tree.hpp): flattened scenes and a few hand-made node arrays.

A case is a dict: nodes / nodes32 (structured numpy arrays of the f64 FlatNode and of FlatNode32), roots (the ENTRY_BVH
records' roots, leaf codes included) and, for a scene, the builder / world / flat it came from.  tests/test_wide_tree.py audits
the records tests/wide_tree_host_check.cpp makes of them; tests/test_gpu_cull_steps.py compares the resident tree with those."""
import os
import subprocess

import numpy as np

import lbvh_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NODE = np.dtype([("bmin", "<f8", (2, 3)), ("bmax", "<f8", (2, 3)), ("child", "<i4", (2,)), ("pad", "<i4", (2,))])
NODE32 = np.dtype([("lo", "<f4", (2, 3)), ("hi", "<f4", (2, 3)), ("child", "<i4", (2,)), ("axis", "<i4"), ("pad", "<i4")])
NODE4 = np.dtype([("lo", "<f4", (3, 4)), ("hi", "<f4", (3, 4)), ("child", "<i4", (4,)), ("pad", "<i4", (4,))])
ENTRY_HEAD = np.dtype([("kind", "<i4"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4")])
assert (NODE.itemsize, NODE32.itemsize, NODE4.itemsize) == (112, 64, 128)
ENTRY_BVH = 2
EMPTY = 0x7FFFFFFF


def make_leaf(first, count):
    return int(np.int32(np.uint32(0x80000000 | (first << 3) | (count - 1))))


def round_out(lo64, hi64):
    """Outward rounding to f32 from its definition: the largest float <= lo, the smallest float >= hi (NaN stays NaN)."""
    with np.errstate(over="ignore", invalid="ignore"):
        lo = lo64.astype(np.float32)
        hi = hi64.astype(np.float32)
    lo = np.where(lo.astype(np.float64) > lo64, np.nextafter(lo, np.float32(-np.inf)), lo)
    hi = np.where(hi.astype(np.float64) < hi64, np.nextafter(hi, np.float32(np.inf)), hi)
    return lo.astype(np.float32), hi.astype(np.float32)


def nodes32_of(nodes):
    out = np.zeros(len(nodes), dtype=NODE32)
    out["lo"], out["hi"] = round_out(nodes["bmin"], nodes["bmax"])
    out["child"] = nodes["child"]
    out["axis"] = nodes["pad"][:, 0]
    return out


def from_flat(b, world, flat):
    entries = flat.array("entries").reshape(-1, 160)
    head = entries[:, :16].copy().view(ENTRY_HEAD).reshape(-1)
    roots = [int(e["a"]) for e in head if e["kind"] == ENTRY_BVH]
    return {"nodes": flat.array("nodes").view(NODE), "nodes32": flat.array("nodes32").view(NODE32), "roots": roots,
            "builder": b, "world": world, "flat": flat}


def _lbvh(case_id):
    def make(rtsr):
        b, world, cam, cfg, _ = lbvh_cases.build(rtsr, case_id)
        c = from_flat(b, world, b.flatten(world, max_leaf=lbvh_cases.CASES[case_id][2][0]))
        c["cam"], c["cfg"] = cam, cfg
        return c
    return make


def _catalogue(sid, max_leaf=0, **opts):
    def make(rtsr):
        b = rtsr.Builder(1)
        world, cam, bg = b.get_world_cam(sid, **opts)
        c = from_flat(b, world, b.flatten(world, max_leaf=max_leaf))
        c["cam"], c["background"] = cam, bg
        return c
    return make


def _spheres(b, n, seed, centre, mats, spread=6.0):
    rng = np.random.default_rng(seed)
    return [b.sphere(tuple(np.array(centre) + spread * (rng.random(3) - 0.5)), 0.1 + 0.2 * float(rng.random()), mats[k % len(mats)])
            for k in range(n)]


def _few(n):
    """One BVH of n spheres, one per leaf: n - 1 inner nodes (1, 2, 3: a wide root of 2, 3 and 4 slots)."""
    def make(rtsr):
        b = rtsr.Builder(1)
        grey = b.lambertian((0.5, 0.5, 0.5))
        objs = [b.sphere((1.5 * k * k, 0.0, 0.0), 0.5, grey) for k in range(n)]
        world = b.hittable_list([b.bvh_from_list(b.hittable_list(objs), 0.0, 1.0), b.xz_rect(-5, 5, -5, 5, 4.0, b.diffuse_light((4.0, 4.0, 4.0)))])
        return from_flat(b, world, b.flatten(world, max_leaf=1))
    return make


def two_bvhs(rtsr):
    b = rtsr.Builder(1)
    mats = [b.lambertian((0.7, 0.3, 0.3)), b.metal((0.8, 0.8, 0.7), 0.1), b.dielectric(1.5)]
    world = b.hittable_list([b.bvh_from_list(b.hittable_list(_spheres(b, 150, 1, (-4.0, 0.0, 0.0), mats)), 0.0, 1.0),
                             b.bvh_from_list(b.hittable_list(_spheres(b, 170, 2, (4.0, 0.0, 0.0), mats)), 0.0, 1.0),
                             b.xz_rect(-8, 8, -8, 8, 6.0, b.diffuse_light((4.0, 4.0, 4.0)))])
    return from_flat(b, world, b.flatten(world))


def two_triangle_bvh(rtsr):
    """A BVH of two triangles -- no more than max_leaf, which is 2 where triangles are -- beside a BVH of 300 spheres, whose 299
    nodes make plan_wide choose the wide tree without being told to.  build_bvh (host/bvh_build.cpp) lowers max_leaf to n - 1
    for such a BVH "so the root is a node", a list of fewer than two primitives becomes a group, the reference's rule makes a
    node for any span and the GPU builder starts at 1024 primitives: no flattened scene has a leaf code for a BVH root, and this
    case pins that (build_wide_nodes still returns at once for one; wide_tree_host_check's own run covers it)."""
    b = rtsr.Builder(1)
    mats = [b.lambertian((0.7, 0.3, 0.3)), b.metal((0.8, 0.8, 0.7), 0.1), b.lambertian((0.2, 0.4, 0.8))]
    tris = [b.triangle((-3.0, -2.0, 2.5), (3.0, -2.0, 2.5), (0.0, 2.5, 2.0), mats[2]),
            b.triangle((-3.0, -2.5, -2.5), (0.0, 2.0, -2.5), (3.0, -2.5, -2.0), mats[0])]
    world = b.hittable_list([b.bvh_from_list(b.hittable_list(tris), 0.0, 1.0),
                             b.bvh_from_list(b.hittable_list(_spheres(b, 300, 3, (0.0, 0.0, 0.0), mats, spread=4.0)), 0.0, 1.0),
                             b.xz_rect(-8, 8, -8, 8, 6.0, b.diffuse_light((4.0, 4.0, 4.0)))])
    c = from_flat(b, world, b.flatten(world))
    c["cam"] = rtsr.Camera.new((0.0, 1.0, 9.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    return c


def _synthetic(children, boxes):
    nodes = np.zeros(len(children), dtype=NODE)
    nodes["child"] = children
    b = np.asarray(boxes, dtype=np.float64)  # (n, 2, 2, 3): node, child, lo / hi, axis
    nodes["bmin"], nodes["bmax"] = b[:, :, 0, :], b[:, :, 1, :]
    return {"nodes": nodes, "nodes32": nodes32_of(nodes), "roots": [0]}


def comb(rtsr, n=120):
    """Node i = (leaf i, node i + 1): the deepest tree of n inner nodes.  The inner child is the larger one at every level, so
    a wide node holds three leaves and the rest of the comb, and the walk's stack grows by three per wide level."""
    children = [(make_leaf(i, 1), i + 1 if i + 1 < n else make_leaf(n, 1)) for i in range(n)]
    third = 1.0 / 3.0  # no float: every plane needs rounding
    boxes = [[[[i * third] * 3, [(i + 0.5) * third] * 3], [[(i + 1) * third] * 3, [(n + 2) * third] * 3]] for i in range(n)]
    return _synthetic(children, boxes)


def ties_and_odd_areas(rtsr):
    """Hand-made: equal areas on both sides (the tie goes to the lower slot), an inner child of area 0 (it still opens), one
    whose area is NaN (inf - inf: it never opens), planes beyond float range and a subnormal one."""
    L = make_leaf
    inf = np.inf
    children = [(1, 2), (3, 4), (5, 6), (L(0, 1), L(1, 1)), (L(2, 1), L(3, 1)), (L(4, 1), L(5, 1)), (7, 8), (L(6, 1), L(7, 1)),
                (L(8, 1), 9), (L(9, 1), L(10, 1))]
    unit = [[0.1, 0.1, 0.1], [1.1, 1.1, 1.1]]
    flat0 = [[0.3, 0.3, 0.3], [0.3, 2.0, 0.3]]          # a segment: area 0
    nan_area = [[-inf, 0.0, 0.0], [inf, 0.0, inf]]      # dx = inf, dy = 0: inf * 0
    huge = [[-1e300, -1e39, 1e-46], [1e300, 1e39, 2e-46]]
    boxes = [[unit, unit], [unit, unit], [flat0, nan_area], [unit, unit], [unit, unit], [unit, unit], [flat0, flat0], [unit, unit],
             [unit, huge], [huge, unit]]
    return _synthetic(children, boxes)


CASES = {
    "same_centroid": _lbvh("same_centroid"), "threshold_1025": _lbvh("threshold_1025"), "odd_cluster": _lbvh("odd_cluster"),
    "coplanar": _lbvh("coplanar"), "collinear": _lbvh("collinear"), "outlier": _lbvh("outlier"),
    "coincident_tris": _lbvh("coincident_tris"), "hollow_shells": _lbvh("hollow_shells"), "movers": _lbvh("movers"),
    "chain_12": _lbvh("chain_12"),
    "dragon_2000": _catalogue(11, mesh_triangles=2000), "dragon_20000": _catalogue(11, mesh_triangles=20000),
    "book2_final": _catalogue(6), "book1_head_moving": _catalogue(13),
    "two_bvhs": two_bvhs, "inner_1": _few(2), "inner_2": _few(3), "inner_3": _few(4),
    "comb": comb, "ties_and_odd_areas": ties_and_odd_areas, "two_triangle_bvh": two_triangle_bvh,
}
_built = {}


def case(rtsr, case_id):
    """Built once per process; callers do not write into it."""
    if case_id not in _built:
        _built[case_id] = CASES[case_id](rtsr)
    return _built[case_id]


def build_host_check(directory, name="wide_tree_host_check"):
    exe = os.path.join(str(directory), name)
    if not os.path.exists(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe], check=True)
    return exe


SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:verify_asan_link_order=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}


def run_host_check(exe, directory, tag, nodes, roots):
    """(wide records, levels) of build_wide_tree on these nodes, run under the sanitizers."""
    src, dst = os.path.join(str(directory), tag + ".in"), os.path.join(str(directory), tag + ".out")
    with open(src, "wb") as f:
        f.write(np.array([len(nodes), len(roots)] + list(roots), dtype="<i4").tobytes())
        f.write(np.ascontiguousarray(nodes).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True, env=dict(os.environ, **SAN_ENV), timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "wide tree host check clean" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    raw = np.fromfile(dst, dtype=np.uint8)
    levels = int(raw[:4].view("<i4")[0])
    return raw[4:].view(NODE4).copy(), levels


def worst_below(wide, roots):
    """For every wide node a walk reaches: the most entries its stack can hold when the node becomes the current item (a step
    with nh hits leaves nh - 1 of them stacked; the node may be any of them)."""
    below = {}
    for root in roots:
        if root < 0:
            continue
        below[root] = 0
        todo = [root]
        while todo:
            i = todo.pop()
            kids = [int(c) for c in wide["child"][i] if c != EMPTY]
            for c in kids:
                if c >= 0:
                    below[c] = below[i] + len(kids) - 1
                    todo.append(c)
    return below
