"""Worlds for the entry of k_trace_lds's walks (csrc/hip/lds_variant.inc: lds_entry_pair): one
bvh_from_list of spheres each, small enough that a frame of 64 x 42 at 4 spp shows every way a walk can begin.

    ground_2, ground_3, ground_20   a ground sphere (r = 1000) and that many small ones: the root is leaf-first (split "axis" 3,
                                    child 0 the ground's leaf), so walks enter with the ground in hand and the rest stacked
    ground_1                        the ground and ONE sphere: both children of the root are leaves, which the builder never
                                    marks leaf-first (bvh_build.cpp asks for a leaf beside a subtree) -- entered at the root
    eight_equal                     eight equal spheres, no bounding primitive: an ordinary root, entered at the root
    twins                           two spheres with one centre and one radius and a smaller one inside them: the first twin
                                    is the bounding leaf, the second lies below child 1, and every ray meets both at one t
    moving                          a static ground, movers and a few static spheres under a BVH with a time interval

build(rtsr, name) -> (builder, world); camera(rtsr, which, ...) -> RtxCamera; expect_leaf_first(name) says what the root must be.
tests/test_lds_entry_plan.py proves the worlds on the CPU, tests/test_gpu_lds_entry.py runs the device on them."""
import math

GROUND_WORLDS = ("ground_2", "ground_3", "ground_20")
WORLDS = GROUND_WORLDS + ("ground_1", "eight_equal", "twins", "moving")
CAMERAS = ("book1", "up", "grazing")
SKY = (0.7, 0.8, 1.0)
WIDTH, SPP, ASPECT = 64, 4, 1.5  # 64 x 42
THIN_FRAMES = ((1, 1.0), (1, 0.25), (5, 5.0))  # (width, aspect ratio): 1 x 1, 1 x 4, 5 x 1 -- primary rays with u or v = x / 0


def expect_leaf_first(name):
    return name.startswith("ground_") and name != "ground_1" or name in ("twins", "moving")


def _material(b, k):
    col = (0.25 + 0.2 * (k % 4), 0.85 - 0.15 * (k % 5), 0.3 + 0.3 * (k % 3))
    if k % 3 == 0:
        return b.lambertian(col)
    if k % 3 == 1:
        return b.metal(col, 0.05 * (k % 4))
    return b.dielectric(1.5)


def _small(k):
    """Centre and radius of small sphere k: a spiral around the origin, every third one (from the second) lifted above the `up` camera."""
    a, d = 2.4 * k, 0.8 + 0.25 * k
    r = 0.4 if k % 2 == 0 else 0.3
    y = 3.0 + 0.1 * k if k % 3 == 1 else r
    return (d * math.cos(a), y, d * math.sin(a)), r


def build(rtsr, name):
    b = rtsr.Builder(1)
    lst = b.hittable_list()
    ground = lambda m: b.sphere((0.0, -1000.0, 0.0), 1000.0, m)
    if name.startswith("ground_"):
        b.list_add(lst, ground(b.lambertian((0.5, 0.5, 0.5))))
        for k in range(int(name.split("_")[1])):
            c, r = _small(k)
            b.list_add(lst, b.sphere(c, r, _material(b, k)))
    elif name == "eight_equal":
        for k in range(8):
            c = (1.2 * (k & 1) - 0.6, 0.6 + 1.2 * ((k >> 1) & 1), 1.2 * ((k >> 2) & 1) - 0.6)
            b.list_add(lst, b.sphere(c, 0.5, _material(b, k)))
    elif name == "twins":
        # (all three centroids coincide: the builder's median split peels the first of the list off as a leaf of its own, and its
        # box is as big as the box of the other two)
        b.list_add(lst, ground(b.metal((0.9, 0.6, 0.2), 0.0)))
        b.list_add(lst, ground(b.lambertian((0.2, 0.7, 0.3))))
        b.list_add(lst, b.sphere((0.0, -1000.0, 0.0), 990.0, b.lambertian((0.9, 0.1, 0.1))))
    elif name == "moving":
        b.list_add(lst, ground(b.lambertian((0.5, 0.5, 0.5))))
        for k in range(12):
            c, r = _small(k)
            if k % 4 == 3:
                b.list_add(lst, b.sphere(c, r, _material(b, k)))
            else:
                c1 = (c[0], c[1] + 0.3 + 0.05 * k, c[2])
                b.list_add(lst, b.moving_sphere(c, c1, 0.0, 1.0, r, _material(b, k)))
    else:
        raise KeyError(name)
    return b, b.hittable_list([b.bvh_from_list(lst, 0.0, 1.0)])


def camera(rtsr, which, time1=0.0, time2=1.0):
    """book1: Book-1's own.  up: from above the ground straight up, so that no primary ray meets the ground's box (y <= 0).
    grazing: along the ground, a hand's breadth above it."""
    if which == "book1":
        return rtsr.Camera.new((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, ASPECT, 0.1, 10.0, time1, time2)
    if which == "up":
        return rtsr.Camera.new((0.0, 1.0, 0.0), (0.0, 11.0, 0.0), (0.0, 0.0, 1.0), 60.0, ASPECT, 0.0, 10.0, time1, time2)
    if which == "grazing":
        return rtsr.Camera.new((13.0, 0.05, 3.0), (0.0, 0.05, 0.0), (0.0, 1.0, 0.0), 20.0, ASPECT, 0.0, 10.0, time1, time2)
    raise KeyError(which)


def config(rtsr, max_depth, seed=11):
    return rtsr.Config.new(ASPECT, WIDTH, SPP, max_depth, 8, seed=seed, background=SKY)


# ---- the node table of a flat scene, and work items as trace_lds.inc codes them (written out here, independent of the library)
def node_table(flat):
    """(root, [(child0, child1, axis)]) of the world's one BVH, from Flat.array("nodes32") and ("entries")."""
    import numpy as np
    nodes = flat.array("nodes32").view(np.dtype([("lo", "<f4", (2, 3)), ("hi", "<f4", (2, 3)), ("child", "<i4", (2,)), ("axis", "<i4"), ("pad", "<i4")]))
    entries = flat.array("entries").view(np.dtype([("kind", "<i4"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4"), ("rest", "u1", (144,))]))
    top = flat.array("top_level").view("<i4")
    assert len(top) == 1 and entries[top[0]]["kind"] == 2, "one BVH is the whole world"
    return int(entries[top[0]]["a"]), [(int(n["child"][0]), int(n["child"][1]), int(n["axis"])) for n in nodes]


def leaf_item(first_slot, count=1):
    v = 0x8000 | (first_slot << 2) | (count - 1)
    return v - 0x10000  # 16 bits, sign-extended


def node_item(index, axis):
    return (axis << 13) | index


def leaf_code(first_slot, count=1):
    """A leaf as a child field holds it (core/flat_types.hpp: make_leaf), as a signed 32-bit number."""
    return ((0x80000000 | (first_slot << 3) | (count - 1)) & 0xFFFFFFFF) - (1 << 32)
