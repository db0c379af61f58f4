"""Scenes of moving static spheres for tests/test_set_spheres_host.py and tests/test_gpu_set_spheres.py (a helper module, not a
test file).

Every case is built twice by the same function: at rest, and from scratch with every movable sphere at its new centre and
radius -- the FRESH scene, the judge of every test.  A case records its movable spheres: the handle rtx_flat_sphere_ids lists
them under and their values (cx cy cz radius) at rest and moved, so update_of() turns a rest scene into the ids and values
handed to set_spheres.  All seeded, all small; everything here runs on the CPU.

Coordinates are random doubles from a fixed seed and stay away from 0: no two primitives tie exactly, and no box plane is +0
in one union order and -0 in another (the tests compare bytes).

The rule of every full update (assert_update_can_show): at least one sphere LEAVES the old box of its leaf -- its centre moves
by more than 2 |r| along one axis -- and at least another SHRINKS.  A refit that was not made cannot hide behind either: the
first needs the boxes above it to grow, the second to shrink.
"""
import math

import numpy as np

import update_cases
from deform_cases import sheet_mesh
from set_transforms_cases import NODE, NODE32, MOTION32, narrow, leaf_boxes, tree_roots  # noqa: F401  (re-exported)
from update_cases import INSTANCED_POSE, cam_cfg  # noqa: F401  (re-exported)

SPHERE = np.dtype([("c", np.float64, (3,)), ("radius", np.float64), ("mat", np.int32), ("pad", np.int32)])
LIGHT = np.dtype([("kind", np.int32), ("slot", np.int32), ("prim", np.int32), ("mat", np.int32), ("area", np.float64), ("cdf", np.float64), ("pmf", np.float64)])
DESC = np.dtype([("flags", np.int32), ("n_ops", np.int32), ("g", np.int32, (3,)), ("medium_mat", np.int32), ("box", np.float32, (6,)), ("rest", np.uint8, (144,))])
assert (SPHERE.itemsize, LIGHT.itemsize, DESC.itemsize) == (40, 40, 192)
WD_BOXED_PRIM, WD_PAIR = 8, 32
FLAT_ARRAYS = ("spheres", "nodes", "nodes32", "motion32", "entries", "top_level", "member_local_box", "top_box32", "triangles", "lights")
# rtx_device_scene_array 1, 2, 3, 4, 7, 10, 11, 13, 14 (and 0, which no sphere update writes)
DEVICE_ARRAYS = ("nodes", "nodes32", "motion32", "world_desc", "nodes4", "triangles", "top_box32", "spheres", "lights", "entries")
FIELD_SIZES = (2, 3, 5, 64, 65, 257)


def moved_values(rest, k):
    """Sphere number k of a case at rest -> where the update puts it.  k % 3 == 0: it LEAVES its old box (2.4 to 3 |r| along x or
    z); 1: it SHRINKS (to 45 .. 70 %); 2: it grows by 20 .. 50 %.  Everything jitters, from a seed of its own."""
    rng = np.random.default_rng(9000 + k)
    c, r = np.array(rest[:3], dtype=np.float64), float(rest[3])
    jitter = 0.3 * abs(r) * rng.uniform(0.2, 1.0, 3)
    if k % 3 == 0:
        step = np.zeros(3)
        step[0 if (k // 3) % 2 == 0 else 2] = abs(r) * rng.uniform(2.4, 3.0)
        return np.array([*(c + step + jitter * np.array([0.0, 1.0, 0.0])), r * rng.uniform(0.9, 1.1)])
    if k % 3 == 1:
        return np.array([*(c + jitter), r * rng.uniform(0.45, 0.7)])
    return np.array([*(c + jitter), r * rng.uniform(1.2, 1.5)])


def assert_update_can_show(rest, moved):
    """The rule of the module docstring, on (n, 4) arrays of values."""
    rest, moved = np.asarray(rest).reshape(-1, 4), np.asarray(moved).reshape(-1, 4)
    leaves = (np.abs(moved[:, :3] - rest[:, :3]).max(axis=1) > 2.0 * np.abs(rest[:, 3])) | (np.abs(moved[:, 3]) >= 3.0 * np.abs(rest[:, 3]))
    shrinks = np.abs(moved[:, 3]) < np.abs(rest[:, 3])
    assert leaves.any(), "no sphere leaves the old box of its leaf"
    assert (shrinks & ~leaves).any(), "no other sphere shrinks"


class Case(update_cases.Case):
    def __init__(self, builder, world, parts, flatten=None, look=((3.0, 5.0, 11.0), (3.0, 0.8, 3.0))):
        super().__init__(builder, world, parts, flatten, look)


class _Maker(update_cases.Maker):
    """Movable spheres: (handle, rest values, moved values) per sphere.  to: where this sphere goes instead of moved_values'
    place (the lamp's updates, the fog's common move)."""

    def sphere(self, c, r, mat, to=None):
        rest = np.array([c[0], c[1], c[2], r], dtype=np.float64)
        mv = np.array(to, dtype=np.float64) if to is not None else moved_values(rest, self.k)
        use = mv if self.on(self.k) else rest
        self.k += 1
        h = self.b.sphere(tuple(use[:3]), float(use[3]), mat)
        self.parts.append((h, rest, mv))
        return h

    def mats(self):
        b = self.b
        return [b.lambertian((0.8, 0.3, 0.3)), b.metal((0.7, 0.7, 0.8), 0.1), b.dielectric(1.5), b.lambertian((0.2, 0.5, 0.8))]


def _random_spheres(m, n, seed, lo=(0.5, 0.45, 0.5), hi=(5.5, 1.7, 5.5)):
    rng = np.random.default_rng(seed)
    mats = m.mats()
    lo, hi = np.array(lo), np.array(hi)
    return [m.sphere(lo + (hi - lo) * rng.uniform(0.0, 1.0, 3), rng.uniform(0.12, 0.4), mats[k % len(mats)]) for k in range(n)]


def field(rtsr, moved, n, max_leaf=0, checker=False):
    """ONE BvhNode of n static spheres and an r = 1000 ground: the world k_trace_lds takes (checker: its second static
    instantiation, which keeps every sphere as a moving-sphere record)."""
    m = _Maker(rtsr, 20 + n, moved)
    b = m.b
    ground_mat = b.lambertian(b.checker_from_colors((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))) if checker else b.lambertian((0.5, 0.5, 0.5))
    ground = b.sphere((2.9, -1000.0, 2.9), 1000.0, ground_mat)
    world = b.bvh_from_list(b.hittable_list([ground] + _random_spheres(m, n, 300 + n)), 0.0, 1.0)
    return Case(b, world, m.parts, {"max_leaf": max_leaf})


def hollow(rtsr, moved):
    """A sphere of negative radius inside a positive one (the hollow glass ball), both updated, in the BVH of a small field."""
    m = _Maker(rtsr, 41, moved)
    b = m.b
    glass = b.dielectric(1.5)
    ground = b.sphere((2.9, -1000.0, 2.9), 1000.0, b.lambertian((0.5, 0.5, 0.5)))
    to = (4.63, 1.52, 2.71)
    outer = m.sphere((2.31, 1.13, 3.07), 0.9, glass, to=(*to, 0.6))
    inner = m.sphere((2.31, 1.13, 3.07), -0.8, glass, to=(*to, -0.5))
    world = b.bvh_from_list(b.hittable_list([ground, outer, inner] + _random_spheres(m, 6, 77)), 0.0, 1.0)
    return Case(b, world, m.parts)


def mixed(rtsr, moved):
    """One BVH of triangles, spheres and rectangles beside a plain ground: k_trace_vote, the wide tree, the wavefront integrator."""
    m = _Maker(rtsr, 42, moved)
    b = m.b
    red, grey = b.lambertian((0.8, 0.3, 0.3)), b.metal((0.7, 0.7, 0.8), 0.1)
    v, f, _ = sheet_mesh(24, origin=(0.5, 0.6, 0.6), extent=3.0, seed=1)
    mesh = b.triangle_mesh(v, f, red)
    others = [b.xz_rect(0.4, 1.6, 2.6, 3.8, 1.9, grey), b.xy_rect(2.6, 3.9, 0.5, 1.8, 0.45, red), b.yz_rect(0.7, 1.9, 1.1, 2.3, 4.1, grey)]
    bvh = b.bvh_from_list(b.hittable_list([mesh] + _random_spheres(m, 9, 78, lo=(0.6, 0.9, 0.6), hi=(4.5, 2.6, 4.5)) + others), 0.0, 1.0)
    world = b.hittable_list([b.sphere((2.3, -500.0, 2.4), 500.0, b.lambertian((0.5, 0.5, 0.5))), bvh])
    case = Case(b, world, m.parts, look=((2.3, 5.0, 8.5), (2.3, 1.0, 2.4)))
    case.mesh = mesh
    return case


def plain(rtsr, moved):
    """Spheres as plain slots of the world list (k_trace_world; top_box32 and the slot records)."""
    m = _Maker(rtsr, 43, moved)
    b = m.b
    world = b.hittable_list([b.sphere((2.9, -1000.0, 2.9), 1000.0, b.lambertian((0.5, 0.5, 0.5)))] + _random_spheres(m, 5, 79) +
                            [b.xz_rect(1.1, 2.3, 1.2, 2.6, 2.4, b.metal((0.8, 0.8, 0.8), 0.0))])
    return Case(b, world, m.parts)


def fog(rtsr, moved):
    """A ConstantMedium around a sphere, moved and resized: once inside a glass ball of the very same values (Book-2's idiom: the
    slot record of the ball says "same sphere as the medium behind me"), once alone."""
    m = _Maker(rtsr, 44, moved)
    b = m.b
    to = (4.13, 1.74, 2.21, 0.85)
    ball = m.sphere((1.71, 1.32, 2.93), 1.1, b.dielectric(1.5), to=to)
    inside = m.sphere((1.71, 1.32, 2.93), 1.1, b.dielectric(1.5), to=to)
    alone = m.sphere((4.63, 1.17, 4.39), 0.9, b.dielectric(1.5), to=(4.71, 1.25, 4.31, 0.55))
    world = b.hittable_list([b.sphere((2.9, -1000.0, 2.9), 1000.0, b.lambertian((0.4, 0.6, 0.4))), ball, b.constant_medium((0.2, 0.4, 0.9), 0.8, inside),
                             b.constant_medium((0.9, 0.9, 1.0), 0.6, alone), b.sphere((0.9, 0.6, 4.8), 0.6, b.metal((0.8, 0.8, 0.8), 0.0))])
    return Case(b, world, m.parts)


CHECKER_CELL = math.pi / 10.0  # Checker::value: the sign of sin(10 x) sin(10 y) sin(10 z) (texture.rs:54-64)


def checker_is_odd(p):
    return math.sin(10.0 * p[0]) * math.sin(10.0 * p[1]) * math.sin(10.0 * p[2]) < 0.0


LAMP_REST = (2.05, 2.6, 2.05, 0.4)           # the sphere light: its centre in a bright (even) cell
LAMP_UPDATES = {
    "other cell": (2.05 + CHECKER_CELL, 2.6, 2.05, 0.4),   # one cell along x: the dark colour; the area stays
    "radius": (2.05, 2.6, 2.05, 0.17),                      # the area changes, the colour does not
    "far": (3.97, 2.71, 1.41, 0.55),                        # both, and the sphere leaves its old box
}
assert not checker_is_odd(LAMP_REST) and checker_is_odd(LAMP_UPDATES["other cell"]) and not checker_is_odd(LAMP_UPDATES["far"])


def lamp(rtsr, moved, to="other cell", dark_rect=False):
    """A top-level sphere light whose emission is a checker with one colour black, next to a rectangle light, over a few plain
    spheres.  dark_rect: the rectangle light wears the same checker with its centre in a black cell, so the sphere light holds
    the only non-zero pick weight -- and once it moves into a black cell too, every weight is 0: the uniform fallback."""
    m = _Maker(rtsr, 45, moved)
    b = m.b
    emit = b.checker_from_colors((6.0, 5.0, 4.0), (0.0, 0.0, 0.0))
    light = m.sphere(LAMP_REST[:3], LAMP_REST[3], b.diffuse_light(emit), to=LAMP_UPDATES[to])
    rect_centre = (3.45 + (0.0 if checker_is_odd((3.45, 3.1, 2.55)) else CHECKER_CELL), 3.1, 2.55)
    assert checker_is_odd(rect_centre)
    rect = b.xz_rect(rect_centre[0] - 0.6, rect_centre[0] + 0.6, 1.95, 3.15, 3.1, b.diffuse_light(emit if dark_rect else (4.0, 4.0, 4.0)))
    world = b.hittable_list([b.sphere((2.9, -1000.0, 2.9), 1000.0, b.lambertian((0.5, 0.5, 0.5))), light, rect] + _random_spheres(m, 3, 80, hi=(5.5, 1.2, 5.5)))
    case = Case(b, world, m.parts, look=((3.0, 4.0, 10.0), (3.0, 1.4, 2.5)))
    case.light = light
    return case


def instanced(rtsr, moved, pose=INSTANCED_POSE, tris_moved=False):
    """An instance tree whose members are a sphere, a group of spheres and a BVH of spheres (and, for the sequence, a BVH of
    triangles), each under a Translate and two under a RotateY as well.  tris_moved: the mesh member displaced (the sequence)."""
    from deform_cases import displace
    m = _Maker(rtsr, 46, moved)
    b = m.b
    mats = m.mats()
    one = m.sphere((0.41, 0.73, 0.52), 0.35, mats[0])
    group = b.hittable_list([m.sphere((0.31 + 0.8 * k, 0.62 + 0.1 * k, 0.43), 0.25 + 0.03 * k, mats[k % 4]) for k in range(3)])
    bvh = b.bvh_from_list(b.hittable_list(_random_spheres(m, 7, 81, lo=(0.2, 0.4, 0.2), hi=(2.2, 1.4, 2.2))), 0.0, 1.0)
    v, f, cell = sheet_mesh(12, origin=(0.2, 0.5, 0.3), extent=1.6, seed=7)
    tri_rest = np.asarray(v)[f]
    tri = displace(tri_rest, cell) if tris_moved else tri_rest
    mesh = b.triangle_mesh(tri.reshape(-1, 3), np.arange(3 * len(tri), dtype=np.int64).reshape(-1, 3), mats[3])
    members = [b.translate(pose[0][0], b.rotate_y(pose[0][1], bvh)), b.translate(pose[1][0], b.rotate_y(pose[1][1], group)),
               b.translate(pose[2][0], one), b.translate((4.4, 0.3, 0.5), b.bvh_from_list(mesh, 0.0, 1.0))]
    ground = b.sphere((2.3, -500.0, 2.4), 500.0, b.lambertian((0.5, 0.5, 0.5)))
    world = b.hittable_list([ground, b.instance_bvh(b.hittable_list(members))])
    case = Case(b, world, m.parts, look=((2.8, 5.5, 10.5), (2.8, 1.0, 2.4)))
    case.mesh, case.mesh_rest, case.mesh_moved = mesh, tri_rest, displace(tri_rest, cell)
    case.handles = {"one": one, "group": group, "bvh": bvh, "members": members}
    return case


def shared(rtsr, moved):
    """ONE sphere handle listed in the world list AND in a BVH: one id, both places move."""
    m = _Maker(rtsr, 47, moved)
    b = m.b
    both = m.sphere((1.53, 1.21, 2.37), 0.5, b.metal((0.9, 0.6, 0.3), 0.05))
    bvh = b.bvh_from_list(b.hittable_list([both] + _random_spheres(m, 6, 82)), 0.0, 1.0)
    world = b.hittable_list([b.sphere((2.9, -1000.0, 2.9), 1000.0, b.lambertian((0.5, 0.5, 0.5))), both, bvh])
    case = Case(b, world, m.parts)
    case.handles = {"both": both, "bvh": bvh}
    return case


def beside_movers(rtsr, moved):
    """A static field next to a BVH that holds a MovingSphere (and one static sphere, whose id an update must refuse)."""
    m = _Maker(rtsr, 48, moved)
    b = m.b
    grey = b.lambertian((0.5, 0.5, 0.5))
    field_bvh = b.bvh_from_list(b.hittable_list(_random_spheres(m, 8, 83)), 0.0, 1.0)
    timed_static = b.sphere((0.8, 2.6, 5.0), 0.3, grey)
    timed = b.bvh_from_list(b.hittable_list([timed_static] + [b.moving_sphere((0.8 + k, 2.5, 1.0), (0.8 + k, 2.5 + 0.2 * k, 1.0), 0.0, 1.0, 0.3, grey) for k in range(1, 4)]), 0.0, 1.0)
    world = b.hittable_list([b.sphere((2.9, -1000.0, 2.9), 1000.0, grey), field_bvh, timed])
    case = Case(b, world, m.parts)
    case.handles = {"timed_static": timed_static, "timed": timed, "field": field_bvh}
    return case


CASES = {
    "hollow": hollow, "mixed": mixed, "plain": plain, "fog": fog, "lamp": lamp, "instanced": instanced, "shared": shared,
    "beside_movers": beside_movers,
    "lamp_radius": lambda r, mv: lamp(r, mv, to="radius"), "lamp_far": lambda r, mv: lamp(r, mv, to="far"),
    "lamp_dark": lambda r, mv: lamp(r, mv, to="other cell", dark_rect=True),
    "field65_checker": lambda r, mv: field(r, mv, 65, checker=True),
}
for _n in FIELD_SIZES:
    CASES["field%d" % _n] = lambda r, mv, n=_n: field(r, mv, n)
    CASES["field%d_leaf1" % _n] = lambda r, mv, n=_n: field(r, mv, n, max_leaf=1)
LDS_CASES = tuple(k for k in CASES if k.startswith("field")) + ("hollow",)  # worlds of one sphere BVH: k_trace_lds by default
# the forced kernels choose_trace_kernel accepts each world under: `simple` and `world` any; `vote` and the wavefront
# integrator a world of ONE BVH beside plain primitives
FORCED_KERNELS = {k: {"simple", "vote", "world", "wavefront"} for k in LDS_CASES + ("mixed", "shared")}
FORCED_KERNELS.update({k: {"simple", "world"} for k in CASES if k not in FORCED_KERNELS})


def update_of(case, flat, moved=True, every=1, only=None):
    """(ids, values[n, 4]) that put the movable spheres of `flat` (flattened from `case`, the REST build) at their moved (or,
    moved=False, their rest) values.  every: each every-th sphere; only: that one position of the full list."""
    ids, vals = [], []
    for h, rest, mv in case.parts:
        got = flat.sphere_ids(case.builder, h)
        assert len(got) == 1
        ids.append(int(got[0]))
        vals.append(mv if moved else rest)
    ids, vals = np.array(ids, dtype=np.int32), np.array(vals, dtype=np.float64).reshape(-1, 4)
    assert len(set(ids.tolist())) == len(ids)
    if only is not None:
        return ids[only:only + 1].copy(), vals[only:only + 1].copy()
    return ids[::every].copy(), vals[::every].copy()


def rest_and_moved(case):
    return np.array([r for _, r, _ in case.parts]), np.array([m for _, _, m in case.parts])


def book1(rtsr):
    """Catalogue scene 100 (Book-1 final: 484 spheres and the ground in one BvhNode) and an update of its small spheres by
    moved_values.  The catalogue builds it from the builder's own random stream, so there is no second build with other
    values: its judges are the exact box audit and the host-updated flat scene uploaded afresh.  -> (builder, world, cam, bg)."""
    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(rtsr.SCENE_BOOK1_CANONICAL)
    return b, world, cam, bg


def book1_update(flat, builder, world):
    """-> (ids of the small spheres, their values now, their moved values)."""
    ids = flat.sphere_ids(builder, world)
    sph = flat.array("spheres").view(SPHERE)
    small = [int(i) for i in ids if abs(sph["radius"][i]) < 0.5]
    rest = np.array([[*sph["c"][i], sph["radius"][i]] for i in small])
    mv = np.array([moved_values(rest[k], k) for k in range(len(small))])
    return np.array(small, dtype=np.int32), rest, mv


def seeded_rays(n, seed):
    return update_cases.seeded_rays(n, seed, (-0.5, 0.3, -0.5), (6.5, 3.5, 6.5), (0.3, 2.2))


def refusals(n_ids):
    """(name, ids or None, n or None, values or None, word of the message, host entries only)."""
    good = np.arange(8, dtype=np.float64).reshape(2, 4) + 1.0
    nan, inf = good.copy(), good.copy()
    nan[1, 2], inf[0, 3] = float("nan"), float("inf")
    return [
        ("null ids", None, 2, good, "ids is NULL", False),
        ("null spheres", [0, 1], None, None, "spheres is NULL", False),
        ("negative n", [0, 1], -1, good, "n < 0", False),
        ("id negative", [0, -1], None, good, "ids[1] is out of range", False),
        ("id past the end", [n_ids, 1], None, good, "ids[0] is out of range", False),
        ("id named twice", [1, 1], None, good, "twice", False),
        ("NaN centre", [0, 1], None, nan, "spheres[1][2] is not finite", True),
        ("infinite radius", [0, 1], None, inf, "spheres[0][3] is not finite", True),
    ]
