"""Scenes of moving and resized rectangles for tests/test_set_rects_host.py and tests/test_gpu_set_rects.py (a helper module, not
a test file).

Every case is built twice by the same function: at rest, and from scratch with every updatable rectangle at its new values --
the FRESH scene, the judge of every test.  A part is (handle, rest values, moved values) with values of shape (r, 5): a0 a1 b0
b1 k per rectangle the handle owns -- one for a rectangle, six for a RectPrism (api.prism_rects), in the order of
Flat.rect_ids.  All seeded, all small; everything here runs on the CPU.

Coordinates are random doubles from a fixed seed and stay away from 0: no two primitives tie exactly and no box plane is +0 in
one union order and -0 in another (the tests compare bytes).  Every third rectangle LEAVES its old box (it slides by more than
its own extent), every third SHRINKS, every third moves along its thin axis and grows: a refit that was not made cannot hide.
"""
import numpy as np

import update_cases
from deform_cases import sheet_mesh
from set_transforms_cases import NODE, NODE32, MOTION32, narrow, leaf_boxes, tree_roots  # noqa: F401  (re-exported)
from update_cases import cam_cfg  # noqa: F401  (re-exported)

RECT = np.dtype([("v", np.float64, (5,)), ("axis", np.int32), ("mat", np.int32)])
LIGHT = np.dtype([("kind", np.int32), ("slot", np.int32), ("prim", np.int32), ("mat", np.int32), ("area", np.float64), ("cdf", np.float64), ("pmf", np.float64)])
assert (RECT.itemsize, LIGHT.itemsize) == (48, 40)
FLAT_ARRAYS = ("rects", "nodes", "nodes32", "motion32", "entries", "top_level", "member_local_box", "top_box32", "triangles", "spheres", "lights")
DEVICE_ARRAYS = ("rects", "entries", "nodes", "nodes32", "motion32", "world_desc", "nodes4", "top_box32", "lights")
BVH_SIZES = (2, 3, 64, 65, 257)
FIELD_SIZES = (3, 65)
AXES = ("xy", "xz", "yz")


def moved_values(rest, k):
    """Rectangle number k of a case at rest -> where the update puts it (the module docstring's three classes)."""
    rng = np.random.default_rng(7000 + k)
    a0, a1, b0, b1, kk = [float(x) for x in rest]
    wa, wb = a1 - a0, b1 - b0
    if k % 3 == 0:
        step = wa * rng.uniform(1.2, 1.6)
        return np.array([a0 + step, a1 + step, b0 + 0.1 * wb * rng.uniform(0.2, 1.0), b1, kk])
    if k % 3 == 1:
        return np.array([a0 + 0.2 * wa * rng.uniform(0.5, 1.0), a1 - 0.2 * wa * rng.uniform(0.5, 1.0), b0 + 0.25 * wb * rng.uniform(0.5, 1.0), b1, kk])
    return np.array([a0 - 0.2 * wa * rng.uniform(0.5, 1.0), a1, b0, b1 + 0.3 * wb * rng.uniform(0.5, 1.0), kk + 0.37 * rng.uniform(0.5, 1.0)])


_BUILD_AT = {}  # built_with: position of a rectangle part -> the values it is built at


def built_with(rtsr, name, part, vals):
    """Case `name` at rest but for rectangle part `part`, which is built at `vals`: the fresh scene of an edge-case update."""
    _BUILD_AT[part] = tuple(float(x) for x in vals)
    try:
        return CASES[name](rtsr, False)
    finally:
        _BUILD_AT.clear()


class Case(update_cases.Case):
    def __init__(self, builder, world, parts, flatten=None, look=((3.0, 5.0, 11.0), (3.0, 0.8, 3.0)), aims=()):
        super().__init__(builder, world, parts, flatten, look)
        self.aims = list(aims)


class _Maker(update_cases.Maker):
    def rect(self, axis, vals, mat, to=None):
        rest = np.array(vals, dtype=np.float64).reshape(1, 5)
        mv = np.array(to, dtype=np.float64).reshape(1, 5) if to is not None else moved_values(rest[0], self.k).reshape(1, 5)
        use = (mv if self.on(self.k) else rest)[0]
        use = np.array(_BUILD_AT.get(self.k, use), dtype=np.float64)
        self.k += 1
        h = getattr(self.b, axis + "_rect")(*[float(x) for x in use], mat)
        self.parts.append((h, rest, mv))
        self.aims.append([(axis,), rest, mv, None])
        return h

    def prism(self, p0, p1, mat, to):
        """A RectPrism p0 .. p1 that the update turns into to = (q0, q1): six rectangles, one position in the list of parts."""
        from_, to_ = (tuple(p0), tuple(p1)), (tuple(to[0]), tuple(to[1]))
        use = to_ if self.on(self.k) else from_
        self.k += 1
        h = self.b.rect_prism(use[0], use[1], mat)
        self.parts.append((h, self.rtsr.prism_rects(*from_), self.rtsr.prism_rects(*to_)))
        self.aims.append([("xy", "xy", "xz", "xz", "yz", "yz"), self.parts[-1][1], self.parts[-1][2], None])
        return h

    def __init__(self, rtsr, seed, moved):
        super().__init__(rtsr, seed, moved)
        self.rtsr, self.aims = rtsr, []  # aims: per part, [axes, rest, moved, (offset, degrees) of the chain above it or None]

    def mats(self):
        b = self.b
        return [b.lambertian((0.8, 0.3, 0.3)), b.metal((0.7, 0.7, 0.8), 0.1), b.lambertian((0.2, 0.5, 0.8)), b.lambertian((0.6, 0.6, 0.2))]


def _random_rects(m, n, seed, lo=(0.5, 0.45, 0.5), hi=(5.5, 2.6, 5.5)):
    """n rectangles with the axes mixed, inside lo .. hi."""
    rng = np.random.default_rng(seed)
    mats = m.mats()
    lo, hi = np.array(lo), np.array(hi)
    out = []
    for k in range(n):
        axis = AXES[k % 3]
        ia, ib, ik = {"xy": (0, 1, 2), "xz": (0, 2, 1), "yz": (1, 2, 0)}[axis]
        c = lo + (hi - lo) * rng.uniform(0.0, 1.0, 3)
        wa, wb = rng.uniform(0.25, 0.6, 2)
        out.append(m.rect(axis, (c[ia] - wa, c[ia] + wa, c[ib] - wb, c[ib] + wb, c[ik]), mats[k % len(mats)]))
    return out


LIGHT_REST = (1.13, 2.87, 1.27, 2.93, 3.55)     # the XZ ceiling light of `walls`: x0 x1 z0 z1 y
LIGHT_MOVED = (2.41, 3.29, 2.11, 2.83, 3.15)    # it slides, shrinks and comes down


def walls(rtsr, moved):
    """Six plain rectangle slots, two of each axis, one of them an XZ DiffuseLight, and a Lambertian sphere: no BVH, so
    k_trace_world; the smallest case that reaches k_slot_boxes and the light table."""
    m = _Maker(rtsr, 61, moved)
    b = m.b
    white, red, green = b.lambertian((0.73, 0.73, 0.73)), b.lambertian((0.65, 0.05, 0.05)), b.lambertian((0.12, 0.45, 0.15))
    light = m.rect("xz", LIGHT_REST, b.diffuse_light((7.0, 7.0, 7.0)), to=LIGHT_MOVED)
    parts = [m.rect("yz", (0.03, 3.61, 0.04, 4.12, 4.07), green, to=(0.03, 3.21, 0.54, 4.12, 4.47)),
             m.rect("yz", (0.03, 3.61, 0.04, 4.12, 0.02), red, to=(0.43, 3.61, 0.04, 3.62, 0.32)),
             light,
             m.rect("xz", (0.02, 4.07, 0.04, 4.12, 0.03), white, to=(0.02, 4.47, 0.04, 4.52, 0.13)),
             m.rect("xy", (0.02, 4.07, 0.03, 3.61, 4.12), white, to=(0.32, 4.07, 0.03, 3.21, 3.82)),
             m.rect("xy", (1.32, 2.07, 0.33, 1.21, 2.42), white, to=(1.62, 2.57, 0.33, 1.61, 2.12))]
    world = b.hittable_list(parts + [b.sphere((2.9, 0.61, 1.3), 0.55, white)])
    case = Case(b, world, m.parts, aims=m.aims, look=((2.05, 1.9, -6.5), (2.05, 1.8, 2.0)))
    case.light = light
    return case


def rect_bvh(rtsr, moved, n, max_leaf=0):
    """ONE BvhNode of n rectangles with the axes mixed, interleaved with n // 2 spheres and triangles so that leaves mix kinds,
    over a ground sphere."""
    m = _Maker(rtsr, 62 + n, moved)
    b = m.b
    rects = _random_rects(m, n, 500 + n)
    rng = np.random.default_rng(900 + n)
    grey = b.lambertian((0.5, 0.5, 0.5))
    others = []
    for k in range(n // 2):
        c = np.array([0.5, 0.5, 0.5]) + np.array([5.0, 2.0, 5.0]) * rng.uniform(0.0, 1.0, 3)
        if k % 2 == 0:
            others.append(b.sphere(tuple(c), float(rng.uniform(0.1, 0.3)), grey))
        else:
            others.append(b.triangle(tuple(c), tuple(c + rng.uniform(0.2, 0.6, 3)), tuple(c + rng.uniform(-0.6, -0.2, 3) * np.array([1.0, -1.0, 1.0])), grey))
    mixed = []
    for k, r in enumerate(rects):
        mixed.append(r)
        if k % 2 == 1 and k // 2 < len(others):
            mixed.append(others[k // 2])
    bvh = b.bvh_from_list(b.hittable_list(mixed), 0.0, 1.0)
    world = b.hittable_list([b.sphere((2.9, -1000.0, 2.9), 1000.0, grey), bvh])
    return Case(b, world, m.parts, {"max_leaf": max_leaf}, aims=m.aims)


def _prism_pose(k, rng):
    p0 = np.array([0.11, 0.13, 0.12]) + 0.05 * rng.uniform(0.0, 1.0, 3)
    p1 = p0 + rng.uniform(0.4, 0.9, 3)
    q0 = p0 + np.array([0.31, 0.07, 0.23]) * rng.uniform(0.5, 1.0, 3)
    q1 = q0 + (p1 - p0) * rng.uniform(0.6, 1.4, 3)
    return (p0, p1), (q0, q1)


def prism_field(rtsr, moved, m_count):
    """An instance tree of m - 1 members: Translate(RotateY(RectPrism)) chains and, last, a bare rectangle under a Translate.
    Chain number 1 is wrapped in a ConstantMedium (the Cornell smoke) and stands beside the tree in the world list: the
    flattener admits no medium as a member of an instance tree."""
    m = _Maker(rtsr, 70 + m_count, moved)
    b = m.b
    mats = m.mats()
    rng = np.random.default_rng(800 + m_count)
    side = int(np.ceil(np.sqrt(m_count)))
    members = []
    for k in range(m_count):
        at = (0.4 + 1.3 * (k % side) + 0.1 * rng.uniform(), 0.2 + 0.1 * rng.uniform(), 0.5 + 1.3 * (k // side) + 0.1 * rng.uniform())
        if k == m_count - 1:
            members.append(b.translate(at, m.rect("xy", (0.12, 0.93, 0.11, 1.07, 0.41), mats[0])))
            m.aims[-1][3] = (at, 0.0)
            continue
        rest, to = _prism_pose(k, rng)
        angle = float(rng.uniform(-40.0, 40.0))
        box = b.translate(at, b.rotate_y(angle, m.prism(rest[0], rest[1], mats[k % 4], to)))
        m.aims[-1][3] = (at, angle)
        if k == 1:
            smoke = b.constant_medium((0.8, 0.8, 0.9), 0.9, box)
        else:
            members.append(box)
    ground = b.sphere((2.3, -500.0, 2.4), 500.0, b.lambertian((0.5, 0.5, 0.5)))
    world = b.hittable_list([ground, b.instance_bvh(b.hittable_list(members)), smoke])
    span = 1.3 * side
    return Case(b, world, m.parts, aims=m.aims, look=((0.5 * span, 0.9 * span + 3.0, 2.2 * span + 4.0), (0.5 * span, 0.5, 0.5 * span)))


def vote_room(rtsr, moved, n_slots=7, with_sphere=False):
    """ONE BvhNode of 64 triangles beside n_slots plain rectangle slots: with seven, plan_vote copies the records into
    k_trace_vote's launch argument; with nine the kernel walks the list; with a sphere among the slots the copy is not made."""
    m = _Maker(rtsr, 80 + n_slots, moved)
    b = m.b
    mats = m.mats()
    v, f, _ = sheet_mesh(64, origin=(0.9, 0.7, 0.9), extent=2.4, seed=3)
    assert len(f) == 64
    mesh = b.triangle_mesh(v, f, mats[0])
    slots = _random_rects(m, n_slots, 990 + n_slots, lo=(0.4, 0.5, 0.4), hi=(4.4, 2.8, 4.4))
    if with_sphere:
        slots.insert(3, b.sphere((3.7, 0.8, 1.1), 0.45, mats[1]))
    world = b.hittable_list(slots[:2] + [b.bvh_from_list(mesh, 0.0, 1.0)] + slots[2:])
    return Case(b, world, m.parts, aims=m.aims, look=((2.3, 5.0, 9.5), (2.3, 1.2, 2.4)))


def shared_prism(rtsr, moved):
    """ONE RectPrism handle under two Translates: twelve rectangles, one part."""
    m = _Maker(rtsr, 90, moved)
    b = m.b
    box = m.prism((0.12, 0.11, 0.13), (0.93, 1.21, 0.87), b.lambertian((0.7, 0.4, 0.3)), ((0.32, 0.11, 0.23), (1.43, 0.81, 1.37)))
    world = b.hittable_list([b.sphere((2.3, -500.0, 2.4), 500.0, b.lambertian((0.5, 0.5, 0.5))), b.translate((0.7, 0.2, 1.1), box),
                             b.translate((2.9, 0.3, 2.2), box)])
    m.parts[0] = (box, np.tile(m.parts[0][1], (2, 1)), np.tile(m.parts[0][2], (2, 1)))
    m.aims = [[m.aims[0][0], m.aims[0][1], m.aims[0][2], ((0.7, 0.2, 1.1), 0.0)], [m.aims[0][0], m.aims[0][1], m.aims[0][2], ((2.9, 0.3, 2.2), 0.0)]]
    return Case(b, world, m.parts, aims=m.aims, look=((2.3, 4.0, 9.0), (2.3, 0.7, 2.0)))


def beside_movers(rtsr, moved):
    """A rectangle in a BVH that holds a MovingSphere (an update of it is refused) beside a plain rectangle slot."""
    m = _Maker(rtsr, 91, moved)
    b = m.b
    grey = b.lambertian((0.5, 0.5, 0.5))
    plain = m.rect("xz", (0.6, 1.7, 0.5, 1.9, 1.3), grey)
    timed_rect = b.xy_rect(0.8, 1.9, 2.1, 2.9, 1.4, grey)
    timed = b.bvh_from_list(b.hittable_list([timed_rect] + [b.moving_sphere((0.8 + k, 2.5, 1.0), (0.8 + k, 2.5 + 0.2 * k, 1.0), 0.0, 1.0, 0.3, grey) for k in range(1, 4)]), 0.0, 1.0)
    world = b.hittable_list([b.sphere((2.9, -1000.0, 2.9), 1000.0, grey), plain, timed])
    case = Case(b, world, m.parts, aims=m.aims)
    case.handles = {"timed_rect": timed_rect}
    return case


CASES = {"walls": walls, "shared_prism": shared_prism,
         "vote_room7": lambda r, mv: vote_room(r, mv, 7), "vote_room9": lambda r, mv: vote_room(r, mv, 9),
         "vote_room_sphere": lambda r, mv: vote_room(r, mv, 7, with_sphere=True)}
for _n in BVH_SIZES:
    CASES["rect_bvh%d" % _n] = lambda r, mv, n=_n: rect_bvh(r, mv, n)
    CASES["rect_bvh%d_leaf1" % _n] = lambda r, mv, n=_n: rect_bvh(r, mv, n, max_leaf=1)
for _n in FIELD_SIZES:
    CASES["prism_field%d" % _n] = lambda r, mv, n=_n: prism_field(r, mv, n)
VOTE_CASES = ("vote_room7", "vote_room9", "vote_room_sphere")
# the forced kernels choose_trace_kernel accepts each world under
FORCED_KERNELS = {k: {"simple", "world"} for k in CASES}
FORCED_KERNELS.update({k: {"simple", "vote", "world", "wavefront"} for k in CASES if k.startswith(("rect_bvh", "vote_room"))})


def update_of(case, flat, moved=True, select=None):
    """(ids, values[n, 5]) that put the updatable rectangles of `flat` (flattened from `case`, the REST build) at their moved
    (moved=False: their rest) values.  select: a predicate on a part's position; the others are left out."""
    ids, vals = [], []
    for k, (h, rest, mv) in enumerate(case.parts):
        if select is not None and not select(k):
            continue
        got = flat.rect_ids(case.builder, h)
        assert len(got) == len(rest), (len(got), len(rest))
        ids.extend(int(i) for i in got)
        vals.extend(mv if moved else rest)
    ids, vals = np.array(ids, dtype=np.int32), np.array(vals, dtype=np.float64).reshape(-1, 5)
    assert len(set(ids.tolist())) == len(ids)
    return ids, vals


def probe_rays(case, n, seed):
    """n rays aimed AT the updated rectangles: each at a random point of a random updatable rectangle, half of them at its rest
    and half at its moved pose (through the chain above it, RotateY then Translate, where it has one), from origins above and
    beside the scene.  A ray at the rest pose meets the rectangle only before the update, one at the moved pose only after: an
    update that wrote nothing cannot answer them as the fresh scene does."""
    rng = np.random.default_rng(seed)
    centre = np.array(case.look[1])
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for r in range(n):
        axes, rest, mv, chain = case.aims[int(rng.integers(0, len(case.aims)))]
        q = int(rng.integers(0, len(axes)))
        a0, a1, b0, b1, k = (rest if r % 2 == 0 else mv)[q if len(rest) > q else 0]
        u, v = a0 + (a1 - a0) * rng.uniform(0.05, 0.95), b0 + (b1 - b0) * rng.uniform(0.05, 0.95)
        p = np.array({"xy": (u, v, k), "xz": (u, k, v), "yz": (k, u, v)}[axes[q]])
        if chain is not None:
            c, s_ = np.cos(np.radians(chain[1])), np.sin(np.radians(chain[1]))
            p = np.array([c * p[0] + s_ * p[2], p[1], -s_ * p[0] + c * p[2]]) + np.array(chain[0])
        org = centre + np.array([rng.uniform(-4.0, 4.0), rng.uniform(2.5, 6.0), rng.uniform(-4.0, 4.0)])
        side = int(rng.integers(0, 3))
        if side == 1:
            org = centre + np.array([-6.0, rng.uniform(0.2, 3.0), rng.uniform(-3.0, 3.0)])
        elif side == 2:
            org = centre + np.array([rng.uniform(-3.0, 3.0), rng.uniform(0.2, 3.0), 6.0])
        o[r], d[r] = org, p - org
    return o, d


def refusals(n_ids):
    """(name, ids or None, n or None, values or None, word of the message, host entries only)."""
    good = np.arange(10, dtype=np.float64).reshape(2, 5) + 1.0
    nan, inf = good.copy(), good.copy()
    nan[1, 2], inf[0, 4] = float("nan"), float("inf")
    return [
        ("null ids", None, 2, good, "ids is NULL", False),
        ("null rects", [0, 1], None, None, "rects is NULL", False),
        ("negative n", [0, 1], -1, good, "n < 0", False),
        ("id negative", [0, -1], None, good, "ids[1] is out of range", False),
        ("id past the end", [n_ids, 1], None, good, "ids[0] is out of range", False),
        ("id named twice", [1, 1], None, good, "twice", False),
        ("NaN extent", [0, 1], None, nan, "rects[1][2] is not finite", True),
        ("infinite k", [0, 1], None, inf, "rects[0][4] is not finite", True),
    ]


def edge_values(rest):
    """The issue's edge cases for one rectangle at `rest`: name -> values."""
    a0, a1, b0, b1, k = [float(x) for x in rest]
    return {"inverted": (a1, a0, b0, b1, k), "zero extent": (a0, a0, b0, b1, k), "negative zero k": (a0, a1, b0, b1, -0.0),
            "k = 1e13": (a0, a1, b0, b1, 1e13), "extents of 1e300": (-1e300, 1e300, -1e300, 1e300, k), "itself": (a0, a1, b0, b1, k)}
