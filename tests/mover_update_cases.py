"""Scenes of MovingSpheres whose values change, for tests/test_set_moving_spheres_host.py and tests/test_gpu_set_moving_spheres.py
(a helper module, not a test file).

A case is a function of `moved`: False builds it at rest, True from scratch with every updatable mover at its new c0, c1 and
radius -- the FRESH scene, the judge of every test -- and a predicate on the mover's position builds the fresh scene of a
partial update.  A case records its updatable movers as (handle, rest values, moved values), values being c0 xyz, c1 xyz,
radius, so update_of() turns a rest scene into the ids and values handed to set_moving_spheres.  time0, time1 and the material
never change.  All seeded, all small; everything here runs on the CPU.

Coordinates are random doubles from a fixed seed and stay away from 0: no two primitives tie exactly, and no box plane is +0 in
one union order and -0 in another (the tests compare bytes).  The default displacement is small -- a few hundredths, a radius
within 7 % -- so that the fresh build chooses the topology the rest build chose and the arrays can be compared byte for byte;
the host test asserts that at least two thirds of the cases keep it, and judges the others by the audits, the top-down
restatement and the frames.  Each shape is named for the place where the code can still go
wrong: see the issue's list in the docstrings below.
"""
import numpy as np

import update_cases
from deform_cases import sheet_mesh
from motion_cases import CASES as MOTION_CASES
from set_transforms_cases import NODE, NODE32, MOTION32, narrow  # noqa: F401  (re-exported)

MOVER = np.dtype([("c0", np.float64, (3,)), ("c1", np.float64, (3,)), ("time0", np.float64), ("time1", np.float64), ("radius", np.float64),
                  ("mat", np.int32), ("pad", np.int32)])
DESC = np.dtype([("flags", np.int32), ("n_ops", np.int32), ("g", np.int32, (3,)), ("medium_mat", np.int32), ("box", np.float32, (6,)),
                 ("neg_inv_density", np.float64), ("ops", np.uint8, (128,)), ("aux", np.float64)])
assert (MOVER.itemsize, DESC.itemsize) == (80, 192)
WD_TIME_BOX = 64
TIME_BOXES, ONE_AXIS, COMMON_RATIO = 1, 2, 4  # bits of RtxRenderStats.trace_variant
# what rtx_flat_array serves and a mover update may or may not touch
FLAT_ARRAYS = ("moving_spheres", "spheres", "nodes", "nodes32", "motion32", "entries", "top_level", "member_local_box", "top_box32", "triangles",
               "lights", "materials")
# rtx_device_scene_array: the arrays an update writes, and those it must keep
DEVICE_WRITTEN = ("moving_spheres", "nodes", "nodes32", "motion32", "nodes4", "world_desc", "top_box32", "lights")
DEVICE_KEPT = ("entries", "spheres", "triangles", "materials", "textures", "plans")


def moved_values(rest, k, scale=1.0):
    """Mover number k of a case at rest -> where the default update puts it: both ends nudged by 0.01 .. 0.04 per axis, each on
    its own, and the radius scaled by 0.93 .. 1.07.  From a seed of its own.  scale: of the nudges and of the radius change (the
    fields of 40 and 300 movers take 1 / 50: the SAH builder bins 32 ways per level, and a centre that crosses a bin edge anywhere
    in a deep tree gives the fresh build another topology)."""
    rng = np.random.default_rng(9100 + k)
    out = np.array(rest, dtype=np.float64)
    out[:6] += scale * rng.uniform(0.01, 0.04, 6) * np.where(rng.uniform(0.0, 1.0, 6) < 0.5, -1.0, 1.0)
    out[6] *= 1.0 + scale * rng.uniform(-0.07, 0.07)
    return out


class Case(update_cases.Case):
    def __init__(self, builder, world, parts, flatten=None, look=((3.0, 4.0, 11.0), (3.0, 1.0, 3.0)), shutter=(0.0, 1.0)):
        super().__init__(builder, world, parts, flatten, look)
        self.shutter = shutter
        self.handles = {}


class _Maker(update_cases.Maker):
    def mover(self, c0, c1, t0, t1, r, mat, to=None, fixed=False):
        """fixed: a mover no update names (it is not a part)."""
        rest = np.array([*c0, *c1, r], dtype=np.float64)
        if fixed:
            return self.b.moving_sphere(tuple(c0), tuple(c1), t0, t1, float(r), mat)
        mv = np.array(to, dtype=np.float64) if to is not None else moved_values(rest, self.k)
        use = mv if self.on(self.k) else rest
        self.k += 1
        h = self.b.moving_sphere(tuple(use[:3]), tuple(use[3:6]), t0, t1, float(use[6]), mat)
        self.parts.append((h, rest, mv))
        return h

    def mats(self):
        b = self.b
        return [b.lambertian((0.8, 0.3, 0.3)), b.metal((0.7, 0.7, 0.8), 0.1), b.dielectric(1.5), b.lambertian((0.2, 0.5, 0.8))]

    def ground(self):
        return self.b.sphere((2.9, -1000.0, 2.9), 1000.0, self.b.lambertian((0.5, 0.5, 0.5)))


def _random_movers(m, n, seed, interval=(0.0, 1.0), axes="xyz", lo=(0.5, 0.45, 0.5), hi=(5.5, 1.7, 5.5), to=None, intervals=None,
                   rest_drift=None):
    """n movers in a box, each travelling 0.25 .. 0.8 along every axis of `axes` (exactly 0 along the others).  to(k, rest) ->
    the moved values of mover k, or None for moved_values'.  intervals: taken by k % len instead of `interval`.  rest_drift: {k: dx}
    added to c1.x of mover k."""
    rng = np.random.default_rng(seed)
    mats = m.mats()
    lo, hi = np.array(lo), np.array(hi)
    out = []
    for k in range(n):
        c0 = lo + (hi - lo) * rng.uniform(0.0, 1.0, 3)
        step = rng.uniform(0.25, 0.8, 3) * np.where(rng.uniform(0.0, 1.0, 3) < 0.5, -1.0, 1.0)
        step[1] = abs(step[1])
        c1 = c0 + np.array([step[a] if "xyz"[a] in axes else 0.0 for a in range(3)])
        c1[0] += (rest_drift or {}).get(k, 0.0)
        r = rng.uniform(0.12, 0.35)
        t0, t1 = intervals[k % len(intervals)] if intervals else interval
        rest = np.array([*c0, *c1, r])
        out.append(m.mover(c0, c1, t0, t1, r, mats[k % len(mats)], to=to(k, rest) if to else None))
    return out


def _along(rest, k, axes, scale=0.02):
    """Mover k nudged as a whole (c0 by moved_values' amounts) and travelling along `axes` only: c1 = c0 exactly on the others."""
    mv = moved_values(rest, k, scale)
    travel = rest[3:6] - rest[:3]
    step = np.zeros(3)
    for a in range(3):
        if "xyz"[a] in axes:
            step[a] = travel[a] if travel[a] != 0.0 else 0.3 + 0.01 * k
    mv[3:6] = mv[:3] + step
    return mv


def _single_bvh(m, movers, interval=(0.0, 1.0), max_leaf=0, statics=(), **kw):
    """ONE BvhNode of the movers, a few static spheres and an r = 1000 ground: the world k_trace_lds takes."""
    b = m.b
    world = b.bvh_from_list(b.hittable_list([m.ground()] + list(statics) + movers), interval[0], interval[1])
    return Case(b, world, m.parts, {"max_leaf": max_leaf}, **kw)


# ---- BVH shapes
def one(rtsr, moved):
    """A BvhNode of ONE mover: no node comes out of it (the flattener makes it a group), only the record changes."""
    m = _Maker(rtsr, 60, moved)
    b = m.b
    lone = b.bvh_from_list(b.hittable_list(_random_movers(m, 1, 600)), 0.0, 1.0)
    return Case(b, b.hittable_list([m.ground(), lone]), m.parts)


def pair(rtsr, moved):
    """Two movers, one node: both climbers meet at the root."""
    m = _Maker(rtsr, 61, moved)
    b = m.b
    return Case(b, b.hittable_list([m.ground(), b.bvh_from_list(b.hittable_list(_random_movers(m, 2, 601)), 0.0, 1.0)]), m.parts)


def mixed5(rtsr, moved, max_leaf=1):
    """Two static spheres and three movers; under max_leaf 4 a leaf holds a static sphere AND a mover."""
    m = _Maker(rtsr, 62, moved)
    b = m.b
    mats = m.mats()
    statics = [b.sphere((1.3, 0.9, 2.1), 0.3, mats[0]), b.sphere((4.2, 1.1, 3.3), 0.25, mats[1])]
    bvh = b.bvh_from_list(b.hittable_list(statics + _random_movers(m, 3, 602)), 0.0, 1.0)
    return Case(b, b.hittable_list([m.ground(), bvh]), m.parts, {"max_leaf": max_leaf})


def tri_mover(rtsr, moved):
    """A small triangle mesh and one mover in one BVH (deform_cases' refusal scene, here with the MOVER updated)."""
    m = _Maker(rtsr, 63, moved)
    b = m.b
    v, f, _ = sheet_mesh(8, origin=(0.5, 0.6, 0.6), extent=3.0, seed=1)
    mesh = b.triangle_mesh(v, f, m.mats()[0])
    bvh = b.bvh_from_list(b.hittable_list([mesh] + _random_movers(m, 1, 603, lo=(1.0, 1.2, 1.0), hi=(3.0, 2.0, 3.0))), 0.0, 1.0)
    return Case(b, b.hittable_list([m.ground(), bvh]), m.parts)


def blocks300(rtsr, moved):
    """300 movers in one BVH: more than 256 leaves, so the climb crosses workgroups."""
    m = _Maker(rtsr, 64, moved)
    return _single_bvh(m, _random_movers(m, 300, 604, lo=(-3.0, 0.4, -3.0), hi=(9.0, 2.5, 9.0), to=lambda k, rest: moved_values(rest, k, 0.02)), max_leaf=1)


def two_bvhs(rtsr, moved):
    """Two timed BVHs and a ground sphere in a world list; ONE is updated, the other's bytes must stay."""
    m = _Maker(rtsr, 65, moved)
    b = m.b
    first = b.bvh_from_list(b.hittable_list(_random_movers(m, 6, 605, hi=(2.8, 1.7, 5.5))), 0.0, 1.0)
    mats = m.mats()
    rng = np.random.default_rng(606)
    others = []
    for k in range(5):
        c0 = np.array([3.2, 0.5, 0.5]) + np.array([2.3, 1.2, 5.0]) * rng.uniform(0.0, 1.0, 3)
        others.append(m.mover(c0, c0 + rng.uniform(0.2, 0.6, 3), 0.0, 1.0, rng.uniform(0.15, 0.3), mats[k % 4], fixed=True))
    second = b.bvh_from_list(b.hittable_list(others), 0.0, 1.0)
    case = Case(b, b.hittable_list([m.ground(), first, second]), m.parts)
    case.handles = {"first": first, "second": second}
    return case


# ---- slope transitions: worlds of one BVH, the slope mask and k_trace_lds's instantiation are judged on these
def _slopes(rtsr, moved, rest_axes, to):
    m = _Maker(rtsr, 66, moved)
    return _single_bvh(m, _random_movers(m, 40, 607, axes=rest_axes, to=to), max_leaf=1)


def y_only(rtsr, moved):
    """40 movers along y, as Book-1 at HEAD builds them; they stay along y."""
    return _slopes(rtsr, moved, "y", lambda k, rest: _along(rest, k, "y"))


def y_to_xy(rtsr, moved):
    """The same, with ONE mover given an x drift: the y-only instantiation would cull it by boxes that no longer hold it."""
    return _slopes(rtsr, moved, "y", lambda k, rest: _along(rest, k, "xy" if k == 7 else "y"))


def xy_to_y(rtsr, moved):
    """The way back: at rest mover 7 drifts along x too."""
    m = _Maker(rtsr, 66, moved)
    return _single_bvh(m, _random_movers(m, 40, 607, axes="y", to=lambda k, rest: _along(rest, k, "y"), rest_drift={7: 0.37}), max_leaf=1)


def still(rtsr, moved):
    """Every c1 = c0: no slope on any axis."""
    return _slopes(rtsr, moved, "y", lambda k, rest: _along(rest, k, ""))


def z_only(rtsr, moved):
    return _slopes(rtsr, moved, "y", lambda k, rest: _along(rest, k, "z"))


# ---- intervals, from motion_cases.py's table: (the movers' own intervals, the BVH's)
INTERVALS = {k: (MOTION_CASES[k][0], MOTION_CASES[k][1]) for k in ("offset", "bvh_narrower", "bvh_wider", "mixed", "reversed", "reversed_bvh", "degenerate")}
INTERVALS["empty_bvh"] = ([(0.0, 1.0)], (0.5, 0.5))
NO_TIME_BOXES = ("reversed_bvh", "empty_bvh")  # a BVH interval that is not ordered: the static path


def interval_case(rtsr, moved, which):
    own, bvh = INTERVALS[which]
    m = _Maker(rtsr, 67, moved)
    shutter = (min(bvh), max(bvh)) if bvh[0] != bvh[1] else (0.0, 1.0)
    return _single_bvh(m, _random_movers(m, 12, 608, intervals=own), interval=bvh, max_leaf=1, shutter=shutter)


# ---- placement
def plain(rtsr, moved):
    """Plain movers in the world list: the slot record's box under WD_TIME_BOX."""
    m = _Maker(rtsr, 68, moved)
    b = m.b
    return Case(b, b.hittable_list([m.ground()] + _random_movers(m, 3, 609) + [b.sphere((0.9, 0.6, 4.8), 0.6, m.mats()[1])]), m.parts)


def plain_overflow(rtsr, moved):
    """A plain mover sent so far that a box plane overflows f32: WD_TIME_BOX must clear, and come back on the way back."""
    m = _Maker(rtsr, 69, moved)
    b = m.b
    far = m.mover((2.1, 1.2, 2.3), (2.4, 1.5, 2.2), 0.0, 1.0, 0.4, m.mats()[0], to=(2.1, 1.2, 2.3, 2.4, 1.0e39, 2.2, 0.4))
    near = m.mover((4.1, 0.9, 3.3), (4.3, 1.3, 3.1), 0.0, 1.0, 0.3, m.mats()[1])
    return Case(b, b.hittable_list([m.ground(), far, near]), m.parts)


def wrapped(rtsr, moved):
    """A mover under Translate(RotateY(..)), a mover as the boundary of a ConstantMedium, and movers in a HittableList group
    under a Translate."""
    m = _Maker(rtsr, 70, moved)
    b = m.b
    mats = m.mats()
    turned = b.translate((1.1, 0.2, 0.7), b.rotate_y(25.0, m.mover((0.6, 0.9, 0.8), (0.9, 1.3, 0.7), 0.0, 1.0, 0.35, mats[0])))
    fog = b.constant_medium((0.8, 0.8, 0.9), 0.7, m.mover((3.6, 1.1, 2.4), (3.9, 1.5, 2.6), 0.0, 1.0, 0.7, mats[2]))
    group = b.translate((0.3, 0.1, 2.9), b.hittable_list(_random_movers(m, 3, 610, lo=(0.4, 0.5, 0.4), hi=(2.4, 1.3, 1.6)) + [b.sphere((1.4, 0.5, 0.9), 0.3, mats[3])]))
    return Case(b, b.hittable_list([m.ground(), turned, fog, group]), m.parts)


def radii(rtsr, moved):
    """A negative radius and a radius of 0 arrive by update, in a small BVH."""
    m = _Maker(rtsr, 71, moved)
    b = m.b

    def to(k, rest):
        mv = moved_values(rest, k)
        mv[6] = -abs(mv[6]) if k == 1 else (0.0 if k == 3 else mv[6])
        return mv

    return Case(b, b.hittable_list([m.ground(), b.bvh_from_list(b.hittable_list(_random_movers(m, 6, 611, to=to)), 0.0, 1.0)]), m.parts, {"max_leaf": 1})


def with_gravity(rtsr, moved):
    """A BVH with a mover and a GravitySphere (refused), beside a BVH of movers alone (still updatable)."""
    m = _Maker(rtsr, 72, moved)
    b = m.b
    mats = m.mats()
    clean = b.bvh_from_list(b.hittable_list(_random_movers(m, 4, 612, hi=(2.8, 1.7, 5.5))), 0.0, 1.0)
    n_clean = len(m.parts)
    bad = m.mover((4.1, 1.0, 2.0), (4.4, 1.4, 2.2), 0.0, 1.0, 0.3, mats[0])
    ball = b.gravity_sphere((4.9, 2.0, 3.5), 0.0, 0.3, mats[1])
    mixed = b.bvh_from_list(b.hittable_list([bad, ball, b.sphere((4.5, 0.8, 4.6), 0.3, mats[3])]), 0.0, 1.0)
    case = Case(b, b.hittable_list([m.ground(), clean, mixed]), m.parts)
    case.handles = {"clean": clean, "mixed": mixed, "bad": bad, "n_clean": n_clean}
    return case


CASES = {
    "one": one, "pair": pair, "mixed5_leaf1": lambda r, mv: mixed5(r, mv, 1), "mixed5_leaf4": lambda r, mv: mixed5(r, mv, 4),
    "tri_mover": tri_mover, "blocks300": blocks300, "two_bvhs": two_bvhs,
    "y_only": y_only, "y_to_xy": y_to_xy, "xy_to_y": xy_to_y, "still": still, "z_only": z_only,
    "plain": plain, "plain_overflow": plain_overflow, "wrapped": wrapped, "radii": radii,
}
for _k in INTERVALS:
    CASES["interval_" + _k] = lambda r, mv, k=_k: interval_case(r, mv, k)
SLOPE_CASES = ("y_only", "y_to_xy", "xy_to_y", "still", "z_only")
# worlds of ONE sphere BVH: k_trace_lds by default, and every forced kernel
LDS_CASES = SLOPE_CASES + ("blocks300",) + tuple("interval_" + k for k in INTERVALS)
FORCED_KERNELS = {k: ("simple", "vote", "world", "wavefront") if k in LDS_CASES else ("simple", "world") for k in CASES}
# movers whose own interval is empty have no finite centre: their boxes are NaN and infinite, which min / max and the casts
# treat alike on either side, but a NaN's sign and payload are not specified across machines -- arrays of this case are compared
# as numbers (NaN == NaN), never as bytes
NAN_CASES = ("interval_degenerate",)


def update_of(case, flat, moved=True, every=1, only=None, reverse=False):
    """(ids, values[n, 7]) that put the updatable movers of `flat` (flattened from `case`, the REST build) at their moved (or,
    moved=False, their rest) values.  every: each every-th mover; only: that one position; reverse: the list back to front."""
    ids, vals = [], []
    for h, rest, mv in case.parts:
        got = flat.moving_sphere_ids(case.builder, h)
        assert len(got) == 1
        ids.append(int(got[0]))
        vals.append(mv if moved else rest)
    ids, vals = np.array(ids, dtype=np.int32), np.array(vals, dtype=np.float64).reshape(-1, 7)
    assert len(set(ids.tolist())) == len(ids)
    if only is not None:
        return ids[only:only + 1].copy(), vals[only:only + 1].copy()
    if reverse:
        return ids[::-1].copy(), vals[::-1].copy()
    return ids[::every].copy(), vals[::every].copy()


def cam_cfg(rtsr, case, width=48, spp=4, depth=8, seed=31):
    """48 x 27 x 4 spp, the shutter the case names."""
    cam = rtsr.Camera.new(case.look[0], case.look[1], (0.0, 1.0, 0.0), 35.0, 16.0 / 9.0, 0.0, 10.0, case.shutter[0], case.shutter[1])
    cfg = rtsr.Config.new(16.0 / 9.0, width, spp, depth, 4, seed=seed)
    return cam, cfg, rtsr.image_height(cfg)


def book1_head(rtsr):
    """Catalogue scene 13 (Book-1 at HEAD: its small spheres are MovingSpheres rising along y, in one BvhNode).  The catalogue
    builds it from the builder's own random stream, so there is no second build with other values: its judges are the audits
    and the host-updated flat scene uploaded afresh.  -> (builder, world, cam, bg)."""
    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(rtsr.SCENE_BOOK1_HEAD)
    return b, world, cam, bg


def book1_update(flat, builder, world, axes="y"):
    """-> (ids of all movers, their values now, their moved values: a hop along `axes`)."""
    ids = flat.moving_sphere_ids(builder, world)
    mov = flat.array("moving_spheres").view(MOVER)
    rest = np.array([[*mov["c0"][i], *mov["c1"][i], mov["radius"][i]] for i in ids])
    mv = np.array([_along(rest[k], k, axes) for k in range(len(ids))])
    return np.asarray(ids, dtype=np.int32), rest, mv


def refusals(n_ids):
    """(name, ids or None, n or None, values or None, word of the message, host entries only), in ladder order."""
    good = np.arange(14, dtype=np.float64).reshape(2, 7) + 1.0
    nan, inf = good.copy(), good.copy()
    nan[1, 2], inf[0, 6] = float("nan"), float("inf")
    return [
        ("null ids", None, 2, good, "ids is NULL", False),
        ("null movers", [0, 1], None, None, "movers is NULL", False),
        ("negative n", [0, 1], -1, good, "n < 0", False),
        ("id negative", [0, -1], None, good, "ids[1] is out of range", False),
        ("id past the end", [n_ids, 1], None, good, "ids[0] is out of range", False),
        ("id named twice", [1, 1], None, good, "twice", False),
        ("NaN centre", [0, 1], None, nan, "movers[1][2] is not finite", True),
        ("infinite radius", [0, 1], None, inf, "movers[0][6] is not finite", True),
    ]


def same_numbers(a, b, dtype):
    """Two byte arrays of `dtype` records hold equal numbers field by field, a NaN equal to a NaN (NAN_CASES)."""
    x, y = a.view(dtype), b.view(dtype)
    if x.shape != y.shape:
        return False
    for f in (x.dtype.names or [None]):
        u, v = (x[f], y[f]) if f else (x, y)
        if u.dtype.kind == "f":
            if not np.array_equal(u, v, equal_nan=True):
                return False
        elif not np.array_equal(u, v):
            return False
    return True
