"""The host checker, scenes and point sets of tests/test_nearest_cases.py and tests/test_gpu_nearest.py (a helper module, not a
test file): everything here runs on the CPU.

Three judges, each for what the one below it cannot see:
  1. closed forms in numpy longdouble, sharing nothing with csrc/: they judge prim_nearest and the transforms;
  2. host_nearest_exhaustive (tests/nearest_host_check.cpp: plain loops over every slot and ref, no box, no ordering): the
     culled walk host_nearest -- world_nearest<F_ALL> -- must equal it bit for bit on every point;
  3. the walk's counters: culling must save primitive tests.
The checker is built with oracle/Makefile's CXXFLAGS, once as it is (f64) and once with -DNEAREST_HOST_F32 (the float judge,
linked to liboracle.so for oracle_f32_images)."""
import ctypes as C
import os
import subprocess

import numpy as np

import cast_rays_cases as cc
from instance_scenes import member_zoo
import lbvh_cases
import occlusion_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "nearest_host_check.cpp")
ORACLE_BUILD = os.path.join(ROOT, "oracle", "_build")
INF = float("inf")
LD = np.longdouble
PRIM_SPHERE, PRIM_MOVING_SPHERE, PRIM_RECT, PRIM_TRIANGLE = 0, 1, 2, 3

_D = C.POINTER(C.c_double)
_ARGS = [C.c_void_p, C.c_int64, _D, _D, _D, C.c_double, C.c_int, _D, _D, C.POINTER(C.c_int32), C.POINTER(C.c_ulonglong)]
_checkers = {}


def checkers(tmp_path_factory):
    """{(f32, exhaustive): entry}, built once per session (needs liboracle.so: the orc fixture)."""
    if not _checkers:
        d = tmp_path_factory.mktemp("nearest_host")
        out64, out32 = str(d / "nearest_host_check.so"), str(d / "nearest_host_check_f32.so")
        subprocess.run(["g++"] + oc.CXXFLAGS + ["-shared", SRC, "-o", out64], check=True)
        subprocess.run(["g++"] + oc.CXXFLAGS + ["-DNEAREST_HOST_F32", "-shared", SRC, os.path.join(ORACLE_BUILD, "liboracle.so"),
                        "-Wl,-rpath," + ORACLE_BUILD, "-o", out32], check=True)
        for f32, path, tail in ((False, out64, ""), (True, out32, "_f32")):
            lib = C.CDLL(path)
            for exhaustive, name in ((False, "host_nearest"), (True, "host_nearest_exhaustive")):
                fn = getattr(lib, name + tail)
                fn.restype, fn.argtypes = C.c_int, _ARGS
                _checkers[(f32, exhaustive)] = fn
        _checkers["refs"] = slot_refs_entry(C.CDLL(out64))
    return _checkers


def slot_refs_entry(lib):
    fn = lib.host_slot_refs
    fn.restype, fn.argtypes = C.c_int64, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int64]
    return fn


def slot_refs(chk, flat, slot):
    """The ref list of the BVH or GROUP in a top-level slot, in list order, as (n, 2) {PrimType, index}: row k is the primitive at
    ref position k, the `order` of the key (read from the flat arrays by the checker, not through core/nearest.hpp)."""
    n = chk["refs"](flat.arrays_ptr(), slot, None, 0)
    assert n >= 0, slot
    out = np.zeros((n, 2), dtype=np.int32)
    assert chk["refs"](flat.arrays_ptr(), slot, out.ctypes.data_as(C.POINTER(C.c_int32)), n) == n
    return out


def bvh_ref_counts(flat):
    """The ref count of every BVH entry of the scene (FlatEntry: kind 2, c = ref count)."""
    e = np.frombuffer(flat.array("entries"), dtype=np.int32).reshape(-1, 40)
    return e[e[:, 0] == 2, 3]


class Answer:
    """d (n,), q (n, 3), ids (n, 4) and the batch's counters (box tests, primitive tests)."""

    def __init__(self, d, q, ids, counters=(0, 0)):
        self.d, self.q, self.ids, self.box_tests, self.prim_tests = d, q, ids, int(counters[0]), int(counters[1])

    @property
    def found(self):
        return self.ids[:, 1] >= 0


def _col(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def host(chk, flat, points, time=None, r_max=None, *, r_max_all=INF, media=False, f32=False, exhaustive=False):
    """A judge's answer to a batch."""
    points, time, r_max = _col(points), _col(time), _col(r_max)
    n = len(points)
    d, q, ids = np.full(n, -1.0), np.full((n, 3), -1.0), np.full((n, 4), -7, dtype=np.int32)
    cnt = (C.c_ulonglong * 2)()
    p = lambda a: a.ctypes.data_as(_D) if a is not None else None
    rc = chk[(f32, exhaustive)](flat.arrays_ptr(), n, p(points), p(time), p(r_max), r_max_all, 1 if media else 0, p(d), p(q),
                                ids.ctypes.data_as(C.POINTER(C.c_int32)), cnt)
    assert rc == 0, rc
    return Answer(d, q, ids, (cnt[0], cnt[1]))


def differing(a, b):
    """The points whose d, q or ids differ between two answers: by bit pattern, NaN equal to NaN."""
    same = cc.same_bits(a.d.reshape(-1, 1), b.d.reshape(-1, 1)) & cc.same_bits(a.q, b.q) & (a.ids == b.ids).all(axis=1)
    return np.flatnonzero(~same)


# ---- judge 2: the scenes ----------------------------------------------------------------------------------------------------------
class Case:
    """name, builder, world, flat; points drawn in the region of interest [lo, hi] (cast_rays_cases' aim box, where the scene's
    objects are: Book-2's mist sphere of radius 5000 is not what bounds it) grown by half its diagonal; times inside and outside
    the scene's shutter when it has one."""

    def __init__(self, name, builder, world, lo, hi, times=None, n=1000, seed=5, flat=None):
        self.name, self.builder, self.world = name, builder, world
        self.flat = flat if flat is not None else builder.flatten(world)
        rng = np.random.default_rng(seed)
        lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        grow = 0.5 * np.linalg.norm(hi - lo)
        self.points = np.ascontiguousarray((lo - grow) + rng.uniform(size=(n, 3)) * ((hi + grow) - (lo - grow)))
        # a mesh that is small in its room (the dragon) is never the nearest thing to a uniform point: a tenth of the points are
        # drawn next to vertices of the scene's triangles instead
        if self.flat.info()["n_triangles"] and n >= 100:
            v0 = np.frombuffer(self.flat.array("triangles"), dtype=np.float64).reshape(-1, 13)[:, :3]
            pick = v0[rng.integers(len(v0), size=n // 10)]
            self.points[:n // 10] = pick + rng.normal(size=pick.shape) * 0.002 * np.linalg.norm(hi - lo)
        self.time = None
        if times is not None:
            span = times[1] - times[0]
            self.time = np.ascontiguousarray(rng.uniform(times[0] - 0.5 * span, times[1] + 0.5 * span, n))
            self.time[:3] = (times[0], times[1], np.nan)


def _zoo(layout):
    """A zoo with a third of its points next to the aim points on or in its members: far from them the ground is nearest."""
    def make(rtsr):
        b, world, aim = member_zoo(rtsr, "instanced", layout, with_aim=True)
        c = Case("zoo_" + layout, b, world, (-8.0, -0.5, -6.5), (8.0, 6.0, 5.5), seed=40 + len(layout))
        rng = np.random.default_rng(41)
        k = len(c.points) // 3
        c.points[-k:] = np.asarray(aim, dtype=np.float64)[rng.integers(len(aim), size=k)] + rng.normal(size=(k, 3)) * 0.3
        return c
    return make


def _from_cast(name):
    def make(rtsr):
        c = (cc.F64_CASES.get(name) or oc.MEDIA_FREE[name])(rtsr)
        return Case(name, c.builder, c.world, c.box[0], c.box[1], times=c.time_range, flat=c.flat)
    return make


def _offset_scene(rtsr):
    """Every coordinate offset by 10^6 (integers: exact in f32, so the outward rounding of a plane adds no slack of its own), and
    points exactly on the spheres' box planes."""
    b = rtsr.Builder(1)
    m = b.lambertian((0.5, 0.5, 0.5))
    rng = np.random.default_rng(3)
    off = 1.0e6
    centres = off + rng.integers(-40, 40, size=(96, 3)).astype(np.float64)
    radii = rng.integers(1, 4, size=96).astype(np.float64)
    objs = [b.sphere(tuple(c), float(r), m) for c, r in zip(centres, radii)]
    for k in range(40):
        v = off + rng.integers(-40, 40, size=(3, 3)).astype(np.float64)
        if np.linalg.norm(np.cross(v[1] - v[0], v[2] - v[0])) > 0:
            objs.append(b.triangle(tuple(v[0]), tuple(v[1]), tuple(v[2]), m))
    world = b.hittable_list([b.bvh_from_list(b.hittable_list(objs), 0.0, 1.0), b.sphere((off, off + 60.0, off), 5.0, m)])
    c = Case("offset_1e6", b, world, (off - 40.0,) * 3, (off + 40.0,) * 3, n=700)
    on_planes = np.concatenate([centres + radii[:, None] * np.array(s) for s in ((1, 1, 1), (-1, 1, -1), (1, 0, 0), (0, -1, 0), (2, 2, -2))])
    c.points = np.ascontiguousarray(np.concatenate([c.points, on_planes]))
    return c


def _slack_probe(rtsr):
    """Where the slack of box_d2_lower decides.  A sphere of radius r = 1.96875 at the origin and p = (a, 0, 0) with
    a = 2.0263671875: a * (r / a) rounds UP, so the computed q.x = r + ulp(r) lies one ulp outside the sphere's box (planes at
    +-r, exact in f32) and the key is (gap - ulp(r))^2 with gap = a - r.  A rectangle at distance gap - ulp(r) / 2 is met
    first: farther than the sphere's computed point, nearer than its box.  Without the slack the box is dropped and the
    rectangle wins; the exhaustive scan finds the sphere.  (f64 numbers; in f32 the product does not round up and the case is
    an ordinary one.)"""
    b = rtsr.Builder(1)
    m = b.lambertian((0.5, 0.5, 0.5))
    r, a = 1.96875, 2.0263671875
    e = (a - r) - 0.5 * float(np.spacing(r))
    assert a * (r / a) > r and (a - r) - float(np.spacing(r)) < e < a - r
    pair = b.bvh_from_list(b.hittable_list([b.sphere((0.0, 0.0, 0.0), r, m), b.sphere((-50.0, 0.0, 0.0), 1.0, m)]), 0.0, 1.0)
    world = b.hittable_list([b.xz_rect(0.0, 4.0, -1.0, 1.0, -e, m), pair])
    c = Case("slack_probe", b, world, (-2.0, -2.0, -2.0), (3.0, 2.0, 2.0), n=8)
    c.points = np.ascontiguousarray([[a, 0.0, 0.0], [a, -0.03, 0.0], [a, 0.5, 0.25], [3.0, -0.05, 0.5], [-60.0, 1.0, 0.0], [1.0, 1.0, 1.0]])
    return c


def two_leaves(rtsr):
    """Where re-judging the far leaf after the near one is visible, by counting.  One BVH of two unit spheres ten apart (its
    root holds two leaf children) and points within a quarter of the first: once that sphere is tested the key is below 0.0625,
    the other's box is at least 8.75 away, so a walk that judges the second leaf against the CURRENT bound tests exactly one
    primitive a point -- and one that kept the bound it entered the node with tests two."""
    b = rtsr.Builder(1)
    m = b.lambertian((0.5, 0.5, 0.5))
    world = b.hittable_list([b.bvh_from_list(b.hittable_list([b.sphere((0.0, 0.0, 0.0), 1.0, m), b.sphere((10.0, 0.0, 0.0), 1.0, m)]), 0.0, 1.0)])
    c = Case("two_leaves", b, world, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), n=8)
    rng = np.random.default_rng(4)
    v = rng.normal(size=(200, 3))
    c.points = np.ascontiguousarray(v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.8, 1.2, (200, 1)))
    return c


def _tie_points(n=400, seed=9):
    """Points of the plane x = 0 with dyadic coordinates: equidistant, exactly, from anything mirrored in that plane."""
    rng = np.random.default_rng(seed)
    yz = rng.integers(-64, 64, size=(n, 2)) / 8.0
    return np.ascontiguousarray(np.column_stack([np.zeros(n), yz]))


def tie_scene(rtsr, kind, where, max_leaf=0, reference_bvh=False):
    """A mirrored pair (spheres or triangles) across x = 0 -- every operation of prim_nearest is sign-symmetric, so d2 is exactly
    equal for points of that plane -- at top level (where = "list": slots 0 and 1) or inside one BVH with two bystanders."""
    b = rtsr.Builder(1)
    m0, m1 = b.lambertian((0.9, 0.1, 0.1)), b.lambertian((0.1, 0.1, 0.9))
    if kind == "spheres":
        pair = [b.sphere((-2.0, 0.5, 0.25), 1.0, m0), b.sphere((2.0, 0.5, 0.25), 1.0, m1)]
    else:
        pair = [b.triangle((-1.0, 0.0, 0.0), (-3.0, 2.0, 0.5), (-2.0, -1.0, 3.0), m0), b.triangle((1.0, 0.0, 0.0), (3.0, 2.0, 0.5), (2.0, -1.0, 3.0), m1)]
    if kind == "spheres":
        far = [b.sphere((-40.0, 30.0, 0.0), 1.0, m0), b.sphere((40.0, 30.0, 0.0), 1.0, m1)]
    else:
        far = [b.triangle((-40.0, 30.0, 0.0), (-41.0, 31.0, 0.0), (-40.0, 31.0, 2.0), m0), b.triangle((40.0, 30.0, 0.0), (41.0, 31.0, 0.0), (40.0, 31.0, 2.0), m1)]
    world = b.hittable_list(pair + far) if where == "list" else b.hittable_list([b.bvh_from_list(b.hittable_list(pair + far), 0.0, 1.0)])
    c = Case("tie_%s_%s" % (kind, where), b, world, (-3.0, -2.0, -2.0), (3.0, 3.0, 4.0), n=8,
             flat=b.flatten(world, max_leaf=max_leaf, reference_bvh=reference_bvh))
    c.points = _tie_points()
    return c


def _chain(K):
    def make(rtsr):
        b, world, _, _, centres = lbvh_cases.chain(rtsr, K)
        c = Case("chain_%d" % K, b, world, (-2.0, -2.0, -2.0), (2.0 ** K,) * 3, n=300)
        c.points[:len(centres[:200])] = centres[:200] + 0.3
        return c
    return make


SCENES = {name: _from_cast(name) for name in ("moving_test", "mesh_room", "book2", "cornell_smoke", "slot_list")}
SCENES["zoo_middle"] = _zoo("middle")
SCENES["zoo_two"] = _zoo("two")
SCENES["offset_1e6"] = _offset_scene
SCENES["slack_probe"] = _slack_probe
# lbvh_cases' chains.  Here they are flattened by the host SAH builder, whose trees are shallow: the 49 and 61 levels they are
# known for come from the GPU builder, which has no host twin -- tests/test_gpu_nearest.py builds them there and holds the
# walk to the exhaustive scan on those trees.  On the CPU they are 1100 concentric and far-flung spheres, nothing more.
SCENES["chain_12"] = _chain(12)
SCENES["chain_16"] = _chain(16)
for _k in ("spheres", "triangles"):
    for _w in ("list", "bvh"):
        SCENES["tie_%s_%s" % (_k, _w)] = (lambda k, w: lambda rtsr: tie_scene(rtsr, k, w))(_k, _w)
ZOOS = ("zoo_middle", "zoo_two")
_built = {}


def case(rtsr, name):
    if name not in _built:
        _built[name] = SCENES[name](rtsr)
    return _built[name]


def finite_r_max(answer):
    """A radius that between a tenth and nine tenths of the points find something within: the median of the exhaustive scan's
    own distances (asserted by the caller on the scan's answers)."""
    d = answer.d[np.isfinite(answer.d)]
    return float(np.median(d)) if len(d) else 1.0


# ---- judge 1: closed forms, in longdouble from the scene's own numbers ------------------------------------------------------------
def _ld(a):
    return np.asarray(a, dtype=LD)


def _norm(v):
    return np.sqrt((v * v).sum(axis=-1))


class Closed:
    """flat, points (time, r_max, media), and the expected d (inf: nothing found) and q (unchecked where d is inf; None: any)
    as longdouble; magnitude: the largest coordinate of the case, which scales the tolerance."""

    def __init__(self, name, builder, world, points, d, q, *, time=None, r_max=None, media=False, prim_type=None):
        self.name, self.builder, self.flat = name, builder, builder.flatten(world)
        self.points, self.time, self.r_max, self.media = _col(points), _col(time), _col(r_max), media
        self.d, self.q, self.prim_type = _ld(d), (None if q is None else _ld(q)), prim_type
        self.magnitude = float(max(np.abs(self.points).max(), np.abs(self.q[np.isfinite(self.d)]).max() if q is not None and np.isfinite(self.d).any() else 0.0))


def tolerance(c, f32):
    """64 ulps of `real` at the case's largest coordinate: about twenty rounded operations of at most that magnitude each."""
    return 64.0 * (2.0 ** -23 if f32 else 2.0 ** -52) * c.magnitude


def _sphere_expect(p, c, r):
    p, c = _ld(p), _ld(c)
    v = p - c
    ln = _norm(v)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = c + v * (abs(LD(r)) / ln)[:, None]
    at_centre = ln == 0
    q[at_centre] = c + _ld([abs(r), 0.0, 0.0])
    return np.abs(ln - abs(LD(r))), q


def _unit_rows(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _segment_point(p, a, b):
    ab = b - a
    t = np.clip(((p - a) * ab).sum(axis=1) / (ab * ab).sum(), 0, 1)
    return a + t[:, None] * ab


def _triangle_expect(p, v0, v1, v2):
    """The closest point of a triangle: the plane projection where it falls inside, else the closest of the three edges."""
    p, v0, v1, v2 = _ld(p), _ld(v0), _ld(v1), _ld(v2)
    n = np.cross(v1 - v0, v2 - v0)
    n = n / _norm(n)
    proj = p - ((p - v0) * n).sum(axis=1)[:, None] * n
    inside = np.ones(len(p), dtype=bool)
    for a, b in ((v0, v1), (v1, v2), (v2, v0)):
        inside &= (np.cross(b - a, proj - a) * n).sum(axis=1) >= 0
    cands = [_segment_point(p, a, b) for a, b in ((v0, v1), (v1, v2), (v2, v0))]
    dist = np.stack([_norm(p - q) for q in cands])
    pick = dist.argmin(axis=0)
    q = np.stack(cands)[pick, np.arange(len(p))]
    q[inside] = proj[inside]
    return _norm(p - q), q


def _box_expect(p, lo, hi):
    """The closest point of a box's SURFACE: the clamp from outside, the nearest face from inside."""
    p, lo, hi = _ld(p), _ld(lo), _ld(hi)
    q = np.minimum(np.maximum(p, lo), hi)
    inside = (q == p).all(axis=1)
    for r in np.flatnonzero(inside):
        gaps = np.concatenate([p[r] - lo, hi - p[r]])
        k = int(gaps.argmin())
        q[r, k % 3] = lo[k % 3] if k < 3 else hi[k % 3]
    return _norm(p - q), q


def closed_form_cases(rtsr, f32=False):
    """Every closed-form case.  f32 only chooses what "one ulp below" means for the r_max case."""
    out = []
    rng = np.random.default_rng(17)
    grey = lambda b: b.lambertian((0.5, 0.5, 0.5))
    # spheres: outside, inside, on the surface, at the centre
    centre, radius = (1.0, 2.0, 3.0), 2.0
    u = _unit_rows(rng, 60)
    p = np.concatenate([np.asarray(centre) + u[:20] * rng.uniform(2.5, 9.0, (20, 1)), np.asarray(centre) + u[20:40] * rng.uniform(0.1, 1.9, (20, 1)),
                        np.asarray(centre) + u[40:] * radius, [centre]])
    b = rtsr.Builder(1)
    out.append(Closed("sphere", b, b.hittable_list([b.sphere(centre, radius, grey(b))]), p, *_sphere_expect(p, centre, radius), prim_type=PRIM_SPHERE))
    # radius -0.45 inside radius 0.5: the hollow-glass idiom, at top level and in a BVH
    c2 = (0.5, -1.0, 0.25)
    p = np.concatenate([np.asarray(c2) + _unit_rows(rng, 40) * rng.uniform(0.05, 1.5, (40, 1)), [c2]])
    da, qa = _sphere_expect(p, c2, 0.5)
    db, qb = _sphere_expect(p, c2, -0.45)
    d, q = np.where(da <= db, da, db), np.where((da <= db)[:, None], qa, qb)
    clear = np.abs(da - db) > 1e-3  # (not a tie within rounding)
    for where in ("list", "bvh"):
        b = rtsr.Builder(1)
        shell = [b.sphere(c2, 0.5, b.dielectric(1.5)), b.sphere(c2, -0.45, b.dielectric(1.5))]
        world = b.hittable_list(shell) if where == "list" else b.hittable_list([b.bvh_from_list(b.hittable_list(shell), 0.0, 1.0)])
        out.append(Closed("hollow_glass_" + where, b, world, p[clear], d[clear], q[clear], prim_type=PRIM_SPHERE))
    # rectangles: each axis, all nine clamp regions, p on the plane and off it
    ext = (-1.0, 2.0, 0.5, 1.75, 0.625)  # a0 a1 b0 b1 k
    grid = np.array([(a, bb, k) for a in (-2.5, 0.25, 3.5) for bb in (-0.75, 1.0, 2.5) for k in (0.0, 1.5, -0.75)])
    for axis, make, order in (("xy", "xy_rect", (0, 1, 2)), ("xz", "xz_rect", (0, 2, 1)), ("yz", "yz_rect", (1, 2, 0))):
        p = np.zeros((len(grid), 3))
        p[:, order[0]], p[:, order[1]], p[:, order[2]] = grid[:, 0], grid[:, 1], ext[4] + grid[:, 2]
        q = _ld(p).copy()
        q[:, order[0]] = np.clip(q[:, order[0]], ext[0], ext[1])
        q[:, order[1]] = np.clip(q[:, order[1]], ext[2], ext[3])
        q[:, order[2]] = ext[4]
        b = rtsr.Builder(1)
        out.append(Closed("rect_" + axis, b, b.hittable_list([getattr(b, make)(*ext, grey(b))]), p, _norm(_ld(p) - q), q, prim_type=PRIM_RECT))
        b = rtsr.Builder(1)
        out.append(Closed("rect_inverted_" + axis, b, b.hittable_list([getattr(b, make)(2.0, -1.0, 0.5, 1.75, 0.625, grey(b))]), p,
                          np.full(len(p), INF), None))
    # triangles: the seven regions, from both sides of the plane
    v = np.array([(0.0, 0.0, 0.0), (2.0, 0.0, 0.5), (0.5, 1.5, 0.0)])
    n = np.cross(v[1] - v[0], v[2] - v[0])
    n /= np.linalg.norm(n)
    cen = v.mean(axis=0)
    spots = [cen] + [v[k] + 1.3 * (v[k] - cen) for k in range(3)]
    for a, bb in ((0, 1), (0, 2), (1, 2)):
        mid = 0.5 * (v[a] + v[bb])
        spots.append(mid + 1.1 * (mid - v[3 - a - bb]))
    p = np.concatenate([np.asarray(spots) + h * n for h in (0.0, 0.8, -0.6)])
    b = rtsr.Builder(1)
    out.append(Closed("triangle", b, b.hittable_list([b.triangle(*map(tuple, v), grey(b))]), p, *_triangle_expect(p, *v), prim_type=PRIM_TRIANGLE))
    b = rtsr.Builder(1)
    out.append(Closed("triangle_zero_area", b, b.hittable_list([b.triangle((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0), grey(b))]), p,
                      np.full(len(p), INF), None))
    # MovingSpheres inside a BVH: inside the interval (0, 0.25, 1) and outside it (1.5, -1: the mover rule)
    movers = [((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), 0.5), ((0.0, 5.0, 0.0), (0.0, 5.0, 4.0), 0.75), ((-3.0, 2.0, 1.0), (-3.0, 4.0, 1.0), 0.25)]
    times = np.repeat([0.0, 0.25, 1.0, 1.5, -1.0], 12)
    p = rng.uniform(-6.0, 8.0, (len(times), 3))
    best_d, best_q = np.full(len(p), LD(INF)), np.zeros((len(p), 3), dtype=LD)
    for c0, c1, r in movers:
        cen_t = _ld(c0) + _ld(times)[:, None] * (_ld(c1) - _ld(c0))
        vv = _ld(p) - cen_t
        ln = _norm(vv)
        d = np.abs(ln - LD(r))
        q = cen_t + vv * (LD(r) / ln)[:, None]
        take = d < best_d
        best_d, best_q = np.where(take, d, best_d), np.where(take[:, None], q, best_q)
    b = rtsr.Builder(1)
    objs = [b.moving_sphere(c0, c1, 0.0, 1.0, r, grey(b)) for c0, c1, r in movers]
    out.append(Closed("moving_spheres_bvh", b, b.hittable_list([b.bvh_from_list(b.hittable_list(objs), 0.0, 1.0)]), p, best_d, best_q,
                      time=times, prim_type=PRIM_MOVING_SPHERE))
    b = rtsr.Builder(1)
    out.append(Closed("moving_sphere_time0_is_time1", b, b.hittable_list([b.moving_sphere((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.5, 0.5, 1.0, grey(b))]),
                      p, np.full(len(p), INF), None, time=times))
    # a RectPrism under Translate(RotateY(30 deg)), from inside and outside
    lo, hi, angle, offset = (-1.0, 0.5, 2.0), (2.0, 2.5, 3.5), 30.0, (4.0, -1.0, 2.0)
    th = LD(angle) * (LD(4) * np.arctan(LD(1))) / LD(180)
    s, c = np.sin(th), np.cos(th)
    local = np.concatenate([rng.uniform(-4.0, 5.0, (40, 3)), np.asarray(lo) + rng.uniform(0.05, 0.95, (25, 3)) * (np.asarray(hi) - np.asarray(lo))])
    d, ql = _box_expect(local, lo, hi)
    out_of = lambda x: np.stack([c * x[:, 0] + s * x[:, 2], x[:, 1], -s * x[:, 0] + c * x[:, 2]], axis=1) + _ld(offset)
    b = rtsr.Builder(1)
    world = b.hittable_list([b.translate(offset, b.rotate_y(angle, b.rect_prism(lo, hi, grey(b))))])
    out.append(Closed("prism_moved", b, world, out_of(_ld(local)).astype(np.float64), d, out_of(ql), prim_type=PRIM_RECT))
    # a ConstantMedium ball: skipped with media = 0, its boundary with media = 1
    p = np.asarray(centre) + _unit_rows(rng, 30) * rng.uniform(0.2, 6.0, (30, 1))
    for media in (False, True):
        b = rtsr.Builder(1)
        world = b.hittable_list([b.constant_medium((0.8, 0.8, 0.8), 0.37, b.sphere(centre, radius, grey(b)))])
        d, q = _sphere_expect(p, centre, radius)
        out.append(Closed("fog_ball_media%d" % media, b, world, p, d if media else np.full(len(p), INF), q if media else None, media=media))
    # r_max exactly at d (found), one ulp of `real` below (not found), NaN (not found), +inf: as a per-point column
    below = float(np.nextafter(np.float32(2.0), np.float32(0.0))) if f32 else float(np.nextafter(2.0, 0.0))
    p = np.tile([[0.25, 0.25, 2.0]], (4, 1))
    b = rtsr.Builder(1)
    out.append(Closed("r_max_column", b, b.hittable_list([b.xy_rect(-1.0, 1.0, -1.0, 1.0, 0.0, grey(b))]), p, [2.0, INF, INF, 2.0],
                      np.tile([[0.25, 0.25, 0.0]], (4, 1)), r_max=[2.0, below, np.nan, INF], prim_type=PRIM_RECT))
    return out


def check_closed(c, got, f32):
    """got (an Answer or a Nearest) against the case's closed form -> (worst |d| error, worst |q| error, tolerance)."""
    found = np.isfinite(c.d)
    assert np.array_equal(np.asarray(got.ids[:, 1] >= 0), found), c.name
    assert np.all(np.isinf(got.d[~found])) and np.all(got.q[~found] == 0.0) and np.all(got.ids[~found] == -1), c.name
    tol = tolerance(c, f32)
    ed = float(np.max(np.abs(_ld(got.d[found]) - c.d[found]))) if found.any() else 0.0
    eq = float(np.max(np.abs(_ld(got.q[found]) - c.q[found]))) if found.any() and c.q is not None else 0.0
    if c.prim_type is not None and found.any():
        assert np.all(got.ids[found, 2] == c.prim_type), c.name
    return ed, eq, tol
