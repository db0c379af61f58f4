"""The host checker, scenes and ray sets of tests/test_occlusion_cases.py and tests/test_gpu_occlusion.py (a helper module, not a
test file): everything here runs on the CPU.

The judge is tests/occlusion_host_check.cpp -- a plain loop over rays calling world_occlusion<rt::F_ALL> -- built with
oracle/Makefile's CXXFLAGS: once as it is (f64) and once with o2_flat_f32.cpp's four defines (the float judge, linked to
liboracle.so for oracle_f32_images).  Scenes and rays are those of tests/cast_rays_cases.py and tests/instance_scenes.py,
reduced to what has no medium; the closed-form scenes, the media segments and the stream experiment are built here."""
import ctypes as C
import os
import subprocess

import numpy as np

import cast_rays_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "occlusion_host_check.cpp")
ORACLE_BUILD = os.path.join(ROOT, "oracle", "_build")
# oracle/Makefile's CXXFLAGS (the O2 checker's)
CXXFLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-pthread"]
HOST_SOURCES = [os.path.join(ROOT, "ray-tracing-series-rust_amd", "csrc", "host", f)
                for f in ("scene_graph.cpp", "flatten.cpp", "bvh_build.cpp", "scenes.cpp")]
SANFLAGS = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-omit-frame-pointer",
            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-pthread"]

T_MIN = cc.T_MIN
SEG_EPS = 1e-6          # Scene.occlusion_between's default: t_max_all = 1 - eps
ENTRY_MEDIUM = 4        # Flat.top_level_kinds()
INF = float("inf")

_D = C.POINTER(C.c_double)
_ARGS = [C.c_void_p, C.c_int64, _D, _D, _D, _D, C.c_double, C.c_double, _D]
_checkers = {}


def checkers(tmp_path_factory):
    """{False: the f64 judge's entry, True: the float judge's}, built once per session (needs liboracle.so: the orc fixture)."""
    if not _checkers:
        d = tmp_path_factory.mktemp("occlusion_host")
        out64, out32 = str(d / "occlusion_host_check.so"), str(d / "occlusion_host_check_f32.so")
        subprocess.run(["g++"] + CXXFLAGS + ["-shared", SRC, "-o", out64], check=True)
        subprocess.run(["g++"] + CXXFLAGS + ["-DOCCLUSION_HOST_F32", "-shared", SRC, os.path.join(ORACLE_BUILD, "liboracle.so"),
                        "-Wl,-rpath," + ORACLE_BUILD, "-o", out32], check=True)
        for f32, path, name in ((False, out64, "occlusion_host"), (True, out32, "occlusion_host_f32")):
            fn = getattr(C.CDLL(path), name)
            fn.restype, fn.argtypes = C.c_int, _ARGS
            _checkers[f32] = fn
    return _checkers


def host_tau(chk, flat, o, d, time=None, t_max=None, *, t_min=T_MIN, t_max_all=INF, f32=False):
    """The judge's tau of a batch."""
    n = len(o)
    o, d = np.ascontiguousarray(o, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
    time = None if time is None else np.ascontiguousarray(time, dtype=np.float64)
    t_max = None if t_max is None else np.ascontiguousarray(t_max, dtype=np.float64)
    tau = np.full(n, -1.0)
    p = lambda a: a.ctypes.data_as(_D) if a is not None else None
    rc = chk[f32](flat.arrays_ptr(), n, p(o), p(d), p(time), p(t_max), t_min, t_max_all, p(tau))
    assert rc == 0, rc
    return tau


def same_bits(a, b):
    """cast_rays_cases.same_bits over (n,) arrays -> one boolean per ray."""
    return cc.same_bits(np.asarray(a).reshape(len(a), 1), np.asarray(b).reshape(len(b), 1))


def medium_slots(flat):
    return [i for i, k in enumerate(flat.top_level_kinds()) if k == ENTRY_MEDIUM]


# ---- 1. the media-free cases: cast_rays_cases' scenes without a medium, the hand-built list of tests/test_gpu_cast_rays.py, and
# the two medium scenes with every density set to 0 (Flat.set_shading) ----
def _slot_list(rtsr):
    """Eight spheres in a list (one under an identity Translate) and a BvhNode of two more: PRIM, XFORM and BVH entries."""
    b = rtsr.Builder(1)
    shared = b.lambertian((0.5, 0.5, 0.5))
    mats = [shared, b.lambertian((0.1, 0.2, 0.3)), shared, b.metal((0.8, 0.8, 0.8), 0.1), b.dielectric(1.5),
            b.lambertian((0.3, 0.2, 0.1)), b.metal((0.7, 0.6, 0.5), 0.0), b.lambertian((0.9, 0.9, 0.9))]
    objs = [b.sphere((3.0 * k, 0.0, 0.0), 1.0, m) for k, m in enumerate(mats)]
    objs[3] = b.translate((0.0, 0.0, 0.0), objs[3])
    pair = [b.sphere((24.0, 0.0, 0.0), 1.0, b.lambertian((0.2, 0.9, 0.2))), b.sphere((27.0, 0.0, 0.0), 1.0, b.lambertian((0.9, 0.2, 0.2)))]
    objs.append(b.bvh_from_list(b.hittable_list(pair), 0.0, 1.0))
    return cc.Case("slot_list", b, b.hittable_list(objs), (-2.0, -2.0, -2.0), (29.0, 2.0, 2.0), 0.8, seed=11)


def _without_density(factory):
    def make(rtsr):
        case = factory(rtsr)
        slots = medium_slots(case.flat)
        assert slots
        case.flat.set_shading([("medium_density", s, 0.0) for s in slots])
        case.name += "_density0"
        return case
    return make


MEDIA_FREE = {name: cc.F64_CASES[name] for name in ("moving_test", "gravity_t0.37", "gravity_t6.2", "mesh_room", "zoo_middle", "zoo_two")}
MEDIA_FREE["slot_list"] = _slot_list
MEDIA_FREE["cornell_smoke_density0"] = _without_density(cc.F64_CASES["cornell_smoke"])
MEDIA_FREE["book2_density0"] = _without_density(cc.F64_CASES["book2"])
MEDIA = {name: cc.F64_CASES[name] for name in cc.MEDIUM_CASES}
_built = {}


def case(rtsr, orc, name):
    """The named case with its 2000 rays (built once, with the f64 oracle); no device is touched."""
    if name not in _built:
        c = (MEDIA_FREE.get(name) or MEDIA[name])(rtsr).build_rays(orc)
        assert c.n == 2000
        c.hit_flags = {}
        _built[name] = c
    return _built[name]


# core32_world_hit narrows the WHOLE flat scene on every call.  Scene 8 carries the GravitySpheres' height tables (about
# 100 000 doubles a ball): half a second a ray, twenty minutes for a 2000-ray set.  The float oracle is asked about every
# GRAVITY_F32_STRIDE-th ray of these two cases only; every other case is asked ray for ray in both precisions.
GRAVITY_F32_STRIDE = 83


def oracle_rays(c, f32):
    """The indices of the rays the oracle of that precision is asked about (see above)."""
    return np.arange(0, c.n, GRAVITY_F32_STRIDE if f32 and c.name.startswith("gravity") else 1)


def oracle_hit_flags(orc, c, f32):
    """The hit flag of core_world_hit / core32_world_hit for the rays oracle_rays names (computed once per precision)."""
    if f32 not in c.hit_flags:
        probe = orc.core32_world_hit if f32 else orc.core_world_hit
        ptr = c.flat.arrays_ptr()
        c.hit_flags[f32] = np.array([probe(ptr, tuple(c.o[r]), tuple(c.d[r]), float(c.time[r]), T_MIN, float(c.t_max[r]), rng_seed=1) is not None
                                     for r in oracle_rays(c, f32)])
    return c.hit_flags[f32]


# ---- 2. closed forms.  Every expected value is computed here in numpy longdouble from the scene's own numbers. ----
LD = np.longdouble
RHO = 0.37


def _ld(a):
    return np.asarray(a, dtype=LD)


def _sphere_interval(o, d, centre, radius):
    """(t_in, t_out) of the lines o + t d through a sphere, longdouble; NaN where the line misses."""
    o, d, c = _ld(o), _ld(d), _ld(centre)
    oc = o - c
    a = (d * d).sum(axis=1)
    hb = (oc * d).sum(axis=1)
    disc = hb * hb - a * ((oc * oc).sum(axis=1) - LD(radius) * LD(radius))
    s = np.sqrt(np.where(disc > 0, disc, LD("nan")))
    return (-hb - s) / a, (-hb + s) / a


def _box_interval(o, d, lo, hi):
    """(t_in, t_out) of the lines through an axis-aligned box, longdouble; NaN where the line misses (no zero components)."""
    o, d = _ld(o), _ld(d)
    ta, tb = (_ld(lo) - o) / d, (_ld(hi) - o) / d
    t_in, t_out = np.minimum(ta, tb).max(axis=1), np.maximum(ta, tb).min(axis=1)
    miss = t_in >= t_out
    return np.where(miss, LD("nan"), t_in), np.where(miss, LD("nan"), t_out)


def _depth(t_in, t_out, d, density, t_min, t_max):
    """density x the length of [max(t_in, t_min, 0), min(t_out, t_max)] along d, 0 where empty or where the line misses."""
    t1 = np.maximum(np.maximum(t_in, LD(t_min)), LD(0))
    t2 = np.minimum(t_out, _ld(t_max))
    length = np.sqrt((_ld(d) ** 2).sum(axis=1))
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(t_in) | (t1 >= t2), LD(0), LD(density) * (t2 - t1) * length)


def _aimed(n, seed, centre, reach, spread):
    """n rays from the sphere of radius `reach` around centre towards uniform points within `spread` of it (not normalised)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    o = np.asarray(centre) + reach * v / np.linalg.norm(v, axis=1, keepdims=True)
    w = rng.normal(size=(n, 3))
    target = np.asarray(centre) + spread * rng.uniform(size=(n, 1)) ** (1.0 / 3.0) * w / np.linalg.norm(w, axis=1, keepdims=True)
    return np.ascontiguousarray(o), np.ascontiguousarray((target - o) * rng.uniform(0.3, 2.5, size=(n, 1)))


class Closed:
    """A closed-form case: flat, rays (o, d, t_max per ray), t_min and the expected tau as longdouble (inf: blocked)."""

    def __init__(self, name, builder, world, o, d, t_max, expected, t_min=T_MIN):
        self.name, self.builder, self.flat = name, builder, builder.flatten(world)
        self.o, self.d = np.ascontiguousarray(o, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
        self.t_max = np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, dtype=np.float64), (len(o),)))
        self.t_min, self.expected = t_min, _ld(expected)


def closed_form_cases(rtsr):
    out = []
    n = 60
    centre, radius = (1.0, 2.0, 3.0), 2.0

    def fog_world(density=RHO, extra=(), first=()):
        b = rtsr.Builder(1)
        fog = b.constant_medium((0.8, 0.8, 0.8), density, b.sphere(centre, radius, b.lambertian((0.5, 0.5, 0.5))))
        return b, list(first(b) if first else []) + [fog] + list(extra(b) if extra else [])

    # a fog sphere: density x chord (aimed inside 0.9 R: every chord is at least 0.87 R), and lines that pass it: 0
    o, d = _aimed(n, 1, centre, 7.0, 0.9 * radius)
    o2, d2 = _aimed(10, 2, (1.0, 9.0, 3.0), 7.0, 1.0)
    o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
    b, objs = fog_world()
    t_in, t_out = _sphere_interval(o, d, centre, radius)
    out.append(Closed("fog_sphere", b, b.hittable_list(objs), o, d, INF, _depth(t_in, t_out, d, RHO, T_MIN, INF)))
    # density 0: +0 on the same rays
    b, objs = fog_world(density=0.0)
    out.append(Closed("fog_sphere_density0", b, b.hittable_list(objs), o, d, INF, np.zeros(len(o))))
    # cut by t_max inside the fog, and before it
    t_cut = np.where(np.isnan(t_in), 1.0, t_in + (t_out - t_in) * np.linspace(-0.3, 0.95, len(o))).astype(np.float64)
    b, objs = fog_world()
    out.append(Closed("fog_sphere_cut", b, b.hittable_list(objs), o, d, t_cut, _depth(t_in, t_out, d, RHO, T_MIN, t_cut)))
    # a segment that starts inside: with the default t_min the part after t_min, with t_min < rec1.t < 0 the part after the origin
    oi, di = _aimed(n, 3, centre, 0.6 * radius, 0.3 * radius)
    t_in, t_out = _sphere_interval(oi, di, centre, radius)
    assert np.all(t_in < -0.01) and np.all(t_out > 0.01)
    for name, t_min in (("fog_sphere_from_inside", T_MIN), ("fog_sphere_from_inside_t_min_behind", -50.0)):
        b, objs = fog_world()
        out.append(Closed(name, b, b.hittable_list(objs), oi, di, INF, _depth(t_in, t_out, di, RHO, t_min, INF), t_min=t_min))
    # two overlapping fog spheres: the sum
    c2, r2, rho2 = (2.5, 2.0, 3.5), 1.5, 1.9
    b = rtsr.Builder(1)
    grey = b.lambertian((0.5, 0.5, 0.5))
    world = b.hittable_list([b.constant_medium((0.8, 0.8, 0.8), RHO, b.sphere(centre, radius, grey)),
                             b.constant_medium((0.2, 0.2, 0.2), rho2, b.sphere(c2, r2, grey))])
    o, d = _aimed(n, 4, (1.7, 2.0, 3.2), 8.0, 1.0)
    ia, ib = _sphere_interval(o, d, centre, radius), _sphere_interval(o, d, c2, r2)
    out.append(Closed("two_fog_spheres", b, world, o, d, INF, _depth(*ia, d, RHO, T_MIN, INF) + _depth(*ib, d, rho2, T_MIN, INF)))
    # a fog box (RectPrism), plain and under Translate(RotateY(.))
    lo, hi = (-1.0, 0.5, 2.0), (2.0, 2.5, 3.5)
    o, d = _aimed(n, 5, (0.5, 1.5, 2.75), 6.0, 0.6)
    b = rtsr.Builder(1)
    world = b.hittable_list([b.constant_medium((0.8, 0.8, 0.8), RHO, b.rect_prism(lo, hi, b.lambertian((0.5, 0.5, 0.5))))])
    out.append(Closed("fog_box", b, world, o, d, INF, _depth(*_box_interval(o, d, lo, hi), d, RHO, T_MIN, INF)))
    angle, offset = 33.0, (4.0, -1.0, 2.0)
    b = rtsr.Builder(1)
    box = b.translate(offset, b.rotate_y(angle, b.rect_prism(lo, hi, b.lambertian((0.5, 0.5, 0.5)))))
    world = b.hittable_list([b.constant_medium((0.8, 0.8, 0.8), RHO, box)])
    # the ray in the box's frame (xform_ray): minus the offset, then x' = cos x - sin z, z' = sin x + cos z
    th = LD(angle) * (LD(4) * np.arctan(LD(1))) / LD(180)
    s, c = np.sin(th), np.cos(th)
    rot = lambda v: np.stack([c * v[:, 0] - s * v[:, 2], v[:, 1], s * v[:, 0] + c * v[:, 2]], axis=1)
    # aim at the box where it stands in the world: the centre rotated back and moved
    cen = _ld([[0.5, 1.5, 2.75]])
    wc = np.stack([c * cen[:, 0] + s * cen[:, 2], cen[:, 1], -s * cen[:, 0] + c * cen[:, 2]], axis=1)[0] + _ld(offset)
    o, d = _aimed(n, 6, tuple(float(x) for x in wc), 6.0, 0.6)
    ob, db = rot(_ld(o) - _ld(offset)), rot(_ld(d))
    out.append(Closed("fog_box_moved", b, world, o, d, INF, _depth(*_box_interval(ob, db, lo, hi), db, RHO, T_MIN, INF)))
    # a wall behind, in front of and inside the fog, in either slot order: +inf.  The rays run along +z through the sphere.
    rng = np.random.default_rng(7)
    o = np.column_stack([centre[0] + rng.uniform(-1.0, 1.0, 20), centre[1] + rng.uniform(-1.0, 1.0, 20), np.full(20, -4.0)])
    d = np.column_stack([rng.uniform(-0.02, 0.02, 20), rng.uniform(-0.02, 0.02, 20), np.full(20, 1.3)])
    for where, z in (("behind", 6.5), ("in_front", -1.0), ("inside", 3.2)):
        for order in ("wall_first", "fog_first"):
            wall = lambda b: [b.xy_rect(-9.0, 9.0, -9.0, 9.0, z, b.lambertian((0.7, 0.7, 0.7)))]
            b, objs = fog_world(first=wall) if order == "wall_first" else fog_world(extra=wall)
            out.append(Closed("wall_%s_%s" % (where, order), b, b.hittable_list(objs), o, d, INF, np.full(20, INF)))
    # ... and the same wall past t_max does not block: the fog's own depth
    b, objs = fog_world(extra=lambda b: [b.xy_rect(-9.0, 9.0, -9.0, 9.0, 6.5, b.lambertian((0.7, 0.7, 0.7)))])
    t_in, t_out = _sphere_interval(o, d, centre, radius)
    out.append(Closed("wall_past_t_max", b, b.hittable_list(objs), o, d, 8.0, _depth(t_in, t_out, d, RHO, T_MIN, 8.0)))
    return out


def relative_error(tau, expected):
    """max |tau - expected| / expected over the rays with a finite expected value > 0 (longdouble); every other ray must be equal."""
    tau, expected = _ld(tau), _ld(expected)
    pos = np.isfinite(expected) & (expected > 0)
    rest_equal = bool(np.all(tau[~pos] == expected[~pos]) and not np.signbit(tau[~pos & (expected == 0)]).any())
    return (float(np.max(np.abs(tau[pos] - expected[pos]) / expected[pos])) if pos.any() else 0.0), rest_equal


# ---- 3. segments through media ----
ROOM_LO, ROOM_HI = -40.0, 595.0  # a box a little larger than the Cornell room (0 .. 555), fitted to the three-way mix below


def segments(n=2000, seed=21, lo=ROOM_LO, hi=ROOM_HI):
    """n segments between uniform point pairs of the cube [lo, hi]^3 -> (a, b)."""
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(lo, hi, size=(n, 3)), rng.uniform(lo, hi, size=(n, 3))
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def segment_tau(chk, flat, a, b, f32=False, time=None):
    """What Scene.occlusion_between(a, b) asks: direction b - a, [0.001, 1 - eps]."""
    return host_tau(chk, flat, a, b - a, time, None, t_min=T_MIN, t_max_all=1.0 - SEG_EPS, f32=f32)


def stream_miss_share(orc, flat, a, b, streams, seed, time=0.0):
    """The share of `streams` streams on which core_world_hit reports no hit at all on the segment a -> b."""
    ptr, o, d = flat.arrays_ptr(), tuple(a), tuple(b - a)
    return sum(orc.core_world_hit(ptr, o, d, time, T_MIN, 1.0 - SEG_EPS, rng_seed=seed + k) is None for k in range(streams)) / streams
