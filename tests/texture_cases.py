"""Textures at their edges: every kind, nesting depth and (u, v) rule (a helper module, not a test file; all of it runs on the
CPU).  tests/test_texture_cases.py proves the cases against judges that share no code with the kernels;
tests/test_gpu_texture_cases.py runs the device on them.

The probe.  An axis-aligned rectangle, a sphere or a triangle carries diffuse_light(texture) under a black background and
one ray is aimed at a chosen point: trace_rays(spp=1, max_depth=1) then returns Texture::value(u, v, p) itself, bit for bit
(tests/light_cases.py: "aimed rays at max_depth 1 are Le").  A ray runs along an axis from distance 1 (o = p + e, d = -e)
onto a plane at a dyadic coordinate, so t = 1 and the hit point's two other coordinates are the origin's, exactly.  The
scatter form puts the texture under a Lambertian on a single rectangle with background (1, 1, 1) and max_depth = 2: the
scattered ray always escapes and the sum is the texture value again.

The judges, from most to least independent (a case names the ones that hold it, Case.judges):
  closed   Python alone: checker parity from the double 10 x against multiples of a 60-digit pi in `decimal` (no sine is
           called), the texel named from (u, v) in `fractions` with every rounding of the f64 expression spelled out, Perlin
           noise at lattice points (every octave exactly 0), over a period of 256 and beyond the range of i32
  numpy    perlin_restated: perlin.rs:28-106 and texture.rs:80-88 in float64, operation by operation in the reference's
           order (IEEE arithmetic: the same bits up to the final sine, which is the project's rt_sin), reading the tables
           through orc.flat_array
  o1       oracle_o1_texture_value / orc.o1_hit: the literal restatement, which recurses to any depth
  host     trace_rays_cases.host_trace, f64 and float: what ties the device run to the core

build(rtsr, name, **variant) returns a Case: the builder, the world, the probes and the case's conditions (Case.conditions:
(text, bool) pairs that make it a test of its edge; the CPU tests assert every one)."""
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

getcontext().prec = 80
PI60 = Decimal("3.14159265358979323846264338327950288419716939937510582097494")
BLACK, WHITE = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
AXES = np.eye(3)
FRAME_WIDTH, FRAME_SPP = 32, 2
MAX_CHAIN = 16  # the longest checker chain the flattener admits (include/rtx_abi.h: rtx_checker)


# ---------------------------------------------------------------------------------------------------- closed forms
def sin_sign_of_10x(x, f32=False):
    """The sign (-1, 0, 1) of sin(fl(10 x)) without a sine: fl(10 x) is the double the reference forms; its place among the
    multiples of pi is decided in 80-digit decimal arithmetic with a 60-digit pi.  (A double is a multiple of pi only at 0, and
    the nearest one comes no closer than 1e-19 relative: 60 digits decide every case here.)"""
    y = float(np.float32(10.0) * np.float32(x)) if f32 else float(10.0 * float(x))  # f32: the float core's 10 x, rounded to float
    if y == 0.0:
        return 0
    q = Decimal(y) / PI60  # Decimal(float) is exact
    m = int(q.to_integral_value(rounding="ROUND_FLOOR"))
    assert abs(q - q.to_integral_value()) > Decimal("1e-30"), x
    return 1 if m % 2 == 0 else -1


def checker_is_odd(p, f32=False):
    """texture.rs:56-62: sines < 0 picks the odd child; a zero factor makes the product +-0: even."""
    s = [sin_sign_of_10x(c, f32) for c in p]
    return s[0] * s[1] * s[2] < 0


def _fl(q):
    """A rational rounded to the nearest double (Python's int / int is correctly rounded)."""
    return q.numerator / q.denominator


def rect_uv(x, a0, a1):
    """(x - a0) / (a1 - a0) as the f64 expression of hit.rs's rectangles, each operation exact in `fractions` then rounded."""
    num, den = _fl(Fraction(x) - Fraction(a0)), _fl(Fraction(a1) - Fraction(a0))
    return _fl(Fraction(num) / Fraction(den))


def _clamp01(x):
    """mutil.rs:1-9: a NaN falls through both comparisons and is returned."""
    if x < 0.0:
        return 0.0
    if x > 1.0:
        return 1.0
    return x


def _as_i32(x):
    """Rust's `as i32`: truncates, saturates, NaN -> 0."""
    if x != x:
        return 0
    return int(max(-2.0 ** 31, min(2.0 ** 31 - 1, np.trunc(x))))


def texel_index(u, v, width, height):
    """texture.rs:102-121 -> (row j, column i) of the texel Image::value(u, v) reads."""
    uc, vc = _clamp01(u), _clamp01(v)
    vc = vc if vc != vc else _fl(1 - Fraction(vc))
    ui = uc if uc != uc else _fl(Fraction(uc) * width)
    vj = vc if vc != vc else _fl(Fraction(vc) * height)
    return min(_as_i32(vj), height - 1), min(_as_i32(ui), width - 1)


def image_value(texels, u, v):
    j, i = texel_index(u, v, texels.shape[1], texels.shape[0])
    return (1.0 / 255.0) * texels[j, i]


def make_texels(width, height, base):
    """Every number distinct within the image (so is every texel, and row 0 from the last row), all <= 255."""
    t = base + np.arange(height * width * 3, dtype=np.float64).reshape(height, width, 3)
    assert t.max() <= 255.0
    return t


# ---------------------------------------------------------------------------------------------------- numpy restatement
PERLIN = np.dtype([("ranvec", np.float64, (256, 3)), ("perm_x", np.int32, (256,)), ("perm_y", np.int32, (256,)), ("perm_z", np.int32, (256,))])


def perlin_tables(orc, flat):
    raw, e = orc.flat_array(flat.arrays_ptr(), "perlins")
    assert e == PERLIN.itemsize == 9216
    return raw.view(PERLIN)


def _noise(tab, p, trace=None):
    """perlin.rs:28-52 + 85-106."""
    f = np.float64
    fl = [np.floor(f(c)) for c in p]
    u, v, w = [f(c) - g for c, g in zip(p, fl)]
    i, j, k = [_as_i32(g) for g in fl]

    def wrap(n, d):  # i + d in wrapping i32 arithmetic, & 255
        return ((n + d + 2 ** 31) % 2 ** 32 - 2 ** 31) & 255
    if trace is not None:
        trace.append(([wrap(i, 0), wrap(i, 1)], [wrap(j, 0), wrap(j, 1)], [wrap(k, 0), wrap(k, 1)], (float(u), float(v), float(w))))
    uu = u * u * (f(3.0) - f(2.0) * u)
    vv = v * v * (f(3.0) - f(2.0) * v)
    ww = w * w * (f(3.0) - f(2.0) * w)
    accum = f(0.0)
    for di in range(2):
        for dj in range(2):
            for dk in range(2):
                c = tab["ranvec"][tab["perm_x"][wrap(i, di)] ^ tab["perm_y"][wrap(j, dj)] ^ tab["perm_z"][wrap(k, dk)]]
                i1, j1, k1 = f(di), f(dj), f(dk)
                wx, wy, wz = u - i1, v - j1, w - k1
                dot = c[0] * wx + c[1] * wy + c[2] * wz
                accum = accum + (i1 * uu + (f(1.0) - i1) * (f(1.0) - uu)) * (j1 * vv + (f(1.0) - j1) * (f(1.0) - vv)) * \
                    (k1 * ww + (f(1.0) - k1) * (f(1.0) - ww)) * dot
    return accum


def perlin_restated(orc, tab, scale, p, trace=None):
    """texture.rs:80-88 over perlin.rs:54-66 in float64, in the reference's order -> the grey value (all three channels)."""
    f = np.float64
    with np.errstate(all="ignore"):
        accum, weight, tp = f(0.0), f(1.0), [f(c) for c in p]
        for _ in range(7):
            accum = accum + weight * _noise(tab, tp, trace)
            weight = weight * f(0.5)
            tp = [c * f(2.0) for c in tp]
        arg = f(scale) * f(p[2]) + f(10.0) * np.abs(accum)
        return float(f(0.5) * (f(1.0) + orc.rt_math("sin", [arg])[0]))


# ---------------------------------------------------------------------------------------------------- cases
class Probe:
    """One ray and what is known of its answer.  tex, u, v, p: the Texture::value call the ray comes to (None where only O1's
    hit record can say); expected: the closed form's rgb or None; f32: the float mode may be held on it."""

    def __init__(self, o, d, tex=None, u=0.0, v=0.0, p=None, expected=None, tag="", time=0.0, f32=True, handle=None):
        self.o, self.d, self.tex, self.u, self.v, self.p = tuple(o), tuple(d), tex, u, v, None if p is None else tuple(p)
        self.expected, self.tag, self.time, self.f32, self.handle = expected, tag, time, f32, handle


class Case:
    def __init__(self, name, rtsr, judges, background=BLACK, max_depth=1):
        self.name, self.judges, self.background, self.max_depth = name, judges, background, max_depth
        self.b = rtsr.Builder(31)
        self.objects, self.probes, self.conditions, self.cam, self.world = [], [], [], None, None
        self.extra, self.planes = {}, []  # planes: (normal axis, k) of every axis-aligned rectangle of the world

    def finish(self, rtsr, lookfrom, lookat, vfov=40.0, vup=(0.0, 0.0, -1.0), bvh=False):
        if bvh:
            self.world = self.b.hittable_list([self.b.bvh_from_list(self.b.hittable_list(self.objects), 0.0, 1.0)])
        else:
            self.world = self.b.hittable_list(self.objects)
        self.cam = rtsr.Camera.new(lookfrom, lookat, vup, vfov, 1.0, 0.0, 10.0, 0.0, 1.0)
        self.cfg = rtsr.Config.new(1.0, FRAME_WIDTH, FRAME_SPP, 4, 4, seed=5, background=self.background)
        self.flat = self.b.flatten(self.world)
        # A ray with o[a] == k and d[a] == 0 runs IN the plane of every rectangle at k on axis a, however far away, and hits it
        # with t = 0 / 0 = NaN, which no comparison rejects; which primitive it ends on then depends on the order of the tests,
        # and no culling structure reproduces the list's ("What the ray tests also showed" and "Textures on
        # adversarial inputs").  Probe rays stand off every plane but the one they are about.
        self.conditions.append(("no probe ray runs in the plane of a rectangle", not any(
            q.d[a] == 0.0 and q.o[a] == k for q in self.probes for a, k in self.planes)))
        return self

    def rays(self, only_f32=False):
        ps = [q for q in self.probes if q.f32 or not only_f32]
        o = np.ascontiguousarray([q.o for q in ps], dtype=np.float64)
        d = np.ascontiguousarray([q.d for q in ps], dtype=np.float64)
        t = np.ascontiguousarray([q.time for q in ps], dtype=np.float64)
        return ps, o, d, t

    def patch(self, kind, a0, a1, b0, b1, k, tex):
        mat = self.b.diffuse_light(tex) if self.max_depth == 1 else self.b.lambertian(tex)
        h = getattr(self.b, kind + "_rect")(a0, a1, b0, b1, k, mat)
        self.planes.append(({"xy": 2, "xz": 1, "yz": 0}[kind], k))
        self.objects.append(h)
        return h

    def aim(self, kind, a, b, k, **kw):
        """A ray along the normal axis of a `kind` rectangle at plane k onto in-plane coordinates (a, b), from distance 1."""
        ia, ib, ik = {"xy": (0, 1, 2), "xz": (0, 2, 1), "yz": (1, 2, 0)}[kind]
        p = [0.0, 0.0, 0.0]
        p[ia], p[ib], p[ik] = float(a), float(b), float(k)
        o = list(p)
        o[ik] = float(k) + 1.0
        assert o[ik] - 1.0 == k, "the plane must be reached at t = 1 exactly"
        d = [0.0, 0.0, 0.0]
        d[ik] = -1.0
        self.probes.append(Probe(o, d, p=p, **kw))
        return self.probes[-1]


def _neighbours(x):
    return [float(np.nextafter(x, -np.inf)), float(x), float(np.nextafter(x, np.inf))]


def _checker_depth(rtsr, as_bvh=False, depths=(1, 2, MAX_CHAIN), extra=None):
    """Chains of 1, 2 and 16 checkers over a solid colour and over an image, in three shapes: `both` (t = checker(t, t): both
    children on the chain), `odd` (t = checker(own colour, t)) and `even` (t = checker(t, own colour)): at a point of odd
    parity the odd chain is followed to its leaf, the even chain left at its first level, and the other way round.  And the
    mixed tree checker(even = noise, odd = image).  as_bvh: the solid-leaf chains under Lambertian spheres in one BVH, under a
    sky: k_trace_lds's form of the case (frames only)."""
    c = Case("checker_depth", rtsr, ("closed", "o1", "host"), background=(0.6, 0.7, 0.9) if as_bvh else BLACK, max_depth=4 if as_bvh else 1)
    b = c.b
    texels = make_texels(3, 2, 100.0)
    image = None if as_bvh else b.image_from_texels(texels)  # (an image record in the table, worn or not, takes the world from k_trace_lds)
    n = 0
    level_colour = lambda n, k: (0.05 + 0.01 * n, 0.02 * k, 0.9 - 0.01 * n)
    chains = []
    for leaf_kind in ("solid",) if as_bvh else ("solid", "image"):
        for shape in ("both", "odd", "even"):
            for depth in depths:
                leaf_rgb = (0.9 - 0.02 * n, 0.3 + 0.02 * n, 0.1)
                t = b.solid_color(leaf_rgb) if leaf_kind == "solid" else image
                firsts = []
                for k in range(depth):
                    own = b.solid_color(level_colour(n, k))
                    firsts.append(level_colour(n, k))
                    t = b.checker(t, t) if shape == "both" else (b.checker(own, t) if shape == "odd" else b.checker(t, own))
                chains.append((n, leaf_kind, shape, depth, t, leaf_rgb, firsts[-1]))
                n += 1
    if as_bvh:
        mats = [b.lambertian(t) for _, _, _, _, t, _, _ in chains]
        for n in range(45):  # every chain on five spheres of a 9 x 5 field
            c.objects.append(b.sphere((1.1 * (n % 9) - 4.4, 0.5, 1.1 * (n // 9) - 2.2), 0.5, mats[n % len(mats)]))
        c.objects.append(b.sphere((0.0, -300.0, 0.0), 300.0, b.lambertian(chains[-1][4])))
        c.objects.append(b.sphere((0.0, 1.6, 0.0), 0.4, b.metal((0.8, 0.8, 0.7), 0.1)))
        c.objects.append(b.sphere((1.1, 1.6, 0.0), 0.4, b.dielectric(1.5)))
        return c.finish(rtsr, (6.0, 5.0, 8.0), (0.0, 0.5, 0.0), 40.0, vup=(0.0, 1.0, 0.0), bvh=True)
    # patches of 1 x 1 at y = 0.25, two units apart; the probe points of one patch: local (0.3, 0.3) and (0.3, 0.6) + more
    local = [(0.3, 0.3), (0.3, 0.6), (0.7, 0.1), (0.95, 0.9), (0.5, 17.3), (0.1, 30.2)]
    parities = set()
    for n, leaf_kind, shape, depth, t, leaf_rgb, first in chains:
        x0 = 2.0 * n
        c.patch("xz", x0, x0 + 1.0, 0.0, 32.0, 0.25, t)  # (long in z: a 32-pixel frame from above sees every patch)
        for a, z in local:
            p = (x0 + a, 0.25, z)
            odd = checker_is_odd(p)
            parities.add((n, odd))
            u, v = rect_uv(p[0], x0, x0 + 1.0), rect_uv(z, 0.0, 32.0)
            at_leaf = shape == "both" or (shape == "odd") == odd
            leaf = np.array(leaf_rgb) if leaf_kind == "solid" else image_value(texels, u, v)
            c.aim("xz", p[0], z, 0.25, tex=t, u=u if leaf_kind == "image" else 0.0, v=v if leaf_kind == "image" else 0.0,
                  expected=leaf if at_leaf else np.array(first), tag="%s/%s/%d" % (leaf_kind, shape, depth))
    c.conditions.append(("every chain is probed at a point of either parity", all((n, o) in parities for n in range(len(chains)) for o in (False, True))))
    # the mixed tree: the odd child an image, the even child a noise texture
    noise = b.noise(4.0)
    mixed = b.checker(noise, image)
    x0 = 2.0 * len(chains)
    c.patch("xz", x0, x0 + 1.0, 0.0, 32.0, 0.25, mixed)
    seen = set()
    for a, z in local:
        p = (x0 + a, 0.25, z)
        odd = checker_is_odd(p)
        seen.add(odd)
        u, v = rect_uv(p[0], x0, x0 + 1.0), rect_uv(z, 0.0, 32.0)
        c.aim("xz", p[0], z, 0.25, tex=mixed, u=u, v=v, expected=image_value(texels, u, v) if odd else None, tag="mixed/" + ("image" if odd else "noise"))
    c.conditions.append(("the mixed tree is probed on its image and on its noise child", seen == {False, True}))
    c.extra = {"mixed": mixed, "n_chains": len(chains), "width": x0 + 1.0}
    _beside(c, extra)
    return c.finish(rtsr, (x0 / 2, 30.0, 16.0), (x0 / 2, 0.0, 16.0), 80.0)


def _checker_edges(rtsr, extra=None):
    """A two-colour checker on two large rectangles (an XZ one at y = 0.25, an XY one at z = 0.75; sin(2.5) and sin(7.5) are
    both positive), probed where one coordinate is the double nearest to k pi / 10 or one of its two neighbours, for k in
    (1, 3, 31, 1000, -7) on each axis; on rectangles at y = 0.0 and y = -0.0, where the zero factor makes every point even; and
    at |p| = 10^6, where 10 x is rounded before the sine."""
    c = Case("checker_edges", rtsr, ("closed", "o1", "host"))
    b = c.b
    even, odd = (0.9, 0.8, 0.1), (0.1, 0.2, 0.7)
    t = b.checker_from_colors(even, odd)
    big = 2.0 ** 21
    c.patch("xz", -big, big, -big, big, 0.25, t)
    c.patch("xy", -big, big, -big, big, 0.75, t)
    c.patch("xz", 3.0e6, 3.0e6 + 8.0, 0.0, 8.0, 0.0, t)
    c.patch("xz", 3.0e6, 3.0e6 + 8.0, 16.0, 24.0, -0.0, t)
    flips = 0
    for k in (1, 3, 31, 1000, -7):
        edge = float(Decimal(k) * PI60 / 10)
        for kind, plane, (first, second) in (("xz", 0.25, "xz"), ("xy", 0.75, "xy")):
            for which in (0, 1):
                got = []
                for x in _neighbours(edge):
                    ab = (x, 0.3) if which == 0 else (0.3, x)
                    pr = c.aim(kind, ab[0], ab[1], plane, tex=t, tag="edge k=%d %s" % (k, (first, second)[which]))
                    pr.expected = np.array(odd if checker_is_odd(pr.p) else even)
                    got.append(checker_is_odd(pr.p))
                flips += got[0] != got[2]
    c.conditions.append(("every edge has a neighbour of either parity", flips == 5 * 2 * 2))
    zero = 0
    for z0, y in ((0.0, 0.0), (16.0, -0.0)):
        for a, z in ((0.5, 0.5), (3.1, 4.3), (7.9, 0.2), (2.2, 6.6), (5.0, 5.0), (6.3, 1.7)):
            # (not in the float mode: its t_min grows with |origin| -- geometry.hpp: ray_t_min -- and is past t = 1 out here)
            pr = c.aim("xz", 3.0e6 + a, z0 + z, y, tex=t, expected=np.array(even), tag="zero plane %r" % y, f32=False)
            # without the zero factor the point would be odd for some of them: the rule is what makes them even
            zero += sin_sign_of_10x(pr.p[0]) * sin_sign_of_10x(pr.p[2]) < 0
    c.conditions.append(("some points of the zero planes would be odd but for the zero factor", zero >= 2))
    c.conditions.append(("-0.0 is a plane of its own", np.signbit(c.probes[-1].p[1]) and not np.signbit(c.probes[-7].p[1])))
    rounded = 0
    rng = np.random.RandomState(3)
    for _ in range(12):
        x, z = (1.0e6 + 100 * rng.rand()) * rng.choice([-1, 1]), (1.0e6 + 100 * rng.rand()) * rng.choice([-1, 1])
        pr = c.aim("xz", x, z, 0.25, tex=t, tag="far", f32=False)
        pr.expected = np.array(odd if checker_is_odd(pr.p) else even)
        rounded += Fraction(10.0 * x) != 10 * Fraction(x)
    c.conditions.append(("10 x is inexact at the far points", rounded >= 6))
    for _ in range(16):  # general points near the origin: what the float mode is held on
        kind, plane = (("xz", 0.25), ("xy", 0.75))[rng.randint(2)]
        pr = c.aim(kind, rng.uniform(-50.0, 50.0), rng.uniform(-50.0, 50.0), plane, tex=t, tag="general")
        pr.expected = np.array(odd if checker_is_odd(pr.p) else even)
    c.conditions.append(("both colours are seen far out", len({tuple(q.expected) for q in c.probes if q.tag == "far"}) == 2))
    for q in c.probes:
        q.f32 = q.f32 and not q.tag.startswith("edge")  # a float cannot hold these neighbours apart
    _beside(c, extra)
    return c.finish(rtsr, (0.5, 3.0, 0.5), (0.0, 0.25, 0.0), 50.0)


def _perlin_points(rtsr, extra=None):
    """Noise textures of scale 4, -3 and 0 on three large XY rectangles (z = 0.5, 2.25 and -1.75: the sine's argument is
    scale z + 10 turbulence(p)), probed at lattice points (xy at integers, and z = an integer on a fourth rectangle), over the
    period of 256, at negative non-integers, where the 7th octave leaves i32 but not the first (2^25 <= |x| < 2^31), at
    |x| >= 2^31 and at general points."""
    c = Case("perlin_points", rtsr, ("closed", "numpy", "o1", "host"))
    b = c.b
    big = 2.0 ** 52
    scales = (4.0, -3.0, 0.0)
    planes = (0.5, 2.25, -1.75)
    tex = [b.noise(s) for s in scales]
    for t, z in zip(tex, planes):
        c.patch("xy", -big, big, -big, big, z, t)
    c.patch("xy", -big, big, -big, big, 7.0, tex[0])  # a lattice plane: z an integer
    c.extra = {"scales": scales + (4.0,), "tex": tex + [tex[0]], "planes": planes + (7.0,)}
    rng = np.random.RandomState(8)

    def aim(which, x, y, tag, **kw):
        return c.aim("xy", x, y, c.extra["planes"][which], tex=c.extra["tex"][which], tag=tag, **kw)
    for x, y in ((0.0, 0.0), (3.0, -5.0), (-17.0, 255.0), (256.0, -256.0), (1000.0, 77.0)):
        aim(3, x, y, "lattice")  # every octave of an integer point is exactly 0: the value is 0.5 (1 + sin(4 x 7))
    for _ in range(6):
        x, y = [float(np.round(v * 2 ** 10) / 2 ** 10) for v in rng.uniform(-2 ** 19, 2 ** 19, 2)]
        for which in (0, 2):
            for dx, dy in ((0.0, 0.0), (256.0, 0.0), (0.0, 256.0), (-256.0, 512.0)):
                aim(which, x + dx, y + dy, "period", f32=False)  # groups of four: the point, then three of its images
    for _ in range(6):
        aim(rng.randint(3), -rng.uniform(0.01, 40.0), -rng.uniform(0.01, 40.0), "negative")
    for _ in range(6):
        s = rng.choice([-1.0, 1.0])
        aim(rng.randint(3), s * rng.uniform(2.0 ** 25, 2.0 ** 31), rng.uniform(-3.0, 3.0), "octave past i32", f32=False)
    for x in (2.0 ** 31, -2.0 ** 31, 3.0e9, -3.0e9, 4.0e7, 1.0e15, -1.0e15):
        aim(0, x, 0.375, "past i32" if abs(x) >= 2.0 ** 31 else "far", f32=False)
        aim(1, 0.375, x, "past i32" if abs(x) >= 2.0 ** 31 else "far", f32=False)
    for _ in range(24):
        aim(rng.randint(3), rng.uniform(-30.0, 30.0), rng.uniform(-30.0, 30.0), "general")
    c.conditions.append(("period points are multiples of 2^-10 below 2^20", all(
        abs(v) < 2.0 ** 20 and v * 2 ** 10 == np.floor(v * 2 ** 10) for q in c.probes if q.tag.startswith("period") for v in q.p)))
    _beside(c, extra)
    return c.finish(rtsr, (0.0, 0.0, 30.0), (0.0, 0.0, 0.0), 60.0, vup=(0.0, 1.0, 0.0))


# (multiples of 2^-4: x + 256 k is exact, so the same table WOULD give the same bits a period away)
LOCAL_POINTS = [(0.3125, 0.4375), (1.6875, 2.1875), (5.5, 0.875), (3.25, 3.75), (7.125, 6.3125), (2.625, 5.0625)]


def _perlin_tables(rtsr, n_tables=3, extra=None):
    """n_tables noise textures (each Noise::new draws its own table) on rectangles of 128 x 128 at x offsets 0, 256, 512 -- one
    period apart, so that the SAME table would give the same value at the same local point -- probed at the same local
    points.  A kernel that reads table 0 for all three fails."""
    c = Case("perlin_tables", rtsr, ("numpy", "o1", "host"))
    b = c.b
    tex = [b.noise(4.0) for _ in range(n_tables)]
    for k, t in enumerate(tex):
        c.patch("xy", 256.0 * k, 256.0 * k + 128.0, 0.0, 128.0, 0.5, t)
        for a, y in LOCAL_POINTS:
            c.aim("xy", 256.0 * k + a, y, 0.5, tex=t, tag="table %d" % k)
    c.extra = {"tex": tex, "n_tables": n_tables}
    c.conditions.append(("the rectangles are whole periods apart and probed at the same local points",
                         all(q.p[0] - 256.0 * (k // len(LOCAL_POINTS)) == LOCAL_POINTS[k % len(LOCAL_POINTS)][0] for k, q in enumerate(c.probes))))
    _beside(c, extra)
    return c.finish(rtsr, (320.0, 64.0, 560.0), (320.0, 64.0, 0.0), 60.0, vup=(0.0, 1.0, 0.0))


def _beside(c, extra, mat=None):
    """What stands beside the probed patches, far from every probe ray, to take the world to another walker or stack depth:
    a gravity sphere (P_ALL), a two-member instance tree (P_INST), or a BVH of 200 small spheres (max_stack grows, and with
    it the place in LDS where k_trace_world's table copies start)."""
    b = c.b
    if extra is None:
        return
    grey = mat if mat is not None else b.lambertian((0.5, 0.5, 0.5))  # (mat: a case that counts its materials lends one)
    if extra == "gravity":
        c.objects.append(b.gravity_sphere((-500.0, 40.0, -500.0), 0.0, 1.0, grey))
    elif extra == "instance":
        # (no face in a plane a probe ray runs in: such a ray meets the face at t = 0 / 0, and a NaN answers it -- hit.rs's
        # range tests let a NaN through, and the project keeps that)
        box = b.rect_prism((0.0, -0.413, 0.0), (1.0, 0.587, 1.0), grey)
        c.planes += [(0, -503.0), (0, -502.0), (1, -0.413), (1, 0.587), (2, -500.0), (2, -499.0)]  # the faces of the unrotated member
        c.objects.append(b.instance_bvh(b.hittable_list([b.translate((-500.0, 0.0, -500.0), b.rotate_y(15.0, box)),
                                                         b.translate((-503.0, 0.0, -500.0), box)])))
    elif extra == "bvh":
        rng = np.random.RandomState(4)
        balls = [b.sphere((-500.0 + 10 * rng.rand(), 10 * rng.rand(), -500.0 + 10 * rng.rand()), 0.05 + 0.1 * rng.rand(), grey) for _ in range(200)]
        c.objects.append(b.bvh_from_list(b.hittable_list(balls), 0.0, 1.0))
    else:
        assert extra is None, extra


IMAGE_SIZES = ((1, 1), (3, 2), (8, 4), (7, 5))  # (width, height)


def _image_lookup(rtsr, extra=None):
    """Four images in one scene (every one after the first has first_texel > 0) on: an XY rectangle x in [3, 11], y in [1, 3]
    (8 x 4 texels: u = k / 8 exactly at the borders), an XZ rectangle x in [13, 20], z in [-5, 0] (7 x 5: u = k / 7 is rounded), a YZ
    rectangle y in [1, 4], z in [5, 7] (3 x 2), an XY rectangle with the 1 x 1 image, a triangle (u = v = 1), a moving sphere
    (u = v = 0) and an XY rectangle under translate(rotate_y(90)), whose (u, v, p) are O1's.  a0 != b0 and the extents differ on
    every rectangle, so a swapped axis shows."""
    c = Case("image_lookup", rtsr, ("closed", "o1", "host"))
    b = c.b
    texels = [make_texels(w, h, 1.0 + 20.0 * m) for m, (w, h) in enumerate(IMAGE_SIZES)]
    images = [b.image_from_texels(t) for t in texels]
    rects = (("xy", 3.0, 11.0, 1.0, 3.0, -2.5, 2), ("xz", 13.0, 20.0, -5.0, 0.0, 0.5, 3), ("yz", 1.0, 4.0, 5.0, 7.0, 40.0, 1),
             ("xy", 30.0, 31.5, -7.0, -6.5, -2.5, 0))
    borders = set()
    for kind, a0, a1, b0, b1, k, m in rects:
        c.patch(kind, a0, a1, b0, b1, k, images[m])
        w, h = IMAGE_SIZES[m]
        aa = [a0, a1] + [x for i in range(1, w) for x in _neighbours(a0 + (a1 - a0) * i / w)] + [a0 + 0.37 * (a1 - a0)]
        bb = [b0, b1] + [x for i in range(1, h) for x in _neighbours(b0 + (b1 - b0) * i / h)] + [b0 + 0.61 * (b1 - b0)]
        # every a with three b and every b with three a: all columns and all rows, at every border, in a few hundred rays
        for a, bv in [(a, bv) for a in aa for bv in (bb[0], bb[-1], bb[1])] + [(a, bv) for bv in bb for a in (aa[0], aa[-1], aa[1])]:
            u, v = rect_uv(a, a0, a1), rect_uv(bv, b0, b1)
            # (the float mode is not held on a ray that runs IN the far face of the rectangle's box: core/cull32.hpp, make_ray32,
            # "an origin EXACTLY on a plane of a zero-component axis" -- the float judge shares that verdict, a closed form does not)
            c.aim(kind, a, bv, k, tex=images[m], u=u, v=v, expected=image_value(texels[m], u, v), tag="%s %dx%d" % (kind, w, h),
                  f32=a != a1 and bv != b1)
            j, i = texel_index(u, v, w, h)
            borders.update({(m, "row", j), (m, "column", i)})
    c.conditions.append(("every row and every column of every image is read", len(borders) == sum(w + h for w, h in IMAGE_SIZES)))
    c.conditions.append(("u = 1 and v = 1 exactly are probed", any(q.u == 1.0 for q in c.probes) and any(q.v == 1.0 for q in c.probes)))
    # (0 < a0 <= x makes x - a0 exact, so the double below a border is a u below it: nothing is rounded back onto the border)
    split = [i for i in range(1, 8) if rect_uv(3.0 + i, 3.0, 11.0) == i / 8 and
             [texel_index(rect_uv(x, 3.0, 11.0), 0.5, 8, 4)[1] for x in _neighbours(3.0 + i)][:2] == [i - 1, i]]
    c.conditions.append(("every border k / 8 is hit exactly, and from below by the neighbouring double", len(split) == 7))
    light = b.diffuse_light(images[3])
    c.objects.append(b.triangle((50.0, 0.0, 0.0), (52.0, 0.0, 0.0), (50.0, 0.0, 2.0), light))
    c.probes.append(Probe((50.5, 1.0, 0.5), (0.0, -1.0, 0.0), tex=images[3], u=1.0, v=1.0, p=(50.5, 0.0, 0.5),
                          expected=image_value(texels[3], 1.0, 1.0), tag="triangle"))
    c.objects.append(b.moving_sphere((60.0, 0.0, 0.0), (62.0, 0.0, 0.0), 0.0, 1.0, 0.5, light))
    c.probes.append(Probe((61.0, 2.0, 0.0), (0.0, -1.0, 0.0), tex=images[3], u=0.0, v=0.0, p=None,
                          expected=image_value(texels[3], 0.0, 0.0), tag="moving sphere", time=0.5))
    c.conditions.append(("the triangle's and the moving sphere's texels differ from each other and from the centre's",
                         len({tuple(image_value(texels[3], *uv)) for uv in ((1.0, 1.0), (0.0, 0.0), (0.5, 0.5))}) == 3))
    turned = b.translate((70.0, 0.0, 0.0), b.rotate_y(90.0, b.xy_rect(-3.0, 5.0, 1.0, 3.0, 0.0, b.diffuse_light(images[2]))))
    c.objects.append(turned)
    # rotate_y(90) takes the rectangle's x axis to -z: rays along -x from x = 72 onto (70, y, z)
    for y, z in ((1.5, 1.0), (2.9, -4.5), (1.01, 2.99), (2.0, -0.5)):
        c.probes.append(Probe((72.0, y, z), (-1.0, 0.0, 0.0), tex=images[2], p=None, tag="turned", handle=turned))
    c.extra = {"texels": texels, "images": images}
    _beside(c, extra)
    return c.finish(rtsr, (7.0, 2.0, 9.0), (7.0, 2.0, -2.5), 50.0, vup=(0.0, 1.0, 0.0))


def _sphere_uv(rtsr, orc, extra=None):
    """Image-textured spheres (8 x 4 texels), rays straight down on the north pole and up on the south pole, onto the seam
    phi = 0 / 2 pi from both sides, and at four general points.  A ray onto a pole often finds |outward.y| = 1 + 2^-52 and
    acos of that is NaN; clamp passes a NaN and `NaN as i32` is 0, so row 0 is read (the reference's behaviour).  A search over
    radius and centre picks one sphere whose north pole has v = NaN and one where it is finite (O1 decides)."""
    c = Case("sphere_uv", rtsr, ("closed", "o1", "host"))
    b = c.b
    texels = make_texels(8, 4, 50.0)
    image = b.image_from_texels(texels)
    light = b.diffuse_light(image)
    rng = np.random.RandomState(12)
    found = {}
    probe_b = rtsr.Builder(1)
    probe_light = probe_b.diffuse_light(probe_b.image_from_texels(texels))
    for _ in range(400):
        r, centre = float(rng.uniform(0.2, 3.0)), tuple(float(x) for x in rng.uniform(-5.0, 5.0, 3))
        s = probe_b.sphere(centre, r, probe_light)
        rec = orc.o1_hit(probe_b.graph_ptr(), s, (centre[0], centre[1] + r + 1.0, centre[2]), (0.0, -1.0, 0.0))
        found.setdefault(bool(np.isnan(rec["v"])), (r, centre))
        if len(found) == 2:
            break
    c.conditions.append(("the search found a NaN pole and a finite pole", len(found) == 2))
    for k, is_nan in enumerate((True, False)):
        r, (cx, cy, cz) = found[is_nan]
        cx += 20.0 * k  # (x does not enter the pole's arithmetic: outward.y and the NaN are unchanged)
        s = b.sphere((cx, cy, cz), r, light)
        c.objects.append(s)
        c.extra["pole %d" % k] = (s, (cx, cy + r + 1.0, cz))
        rays = [((cx, cy + r + 1.0, cz), (0.0, -1.0, 0.0), "north pole"), ((cx, cy - r - 1.0, cz), (0.0, 1.0, 0.0), "south pole"),
                ((cx - r - 1.0, cy, cz), (1.0, 0.0, 0.0), "seam")]
        for eps in (1e-9, -1e-9, 1e-3, -1e-3):
            dirn = np.array([-np.cos(eps), 0.0, np.sin(eps)])
            rays.append((tuple(np.array([cx, cy, cz]) + (r + 1.0) * dirn), tuple(-dirn), "seam side"))
        for dirn in ((0.3, 0.8, -0.5), (-0.6, -0.2, 0.7), (0.9, 0.1, 0.4), (-0.2, -0.9, -0.3)):
            dirn = np.array(dirn) / np.linalg.norm(dirn)
            rays.append((tuple(np.array([cx, cy, cz]) + (r + 1.0) * dirn), tuple(-dirn), "general"))
        for o, d, tag in rays:
            c.probes.append(Probe(o, d, tex=image, p=None, tag=tag, handle=s))
    c.extra["texels"] = texels
    r, centre = found[True]
    _beside(c, extra)
    return c.finish(rtsr, (centre[0] + 2.0 * r, centre[1] + 2.5 * r, centre[2] + 3.0 * r), centre, 40.0, vup=(0.0, 1.0, 0.0))


def _table_limits(rtsr, n_mat=64, n_tex=64, extra=None):
    """n_mat materials and n_tex textures, 64 or 65 of each -- either side of the limit of k_trace_world's LDS copy of both
    tables, the texture copy indexed behind the material copy: thin emissive rectangles in a row, each of its own solid
    colour, a checker whose children are the last two solid records (the checker itself is the last record), and what the
    count asks for: one more material over texture 0, two solid records that only the checker names."""
    own_children = n_tex == n_mat + 1
    more_mat = n_mat == n_tex + 1 or own_children
    n_plain = n_mat - 1 - (1 if more_mat else 0)
    c = Case("table_limits", rtsr, ("closed", "o1", "host"))
    b = c.b
    colour = lambda k: (0.01 * (k + 1), 1.0 - 0.01 * k, 0.5 + 0.005 * k)
    solids = [b.solid_color(colour(k)) for k in range(n_plain)]
    lights = [b.diffuse_light(t) for t in solids]
    if own_children:
        solids += [b.solid_color(colour(n_plain)), b.solid_color(colour(n_plain + 1))]
    checker = b.checker(solids[-2], solids[-1])
    lights.append(b.diffuse_light(checker))
    expect = [np.array(colour(k)) for k in range(n_plain)] + [None]
    if more_mat:
        lights.append(b.diffuse_light(solids[0]))
        expect.append(np.array(colour(0)))
    for k, m in enumerate(lights):
        c.objects.append(b.xz_rect(2.0 * k, 2.0 * k + 1.0, 0.0, 128.0, 0.25, m))  # (long in z: a 32-pixel frame sees every one)
    c.planes.append((1, 0.25))
    seen = set()
    for k, e in enumerate(expect):
        if e is not None:
            c.aim("xz", 2.0 * k + 0.5, 0.5, 0.25, tex=solids[k] if k < n_plain else solids[0], expected=e, tag="own colour")
            continue
        for a, z in ((0.3, 0.3), (0.3, 0.6), (0.7, 0.1), (0.95, 0.9)):
            p = (2.0 * k + a, 0.25, z)
            odd = checker_is_odd(p)
            seen.add(odd)
            c.aim("xz", p[0], z, 0.25, tex=checker, expected=np.array(colour(len(solids) - 1 if odd else len(solids) - 2)), tag="last checker")
    c.conditions.append(("the last checker shows both children", seen == {False, True}))
    c.extra = {"n_mat": n_mat, "n_tex": n_tex}
    _beside(c, extra, lights[0])
    return c.finish(rtsr, (65.0, 110.0, 64.0), (65.0, 0.0, 64.0), 70.0)


def _scatter(rtsr, extra=None):
    """The scatter path: checker(even = noise, odd = image) under a Lambertian on a single rectangle, background (1, 1, 1),
    max_depth = 2.  The scattered ray leaves the only object of the world, so the sum is attenuation x 1: the texture value."""
    c = Case("scatter", rtsr, ("closed", "o1", "host"), background=WHITE, max_depth=2)
    b = c.b
    texels = make_texels(7, 5, 30.0)
    image = b.image_from_texels(texels)
    mixed = b.checker(b.noise(-2.0), image)
    c.patch("yz", -1.0, 2.0, 4.0, 6.0, 0.5, mixed)
    seen = set()
    for y, z in ((-0.9, 4.1), (0.3, 4.4), (0.8, 5.1), (1.9, 5.9), (1.2, 4.05), (-0.35, 5.55), (0.05, 4.9), (1.55, 5.3)):
        p = (0.5, y, z)
        odd = checker_is_odd(p)
        seen.add(odd)
        u, v = rect_uv(y, -1.0, 2.0), rect_uv(z, 4.0, 6.0)
        c.aim("yz", y, z, 0.5, tex=mixed, u=u, v=v, expected=image_value(texels, u, v) if odd else None, tag="scatter/" + ("image" if odd else "noise"))
    c.conditions.append(("both children are reached", seen == {False, True}))
    # (a neighbour stands at x = -500, behind the rectangle's plane: a ray scattered off its +x face cannot reach it)
    _beside(c, extra)
    return c.finish(rtsr, (12.0, 0.5, 5.0), (0.5, 0.5, 5.0), 30.0, vup=(0.0, 1.0, 0.0))


def deep_checker(rtsr, depth, over_image=False):
    """(builder, a world of one emissive sphere under t = checker(t, t) applied `depth` times, the texture): depth 17 is the
    scene the flattener refuses."""
    b = rtsr.Builder(2)
    t = b.image_from_texels(make_texels(2, 2, 7.0)) if over_image else b.solid_color((0.9, 0.1, 0.1))
    for _ in range(depth):
        t = b.checker(t, t)
    return b, b.hittable_list([b.sphere((0.0, 0.0, 0.0), 1.0, b.diffuse_light(t))]), t


CASES = ("checker_depth", "checker_edges", "perlin_points", "perlin_tables", "image_lookup", "sphere_uv", "table_limits", "scatter")
_built = {}


def build(rtsr, orc, name, **variant):
    """The named case, built once per variant."""
    key = (name,) + tuple(sorted(variant.items()))
    if key not in _built:
        fn = globals()["_" + name]
        _built[key] = fn(rtsr, orc, **variant) if name == "sphere_uv" else fn(rtsr, **variant)
    return _built[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host_values(chk, case, f32=False):
    """The host judge's per-probe sums (n, 3) of the case's rays (only those the float mode may be held on, with f32)."""
    import trace_rays_cases as tc
    ps, o, d, t = case.rays(only_f32=f32)
    S, _ = tc.host_trace(chk, case.flat, o, d, t, spp=1, max_depth=case.max_depth, background=case.background, seed=1, f32=f32)
    return ps, S
