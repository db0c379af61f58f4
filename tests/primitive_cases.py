"""The judge, the scenes and the rays of tests/test_primitive_cases.py and tests/test_gpu_primitive_cases.py (a helper module, not
a test file): everything here runs on the CPU and shares no code with csrc/ or oracle/.

The judge restates the closest-hit rule of the reference (hit.rs: Sphere, XyRect / XzRect / YzRect, Triangle, RectPrism,
Translate, RotateY, HittableList) once, over a number kind:

  Exact    fractions.Fraction.  -0.0, +-inf and NaN are kept as Python floats and combined by IEEE rules, so a division by a
           signed zero, 0 / 0 of a zero radius and the NaN of a zero direction come out as the floating rule gives them.  A square
           root must be the root of a perfect square (the cases are chosen so).  Every finite intermediate is recorded: a lattice
           case proves its premise -- floating arithmetic is exact arithmetic on it -- by round-tripping each through float64 and
           float32 (lattice_premise).  The sign of a COMPUTED zero is not modelled (a Fraction has none); records are compared
           by value with NaN equal to NaN.
  Bounded  numpy.longdouble with a first-order error bound beside every value, in units of the unit roundoff u of the judged
           build (2^-53, 2^-24): an operation adds u |result| to what its operands carry (a + b: ea + eb; a b: |a| eb + |b| ea;
           a / b: ea / |b| + |a| eb / b^2; sqrt a: ea / (2 sqrt a)), the total is doubled for the second-order terms.  A comparison
           whose margin is below 4 x the doubled bound of its two sides marks the ray undecided; such a ray is judged on nothing.

Quirks of the reference that are part of the rule: a Translate and a RotateY face the record of their child AGAIN, and that
record's normal already points against the ray, so under either wrapper front_face reads true for a hit from behind as well
(false only where the dot is exactly 0 or, under a RotateY, where the mixed frames below disagree).  RotateY faces the normal against the ray it handed to its child AFTER
rotating the normal back (hit.rs:916-921), so front_face under a RotateY is not the geometric one; a Translate re-faces against
its moved ray (same direction: it only flips when the dot is exactly 0, hit.rs:810); every range test is inclusive at both ends
(`t < t_min || t > t_max` rejects), so a later object of a list wins a tie.

The f32 build raises a sphere's t_min by G = 2^-22 (|oc|^2 + r^2) / |half_b| (core/geometry.hpp: sphere_root).  The judge of the
f32 build adds G, evaluated in its own number kind, and a root within G / 2 of that edge is undecided.
Its culling ray gives up one class of rays (a direction component of exactly 0 with the origin on a box plane): the judge restates
that interval test (f32_culling_ray_rules_out) and such a lattice ray has two stated records, with and without the culled primitives.
"""
import math
import operator
from fractions import Fraction as Fr

import numpy as np

LD = np.longdouble
U = {"f64": LD(2.0) ** -53, "f32": LD(2.0) ** -24}
MODES = ("f64", "f32")
INF = float("inf")


def narrow(x, mode):
    """The value the build of `mode` works on: a double as given, or rounded to float."""
    return float(np.float32(x)) if mode == "f32" else float(x)


def next_up(x, mode):
    return float(np.nextafter(np.float32(x), np.float32(np.inf))) if mode == "f32" else float(np.nextafter(x, np.inf))


def next_down(x, mode):
    return float(np.nextafter(np.float32(x), np.float32(-np.inf))) if mode == "f32" else float(np.nextafter(x, -np.inf))


def threshold(mode):
    """The constant 0.0001 of Triangle::hit as the build of `mode` holds it."""
    return narrow(0.0001, mode)


# ---- number kinds --------------------------------------------------------------------------------------------------------
_QOPS = {"add": operator.add, "sub": operator.sub, "mul": operator.mul, "div": operator.truediv}
_FOPS = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide}


def _exact(x):
    if isinstance(x, Fr):
        return x
    if isinstance(x, int):
        return Fr(x)
    x = float(x)
    if not math.isfinite(x) or (x == 0.0 and math.copysign(1.0, x) < 0.0):
        return x
    return Fr(x)


def _xop(a, b, op):
    if isinstance(a, Fr) and isinstance(b, Fr) and not (op == "div" and b == 0):
        return _QOPS[op](a, b)
    with np.errstate(all="ignore"):
        r = float(_FOPS[op](np.float64(float(a)), np.float64(float(b))))
    if r != 0.0 and math.isfinite(r):  # a finite value met -0.0: the value is that of the rational operation
        return _QOPS[op](Fr(a), Fr(b))
    return Fr(0) if (r == 0.0 and math.copysign(1.0, r) > 0.0) else r


class XNum:
    __slots__ = ("k", "q")

    def __init__(self, k, q):
        self.k, self.q = k, q

    def _o(self, o):
        return o.q if isinstance(o, XNum) else _exact(o)

    def __add__(self, o): return self.k._res(_xop(self.q, self._o(o), "add"))
    def __radd__(self, o): return self.k._res(_xop(self._o(o), self.q, "add"))
    def __sub__(self, o): return self.k._res(_xop(self.q, self._o(o), "sub"))
    def __rsub__(self, o): return self.k._res(_xop(self._o(o), self.q, "sub"))
    def __mul__(self, o): return self.k._res(_xop(self.q, self._o(o), "mul"))
    def __rmul__(self, o): return self.k._res(_xop(self._o(o), self.q, "mul"))
    def __truediv__(self, o): return self.k._res(_xop(self.q, self._o(o), "div"))
    def __neg__(self): return XNum(self.k, -self.q)

    def value(self):
        return float(self.q)


class Exact:
    """The exact judge's context for one ray."""

    def __init__(self, mode):
        self.mode, self.f32 = mode, mode == "f32"
        self.seen, self.record, self.undecided = [], True, False

    def num(self, x):
        return x if isinstance(x, XNum) else XNum(self, _exact(x))

    stored = num

    def _res(self, r):
        if self.record and isinstance(r, Fr):
            self.seen.append(r)
        return XNum(self, r)

    def lt(self, a, b, slack=None):
        a, b = self.num(a).q, self.num(b).q
        if slack is not None and slack.q == slack.q:  # the f32 guard: within half of it of the edge, nothing is claimed
            with np.errstate(all="ignore"):
                gap = abs(np.float64(float(a)) - np.float64(float(b)))
            if gap < float(slack.q):
                self.undecided = True
        return a < b

    def abs(self, a):
        return XNum(self, abs(a.q))

    def sqrt(self, a):
        q = a.q
        if not isinstance(q, Fr):
            return XNum(self, math.sqrt(q) if q >= 0.0 else float("nan"))
        n, d = math.isqrt(q.numerator), math.isqrt(q.denominator)
        assert n * n == q.numerator and d * d == q.denominator, "a lattice case with an inexact square root: %r" % (q,)
        return self._res(Fr(n, d))


class BNum:
    __slots__ = ("k", "v", "e")

    def __init__(self, k, v, e):
        self.k, self.v, self.e = k, v, e

    def _o(self, o):
        return o if isinstance(o, BNum) else BNum(self.k, LD(o), 0.0)

    def __add__(self, o):
        o = self._o(o)
        v = self.v + o.v
        return BNum(self.k, v, self.e + o.e + abs(float(v)))

    __radd__ = __add__

    def __sub__(self, o):
        o = self._o(o)
        v = self.v - o.v
        return BNum(self.k, v, self.e + o.e + abs(float(v)))

    def __rsub__(self, o):
        return self._o(o) - self

    def __mul__(self, o):
        o = self._o(o)
        v = self.v * o.v
        return BNum(self.k, v, abs(float(self.v)) * o.e + abs(float(o.v)) * self.e + abs(float(v)))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._o(o)
        v = self.v / o.v
        b = abs(float(o.v))
        return BNum(self.k, v, self.e / b + abs(float(self.v)) * o.e / (b * b) + abs(float(v)))

    def __neg__(self):
        return BNum(self.k, -self.v, self.e)

    def value(self):
        return self.v

    def bound(self):
        """The doubled first-order bound, as a longdouble."""
        return 2 * self.k.u * LD(self.e)


class Bounded:
    """The bounded judge's context for one ray."""

    def __init__(self, mode):
        self.mode, self.f32, self.u = mode, mode == "f32", U[mode]
        self.undecided = False
        self.record = True

    def num(self, x):
        return x if isinstance(x, BNum) else BNum(self, LD(x), 0.0)

    def inp(self, x, e):
        """An input known to within e units of u (a frame's f32 primary ray, computed on the device)."""
        return BNum(self, LD(x), float(e))

    def stored(self, x):
        """A double the scene stores (a sine, a cosine): exact for the f64 build, one rounding away for the f32 build."""
        return BNum(self, LD(x), abs(float(x)) if self.f32 else 0.0)

    def lt(self, a, b, slack=None):
        a, b = self.num(a), self.num(b)
        need = 4 * (a.bound() + b.bound())
        if slack is not None:
            need = need + abs(slack.v) + 4 * slack.bound()
        with np.errstate(all="ignore"):
            if not (abs(a.v - b.v) >= need):
                self.undecided = True
        return bool(a.v < b.v)

    def abs(self, a):
        return BNum(self, abs(a.v), a.e)

    def sqrt(self, a):
        v = np.sqrt(a.v)
        fv = float(v)
        return BNum(self, v, (a.e / (2.0 * fv) if fv > 0.0 else (INF if a.e > 0.0 else 0.0)) + fv)


# ---- the rule -----------------------------------------------------------------------------------------------------------
def _dot(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
def _sub(a, b): return (a[0] - b[0], a[1] - b[1], a[2] - b[2])
def _add(a, b): return (a[0] + b[0], a[1] + b[1], a[2] + b[2])
def _neg(a): return (-a[0], -a[1], -a[2])
def _at(o, d, t): return (o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2])
def _cross(a, b): return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
def _v3(K, p): return tuple(K.num(x) for x in p)


def _face(K, d, outward):
    """HitRecord::create_normal_face: front when dot < 0 (a dot of exactly 0 reads as back)."""
    ff = K.lt(_dot(d, outward), 0)
    return (outward if ff else _neg(outward)), ff


def _sphere(K, node, o, d, t_min, t_max):
    c, r = _v3(K, node.a["c"]), K.num(node.a["r"])
    oc = _sub(o, c)
    a, half_b, cc = _dot(d, d), _dot(oc, d), _dot(oc, oc) - r * r
    disc = half_b * half_b - a * cc
    if K.lt(disc, 0):
        return None
    slack = None
    if K.f32:  # the documented guard of the fast mode, not a rule of the reference: kept out of the lattice premise
        K.record = False
        slack = (_dot(oc, oc) + r * r) / K.abs(half_b) * K.num(2.0 ** -23)  # half the guard
        t_min = K.num(t_min) + (slack + slack)
        K.record = True
    sq = K.sqrt(disc)
    root = (-half_b - sq) / a
    if K.lt(root, t_min, slack) or K.lt(t_max, root):
        root = (-half_b + sq) / a
        if K.lt(root, t_min, slack) or K.lt(t_max, root):
            return None
    p = _at(o, d, root)
    outward = tuple(x / r for x in _sub(p, c))
    n, ff = _face(K, d, outward)
    return {"t": root, "p": p, "n": n, "ff": ff, "id": node.id}


_RECT_AXES = {"xy": (2, 0, 1), "xz": (1, 0, 2), "yz": (0, 1, 2)}


def _rect(K, axis, a0, a1, b0, b1, k, ident, o, d, t_min, t_max):
    kk, ia, ib = _RECT_AXES[axis]
    t = (K.num(k) - o[kk]) / d[kk]
    if K.lt(t, t_min) or K.lt(t_max, t):
        return None
    x, y = o[ia] + t * d[ia], o[ib] + t * d[ib]
    if K.lt(x, a0) or K.lt(a1, x) or K.lt(y, b0) or K.lt(b1, y):
        return None
    n, ff = _face(K, d, _v3(K, [1.0 if i == kk else 0.0 for i in range(3)]))
    return {"t": t, "p": _at(o, d, t), "n": n, "ff": ff, "id": ident}


def _triangle(K, node, o, d, t_min, t_max):
    v0, v1, v2 = (_v3(K, node.a[v]) for v in ("v0", "v1", "v2"))
    # Triangle::new: (v1 - v0) x (v2 - v0) divided by its length, part of the rule's operation count (the f32 scene holds the f64
    # normal rounded once, which the same count covers)
    c = _cross(_sub(v1, v0), _sub(v2, v0))
    length = K.sqrt(_dot(c, c))
    n = tuple(x / length for x in c)
    n_dot_d = _dot(n, d)
    if K.lt(K.abs(n_dot_d), threshold(K.mode)):
        return None
    dd = -_dot(n, v0)
    t = -(_dot(n, o) + dd) / n_dot_d
    if K.lt(t, t_min) or K.lt(t_max, t):
        return None
    p = _at(o, d, t)
    for va, vb in ((v0, v1), (v1, v2), (v2, v0)):
        if K.lt(_dot(n, _cross(_sub(vb, va), _sub(p, va))), 0):
            return None
    nn, ff = _face(K, d, n)
    return {"t": t, "p": p, "n": nn, "ff": ff, "id": node.id}


def prism_faces(p0, p1):
    """RectPrism::new: front, back, top, bottom, right, left."""
    (x0, y0, z0), (x1, y1, z1) = p0, p1
    return [("xy", x0, x1, y0, y1, z1), ("xy", x0, x1, y0, y1, z0), ("xz", x0, x1, z0, z1, y1), ("xz", x0, x1, z0, z1, y0),
            ("yz", y0, y1, z0, z1, x1), ("yz", y0, y1, z0, z1, x0)]


def hit(K, node, o, d, t_min, t_max):
    """Hittable::hit of `node` for the ray (o, d) over [t_min, t_max], all of the context's numbers -> a record or None."""
    kind = node.kind
    if getattr(K, "cull", False) and kind in ("sphere", "rect", "tri") and f32_culling_ray_rules_out(node, o, d, t_min, t_max):
        return None
    if kind == "sphere":
        return _sphere(K, node, o, d, t_min, t_max)
    if kind == "rect":
        return _rect(K, *node.a["rect"], node.id, o, d, t_min, t_max)
    if kind == "tri":
        return _triangle(K, node, o, d, t_min, t_max)
    if kind == "prism" or kind in ("list", "bvh", "inst"):  # HittableList::hit: in order, closest_so_far shrinks, ties go to the later
        best, closest = None, t_max
        if kind == "prism":
            for f in prism_faces(node.a["p0"], node.a["p1"]):
                rec = _rect(K, *f, node.id, o, d, t_min, closest)
                if rec is not None:
                    best, closest = rec, rec["t"]
            return best
        for i, child in enumerate(node.children):
            rec = hit(K, child, o, d, t_min, closest)
            if rec is not None:
                best, closest = rec, rec["t"]
                best["slot"] = i
        return best
    if kind == "translate":  # hit.rs:801-823
        off = _v3(K, node.a["off"])
        moved = _sub(o, off)
        rec = hit(K, node.children[0], moved, d, t_min, t_max)
        if rec is None:
            return None
        rec["n"], rec["ff"] = _face(K, d, rec["n"])
        rec["p"] = _add(rec["p"], off)
        return rec
    assert kind == "rotate_y"  # hit.rs:891-931
    s, c = K.stored(node.a["sin"]), K.stored(node.a["cos"])
    ro = (c * o[0] - s * o[2], o[1], s * o[0] + c * o[2])
    rd = (c * d[0] - s * d[2], d[1], s * d[0] + c * d[2])
    rec = hit(K, node.children[0], ro, rd, t_min, t_max)
    if rec is None:
        return None
    p, n = rec["p"], rec["n"]
    rec["p"] = (c * p[0] + s * p[2], p[1], -s * p[0] + c * p[2])
    n = (c * n[0] + s * n[2], n[1], -s * n[0] + c * n[2])
    rec["n"], rec["ff"] = _face(K, rd, n)  # the quirk: the rotated ray against the normal rotated back
    return rec


# ---- scene descriptions --------------------------------------------------------------------------------------------------
class Node:
    def __init__(self, kind, children=(), **a):
        self.kind, self.children, self.a, self.id = kind, list(children), a, -1


def sphere(c, r): return Node("sphere", c=tuple(c), r=r)
def rect(axis, a0, a1, b0, b1, k): return Node("rect", rect=(axis, a0, a1, b0, b1, k))
def tri(v0, v1, v2): return Node("tri", v0=tuple(v0), v1=tuple(v1), v2=tuple(v2))
def prism(p0, p1): return Node("prism", p0=tuple(p0), p1=tuple(p1))
def translate(off, child): return Node("translate", [child], off=tuple(off))
def rotate_y(deg, child): return Node("rotate_y", [child], deg=deg)
def lst(*children): return Node("list", children)
def bvh(*children): return Node("bvh", children)
def inst(*children): return Node("inst", children)


def chain_of(node):
    """(op names outermost first, op nodes, innermost object) of a world slot."""
    names, ops = [], []
    while node.kind in ("translate", "rotate_y"):
        names.append(node.kind)
        ops.append(node)
        node = node.children[0]
    return names, ops, node


def _number(node, counter):
    if node.kind in ("sphere", "rect", "tri", "prism"):
        node.id = counter[0]
        counter[0] += 1
    for c in node.children:
        _number(c, counter)


class World:
    """A description (a "list" node: the world) built through the package's Builder and flattened.  Every primitive gets a
    Lambertian of its own whose red channel spells its id, so a material index reads back as a primitive.  After the build the
    RotateY nodes of the world's slots hold the sine and cosine the flat scene stores."""

    def __init__(self, rtsr, desc, max_leaf=0, emit=None):
        assert desc.kind == "list"
        self.desc, self.emit = desc, emit
        counter = [0]
        _number(desc, counter)
        self.n_prims = counter[0]
        assert self.n_prims < 250
        self.b = rtsr.Builder(1)
        self.handle = self._build(desc)
        self.flat = self.b.flatten(self.handle, max_leaf=max_leaf)
        n_mat = self.flat.info()["n_materials"] if emit is None else 0
        self.prim_of_material = np.array([int(round(self.flat.material(m)["albedo"][0] * 256.0)) - 1 for m in range(n_mat)], dtype=np.int64)
        self._read_chains()
        self.scenes = {}

    def _mat(self, node):
        if self.emit == "light":   # a DiffuseLight of a pure colour: a frame's pixel sums decode into hit counts (emit_colour)
            return self.b.diffuse_light(emit_colour(node.id))
        if self.emit == "matte":   # at max_depth 1 a hit is black and a miss the background
            return self.b.lambertian((0.5, 0.5, 0.5))
        return self.b.lambertian(((node.id + 1) / 256.0, 0.5, 0.5))

    def _build(self, n):
        b, a = self.b, n.a
        if n.kind == "sphere":
            return b.sphere(a["c"], a["r"], self._mat(n))
        if n.kind == "rect":
            axis, a0, a1, b0, b1, k = a["rect"]
            return {"xy": b.xy_rect, "xz": b.xz_rect, "yz": b.yz_rect}[axis](a0, a1, b0, b1, k, self._mat(n))
        if n.kind == "tri":
            return b.triangle(a["v0"], a["v1"], a["v2"], self._mat(n))
        if n.kind == "prism":
            return b.rect_prism(a["p0"], a["p1"], self._mat(n))
        if n.kind == "translate":
            return b.translate(a["off"], self._build(n.children[0]))
        if n.kind == "rotate_y":
            return b.rotate_y(a["deg"], self._build(n.children[0]))
        kids = b.hittable_list([self._build(c) for c in n.children])
        if n.kind == "bvh":
            return b.bvh_from_list(kids, 0.0, 1.0)
        return b.instance_bvh(kids) if n.kind == "inst" else kids

    def slots(self):
        """The description's nodes in the order of the world list's slots (an instance tree's members are slots)."""
        out = []
        for c in self.desc.children:
            out += c.children if c.kind == "inst" else [c]
        return out

    def _read_chains(self):
        """Flat.slot_chain names the ops of a slot; their parameters are read from the entry the slot points at (FlatEntry: four
        int32, f[2], then four ops of {int32 op, int32 pad, double v[3]}; a RotateY stores v[0] = sin, v[1] = cos)."""
        slots = self.slots()
        if not any(chain_of(s)[0] for s in slots):
            return
        assert self.flat.info()["n_top_level"] == len(slots), "a slot per child of the world list"
        entries = np.frombuffer(self.flat.array("entries"), dtype=np.uint8).reshape(-1, 160)
        top = np.frombuffer(self.flat.array("top_level"), dtype=np.int32)
        for i, s in enumerate(slots):
            names, ops, _ = chain_of(s)
            assert self.flat.slot_chain(i) == names, (i, names, self.flat.slot_chain(i))
            for k, op in enumerate(ops):
                v = entries[top[i], 32 + 32 * k + 8: 32 + 32 * k + 32].copy().view(np.float64)
                if op.kind == "rotate_y":
                    op.a["sin"], op.a["cos"] = float(v[0]), float(v[1])
                else:
                    assert tuple(v) == tuple(float(x) for x in op.a["off"])

    def scene(self, mode):
        if mode not in self.scenes:
            self.scenes[mode] = self.flat.upload(f32=(mode == "f32"))
        return self.scenes[mode]

    def rotations(self):
        return [op for s in self.slots() for op in chain_of(s)[1] if op.kind == "rotate_y"]


def stored_sin_cos_ulps(world):
    """For every RotateY of the world: how far the stored sine and cosine are from longdouble sin / cos of the angle in
    radians (the double the reference forms, f64::to_radians: degrees x (pi / 180) rounded once), in ulps of the stored value's
    binade (at least the ulp of 2^-1022)."""
    out = []
    for op in world.rotations():
        rad = LD(np.float64(op.a["deg"]) * np.float64(math.pi / 180.0))
        for got, want in ((op.a["sin"], np.sin(rad)), (op.a["cos"], np.cos(rad))):
            ulp = LD(np.spacing(np.float64(abs(float(want)))))
            out.append((op.a["deg"], float(abs(LD(got) - want) / ulp)))
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------
class Case:
    """A world description and rays: o, d (n, 3), t_max (n,), one t_min.  kind "lattice" (the exact judge) or "general" (the
    bounded judge).  `modes`: the builds the case is meant for (its numbers are exact inputs of those builds).  o1: whether the
    literal oracle is asked too (it is not for BVH and instance containers, whose box tests are not part of this rule).
    ids: whether the winning primitive is compared (not where the members of a BVH tie)."""

    def __init__(self, name, desc, rays, t_min=0.001, kind="lattice", modes=MODES, o1=True, ids=True, max_leaf=0, expect=None):
        self.name, self.desc, self.kind, self.modes, self.o1, self.ids, self.max_leaf = name, desc, kind, modes, o1, ids, max_leaf
        self.t_min = t_min
        _number(desc, [0])
        self.o = np.ascontiguousarray([r[0] for r in rays], dtype=np.float64).reshape(-1, 3)
        self.d = np.ascontiguousarray([r[1] for r in rays], dtype=np.float64).reshape(-1, 3)
        self.t_max = np.ascontiguousarray([r[2] if len(r) > 2 else INF for r in rays], dtype=np.float64)
        self.expect = expect  # optional: a list of "hit" / "miss" / None per ray, what the case was built to show
        self.world = None
        self.verdicts = {}
        assert 1 <= self.n <= 4096

    @property
    def n(self):
        return len(self.o)

    def build(self, rtsr):
        if self.world is None:
            self.world = World(rtsr, self.desc, self.max_leaf)
        return self.world

    def _values(self, K, rec):
        if self.kind == "lattice":
            return {"t": rec["t"].value(), "p": [x.value() for x in rec["p"]], "n": [x.value() for x in rec["n"]],
                    "ff": rec["ff"], "id": rec["id"], "slot": rec.get("slot", -1)}
        pair = lambda x: (K.num(x).v, K.num(x).bound())
        return {"t": pair(rec["t"]), "p": [pair(x) for x in rec["p"]], "n": [pair(x) for x in rec["n"]],
                "ff": rec["ff"], "id": rec["id"], "slot": rec.get("slot", -1)}

    def plain_top_level(self):
        """Every slot of the world is a bare sphere, rectangle or triangle: the slots world_hit culls by their own f32 box."""
        return all(c.kind in ("sphere", "rect", "tri") for c in self.desc.children)

    def judge(self, mode):
        """-> a list of verdicts, one per ray: {"undecided": bool, "rec": None or {t, p, n, ff, id} of floats (Exact) or of
        (value, bound) pairs in longdouble (Bounded), "seen": the Exact context's intermediates}.  The world must be built
        when a RotateY is in it (the stored sine and cosine)."""
        if mode in self.verdicts:
            return self.verdicts[mode]
        out = []
        for r in range(self.n):
            K = Exact(mode) if self.kind == "lattice" else Bounded(mode)
            o = _v3(K, [narrow(x, mode) for x in self.o[r]])
            d = _v3(K, [narrow(x, mode) for x in self.d[r]])
            rec = hit(K, self.desc, o, d, K.num(narrow(self.t_min, mode)), K.num(narrow(self.t_max[r], mode)))
            v = {"undecided": K.undecided, "rec": None, "seen": getattr(K, "seen", None)}
            if rec is not None:
                v["rec"] = self._values(K, rec)
            if mode == "f32" and self.kind == "lattice":
                # the same rule with the primitives the f32 culling ray rules out left out (f32_culling_ray_rules_out): where
                # that changes the record the ray belongs to the documented face-touch class, and "culled" is what a build
                # that culls it answers
                K2 = Exact(mode)
                K2.cull = True
                o2, d2 = _v3(K2, [narrow(x, mode) for x in self.o[r]]), _v3(K2, [narrow(x, mode) for x in self.d[r]])
                rec2 = hit(K2, self.desc, o2, d2, K2.num(narrow(self.t_min, mode)), K2.num(narrow(self.t_max[r], mode)))
                culled = None if rec2 is None else self._values(K2, rec2)
                if not same_record(culled, v["rec"]):
                    v["face_touch"], v["culled"] = True, culled
            out.append(v)
        self.verdicts[mode] = out
        return out


def _prim_boxes(node, off=(0.0, 0.0, 0.0)):
    """(lo, hi) of every primitive below `node` in world space, through Translates (lattice worlds have no RotateY).  A
    rectangle's own axis is padded as the reference pads it (k -+ 0.0001)."""
    a = node.a
    if node.kind == "sphere":
        box = [tuple(c - abs(a["r"]) for c in a["c"]), tuple(c + abs(a["r"]) for c in a["c"])]
    elif node.kind == "rect":
        axis, a0, a1, b0, b1, k_ = a["rect"]
        _ = (k_,)
        kk, ia, ib = _RECT_AXES[axis]
        lo, hi = [0.0] * 3, [0.0] * 3
        lo[kk], hi[kk], lo[ia], hi[ia], lo[ib], hi[ib] = _[0] - 0.0001, _[0] + 0.0001, min(a0, a1), max(a0, a1), min(b0, b1), max(b0, b1)
        box = [tuple(lo), tuple(hi)]
    elif node.kind == "tri":
        vs = (a["v0"], a["v1"], a["v2"])
        box = [tuple(min(v[i] for v in vs) for i in range(3)), tuple(max(v[i] for v in vs) for i in range(3))]
    elif node.kind == "prism":
        box = [a["p0"], a["p1"]]
    elif node.kind == "translate":
        return _prim_boxes(node.children[0], tuple(off[i] + a["off"][i] for i in range(3)))
    elif node.kind == "rotate_y":
        return []
    else:
        return [b for c in node.children for b in _prim_boxes(c, off)]
    return [(tuple(box[0][i] + off[i] for i in range(3)), tuple(box[1][i] + off[i] for i in range(3)))]


def f32_culling_ray_rules_out(node, o, d, t_min, t_max):
    """Whether the f32 build's culling ray (core/cull32.hpp: make_ray32 under RT_F32, cull32_may_hit) rules out the box of the
    primitive `node` for a ray with a direction component of exactly 0, restated on the Exact judge's numbers (lattice numbers:
    the float products are exact).  Such an axis gets the slope +2^60 (d = +0) or -2^60 (d = -0) instead of an infinite one, so
    its plane distances are (lo - o) s and (hi - o) s: an origin outside the slab sees both on one side (a true miss, unless
    the direction is all zero and the rule answers NaN), and an origin exactly ON a plane sees that plane at t = 0 instead of
    "inside for all t" -- when it is the far one, the interval ends at 0 and is empty as soon as t_min or another slab's entry
    lies above it.  That is the class the header documents as given up ("a ray that runs in a face of the box is culled when
    the plane is the far one and t_min > 0").  The box is ruled out when near - far exceeds the test's own slack,
    (|near| + |far|) 2^-21 + 2^-20 max |o / d| over the axes with a finite slope.  A ray without a zero component is not
    modelled (there the test is conservative and changes nothing): False."""
    (lo, hi), = _prim_boxes(node)
    fo, fd = [float(x.q) for x in o], [x.q for x in d]
    if not any(q == 0 for q in fd) or any(x != x for x in fo):
        return False
    nears, fars, err = [float(t_min.q)], [float(t_max.q)], 0.0
    for i in range(3):
        if fd[i] == 0:
            slope = -2.0 ** 60 if (isinstance(fd[i], float) and math.copysign(1.0, fd[i]) < 0.0) else 2.0 ** 60
        else:
            slope = 1.0 / float(fd[i])
            err = max(err, abs(fo[i] * slope))
        a, b = (lo[i] - fo[i]) * slope, (hi[i] - fo[i]) * slope
        nears.append(min(a, b))
        fars.append(max(a, b))
    tn, tf = max(x for x in nears if x == x), min(x for x in fars if x == x)  # fmaxf / fminf drop a NaN (the running closest t)
    return tn - tf > (abs(tn) + abs(tf)) * 2.0 ** -21 + err * 2.0 ** -20


def lattice_premise(case, mode):
    """Every finite intermediate of every ray of a lattice case round-trips through the float type of `mode` -> the number of
    intermediates checked.  AssertionError names the first that does not."""
    count = 0
    ftype = np.float32 if mode == "f32" else np.float64
    for r, v in enumerate(case.judge(mode)):
        for q in v["seen"]:
            with np.errstate(over="ignore"):
                back = ftype(q.numerator) / ftype(q.denominator) if abs(q.numerator) < 2 ** 1000 else ftype(float(q))
            assert math.isfinite(float(back)) and Fr(float(back)) == q, "%s (%s), ray %d: %r is not a %s" % (case.name, mode, r, q, ftype.__name__)
            count += 1
    return count


def same_record(a, b):
    """Two exact records (or None) are the same answer."""
    if a is None or b is None:
        return a is None and b is None
    flat = lambda r: [r["t"]] + list(r["p"]) + list(r["n"])
    return a["ff"] == b["ff"] and a["id"] == b["id"] and all(same_value(x, y) for x, y in zip(flat(a), flat(b)))


def check_touch_record(case, mode, r, verdict, got, allow_rule):
    """A ray of the f32 face-touch class: a build that culls answers verdict["culled"], one that does not the rule's record.
    -> "culled" or "rule", whichever `got` equals; the rule's record is only admissible where allow_rule says so."""
    try:
        check_record(case, mode, r, dict(verdict, rec=verdict["culled"], undecided=False), got)
        return "culled"
    except AssertionError:
        if not allow_rule:
            raise
    check_record(case, mode, r, dict(verdict, undecided=False), got)
    return "rule"


def same_value(a, b):
    """Equal as numbers, NaN equal to NaN (+0 equals -0: the exact judge has no signed computed zero)."""
    a, b = float(a), float(b)
    return a == b or (a != a and b != b)


def check_record(case, mode, r, verdict, got, want_id=True):
    """One ray's record from a build against its verdict -> the worst observed-to-bound ratio of the ray (0 for an exact match
    or a ray judged on nothing).  got: None (miss) or {"t", "p", "normal", "front_face", and optionally "id"}."""
    tag = "%s (%s), ray %d o=%r d=%r t_min=%r t_max=%r" % (case.name, mode, r, case.o[r].tolist(), case.d[r].tolist(), case.t_min, case.t_max[r])
    if verdict["undecided"]:
        return 0.0
    want = verdict["rec"]
    assert (got is None) == (want is None), "%s: the build says %s, the judge %s" % (tag, "miss" if got is None else "hit %r" % (got,), want)
    if want is None:
        return 0.0
    assert bool(got["front_face"]) == bool(want["ff"]), "%s: front_face %r, the judge %r" % (tag, got["front_face"], want["ff"])
    if want_id and case.ids and got.get("id") is not None:
        assert got["id"] == want["id"], "%s: primitive %r, the judge %r" % (tag, got["id"], want["id"])
    pairs = [(got["t"], want["t"], "t")] + [(got["p"][i], want["p"][i], "p[%d]" % i) for i in range(3)] + \
            [(got["normal"][i], want["n"][i], "normal[%d]" % i) for i in range(3)]
    worst = 0.0
    for g, w, what in pairs:
        if case.kind == "lattice":
            assert same_value(g, w), "%s: %s = %r, the judge %r" % (tag, what, g, w)
            continue
        value, bound = w
        err = abs(LD(g) - value)
        ratio = float(err / bound) if bound > 0 else (0.0 if err == 0 else INF)
        worst = max(worst, ratio)
        assert ratio <= 1.0, "%s: %s = %r, the judge %r +- %r (ratio %.3g)" % (tag, what, g, float(value), float(bound), ratio)
    return worst


def undecided_count(case, mode):
    return sum(1 for v in case.judge(mode) if v["undecided"])


UNDECIDED_CAP = 0.005  # of a case's rays, in f64 and in f32


# ---- lattice cases -------------------------------------------------------------------------------------------------------
C0 = (2.0, -1.0, 4.0)  # the lattice sphere: radius 5 around C0, so that 3-4-5 offsets are lattice points on it


def _from(c, *off):
    return tuple(c[i] + off[i] for i in range(3))


def _aimed(target, d, t0=2.0):
    """A ray that reaches `target` at t = t0 exactly (all numbers small dyadics)."""
    return (tuple(target[i] - t0 * d[i] for i in range(3)), tuple(d))


def sphere_lattice_cases(mode):
    S = lambda r=5.0: lst(sphere(C0, r))
    up, dn = (lambda x: next_up(x, mode)), (lambda x: next_down(x, mode))
    through = (_from(C0, 0, 0, -13), (0.0, 0.0, 1.0))  # roots 8 and 18
    axis_points = [(5, 0, 0), (-5, 0, 0), (0, 5, 0), (0, -5, 0), (0, 0, 5), (0, 0, -5)]
    oblique = [(-1.0, 2.0, 2.0), (2.0, -1.0, 2.0), (2.0, 2.0, -1.0), (1.0, 2.0, -2.0), (-3.0, 0.0, 4.0), (0.5, -1.0, 1.0)]
    out = [
        # discriminant exactly 0: a hit, with dot(d, outward) exactly 0 (front_face false, the normal negated)
        Case("sphere_tangent", S(), [(_from(C0, 5, 0, -8), (0.0, 0.0, 1.0)), (_from(C0, 5, -6, -8), (0.0, 3.0, 4.0)),
                                     (_from(C0, -8, 5, 0), (1.0, 0.0, 0.0)), (_from(C0, 0, -8, -5), (0.0, 2.0, 0.0))], expect=["hit"] * 4),
        # oblique lattice rays onto the six axis points: disc = dot(P - c, d)^2, root1 = t0 exactly
        Case("sphere_axis_points", S(), [_aimed(_from(C0, *P), d, t0) for P in axis_points for d in oblique for t0 in (2.0, 0.5)
                                         if sum(P[i] * d[i] for i in range(3)) < 0]),
        Case("sphere_window_tmin_eq_root1", S(), [through], t_min=8.0),
        Case("sphere_window_tmin_above_root1", S(), [through, through + (18.0,), through + (dn(18.0),)], t_min=up(8.0)),
        Case("sphere_window_tmax_eq_root2", S(), [through + (18.0,), through + (dn(18.0),), through + (up(18.0),)], t_min=9.0),
        Case("sphere_window_tmin_eq_tmax_root1", S(), [through + (8.0,)], t_min=8.0),
        Case("sphere_window_tmin_eq_tmax_root2", S(), [through + (18.0,)], t_min=18.0),
        Case("sphere_origin_at_centre", S(), [(C0, (0.0, 0.0, 1.0)), (C0, (0.0, -2.0, 0.0)), (C0, (0.5, 0.0, 0.0))]),
        Case("sphere_origin_on_surface_tmin_0", S(), [(_from(C0, 5, 0, 0), (-1.0, 0.0, 0.0)), (_from(C0, 5, 0, 0), (1.0, 0.0, 0.0)),
                                                      (_from(C0, 0, -5, 0), (0.0, 2.0, 0.0))], t_min=0.0),
        Case("sphere_origin_on_surface_tmin_0.001", S(), [(_from(C0, 5, 0, 0), (-1.0, 0.0, 0.0)), (_from(C0, 5, 0, 0), (1.0, 0.0, 0.0))], t_min=0.001),
        Case("sphere_negative_radius", S(-5.0), [through, (C0, (0.0, 0.0, 1.0)), (_from(C0, 5, 0, -8), (0.0, 0.0, 1.0))] +
             [_aimed(_from(C0, *P), d) for P in axis_points for d in oblique[:3] if sum(P[i] * d[i] for i in range(3)) < 0]),
        Case("sphere_zero_radius", S(0.0), [(_from(C0, 0, 0, -4), (0.0, 0.0, 1.0)), (_from(C0, 3, 0, 0), (-1.0, 0.0, 0.0)),
                                            (_from(C0, 0, 1, -4), (0.0, 0.0, 1.0))], expect=["hit", "hit", "miss"]),
    ]
    for k in (-20, 0, 20):
        s = 2.0 ** k
        out.append(Case("sphere_direction_scaled_2^%d" % k, S(), [(through[0], (0.0, 0.0, s)), (_from(C0, 5, 0, -8), (0.0, 0.0, s)),
                                                                 _aimed(_from(C0, 5, 0, 0), (-s, 2 * s, 2 * s), 2.0 / s)], t_min=0.0))
    # the zero direction: t = NaN for every sphere reached, so the last of a list answers
    out.append(Case("sphere_zero_direction", lst(sphere(C0, 5.0), sphere((20.0, 0.0, 0.0), 2.0), sphere((-9.0, 3.0, 1.0), 1.0)),
                    [((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), (C0, (0.0, 0.0, 0.0)), ((1.0, 2.0, 3.0), (0.0, 0.0, 0.0), 7.0)], expect=["hit"] * 3))
    return out


def _rect_point(axis, x, y, k):
    kk, ia, ib = _RECT_AXES[axis]
    p = [0.0, 0.0, 0.0]
    p[kk], p[ia], p[ib] = k, x, y
    return tuple(p)


def _rect_dir(axis, da, db, dk):
    return _rect_point(axis, da, db, dk)


def rect_lattice_cases(mode):
    out = []
    up, dn = (lambda x: next_up(x, mode)), (lambda x: next_down(x, mode))
    a0, a1, b0, b1, k = 0.0, 4.0, -2.0, 6.0, 3.0
    tiny = 2.0 ** -40
    for axis in ("xy", "xz", "yz"):
        R = lambda: lst(rect(axis, a0, a1, b0, b1, k))
        P, D = (lambda x, y, kk=k: _rect_point(axis, x, y, kk)), (lambda da, db, dk: _rect_dir(axis, da, db, dk))
        border = [(0.0, 1.0), (4.0, 1.0), (2.0, -2.0), (2.0, 6.0), (0.0, -2.0), (0.0, 6.0), (4.0, -2.0), (4.0, 6.0)]
        rays = []
        for x, y in border:
            rays += [(P(x, y, k + 4.0), D(0.0, 0.0, -1.0)), (P(x, y, k - 4.0), D(0.0, 0.0, 2.0)), _aimed(P(x, y), D(1.0, -2.0, -4.0)),
                     _aimed(P(x, y), D(-0.5, 1.0, 2.0), 4.0)]
        out.append(Case("rect_%s_edges_and_corners" % axis, R(), rays, expect=["hit"] * len(rays)))
        # 2^-40 inside and outside where the float type holds it (next to the edges at 0: exact in f32 too), one float in and out
        # of every edge otherwise; perpendicular rays, so the origin carries the offset exactly
        near = [((tiny, 1.0), "hit"), ((-tiny, 1.0), "miss"), ((up(4.0), 1.0), "miss"), ((dn(4.0), 1.0), "hit"),
                ((2.0, dn(-2.0)), "miss"), ((2.0, up(-2.0)), "hit"), ((2.0, up(6.0)), "miss"), ((2.0, dn(6.0)), "hit")]
        if mode == "f64":
            near += [((4.0 + tiny, 1.0), "miss"), ((4.0 - tiny, 1.0), "hit"), ((2.0, -2.0 - tiny), "miss"), ((2.0, -2.0 + tiny), "hit"),
                     ((2.0, 6.0 + tiny), "miss"), ((2.0, 6.0 - tiny), "hit")]
        out.append(Case("rect_%s_one_step_from_the_edges" % axis, R(), [(P(x, y, k + 4.0), D(0.0, 0.0, -1.0)) for (x, y), _ in near],
                        expect=[e for _, e in near]))
        ray = (P(1.0, 1.0, k + 4.0), D(0.0, 0.0, -2.0))  # t = 2
        out.append(Case("rect_%s_window_tmin" % axis, R(), [ray], t_min=2.0, expect=["hit"]))
        out.append(Case("rect_%s_window_tmin_above" % axis, R(), [ray], t_min=up(2.0), expect=["miss"]))
        out.append(Case("rect_%s_window_tmax" % axis, R(), [ray + (2.0,), ray + (dn(2.0),), ray + (up(2.0),)], t_min=0.0, expect=["hit", "miss", "hit"]))
        # parallel to the plane and off it: dk = +0 and -0, k - ok of both signs, finite and infinite t_max: t is an infinity
        par = [(P(1.0, 1.0, k + s), D(1.0, 2.0, z), tm) for s in (2.0, -2.0) for z in (0.0, -0.0) for tm in (INF, 100.0)]
        out.append(Case("rect_%s_parallel_off_plane" % axis, R(), par, expect=["miss"] * len(par)))
        inside = [(P(2.0, 1.0, k + 4.0), D(0.0, 0.0, -1.0)), _aimed(P(2.0, 1.0), D(1.0, -2.0, -4.0)), (P(2.0, 1.0, k - 4.0), D(0.0, 0.0, 1.0))]
        out.append(Case("rect_%s_reversed_extents" % axis, lst(rect(axis, a1, a0, b0, b1, k), rect(axis, a0, a1, b1, b0, k - 8.0)),
                        inside + [(P(2.0, 1.0, k + 4.0), D(0.0, 0.0, -1.0), 100.0)], expect=["miss"] * 4))
        out.append(Case("rect_%s_zero_width" % axis, lst(rect(axis, 2.0, 2.0, b0, b1, k)),
                        [inside[0], inside[1], (P(up(2.0), 1.0, k + 4.0), D(0.0, 0.0, -1.0)), (P(dn(2.0), 1.0, k + 4.0), D(0.0, 0.0, -1.0))],
                        expect=["hit", "hit", "miss", "miss"]))
    return out


PRISM = ((0.0, 0.0, 0.0), (4.0, 2.0, 8.0))


def prism_lattice_cases(mode):
    """Through edges and corners of the box exactly: two or three faces tie, the later of front, back, top, bottom, right, left
    answers -- the normal tells which."""
    rays = [_aimed((4.0, 2.0, 3.0), (-1.0, -1.0, 0.0)),     # top and right -> right (1, 0, 0)
            _aimed((1.0, 2.0, 8.0), (0.0, -1.0, -1.0)),     # front and top -> top (0, 1, 0)
            _aimed((4.0, 1.0, 8.0), (-2.0, 0.0, -2.0)),     # front and right -> right
            _aimed((0.0, 2.0, 3.0), (1.0, -1.0, 0.0)),      # top and left -> left
            _aimed((4.0, 2.0, 8.0), (-1.0, -1.0, -1.0)),    # a corner: front, top and right -> right
            _aimed((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),       # the opposite corner: back, bottom and left -> left
            _aimed((0.0, 2.0, 8.0), (0.5, -1.0, -2.0)),     # a corner: front, top, left -> left
            _aimed((1.0, 0.0, 0.0), (0.0, 1.0, 1.0))]       # back and bottom -> bottom (0, -1, 0)
    normals = [(1, 0, 0), (0, 1, 0), (1, 0, 0), (-1, 0, 0), (1, 0, 0), (-1, 0, 0), (-1, 0, 0), (0, -1, 0)]
    return [Case("prism_edges_and_corners", lst(prism(*PRISM)), rays, expect=[("normal", n) for n in normals])]


T0 = ((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 4.0, 0.0))
T1 = ((4.0, 4.0, 0.0), (0.0, 4.0, 0.0), (4.0, 0.0, 0.0))  # the mirror: shares the hypotenuse, same normal (0, 0, 1)


def triangle_lattice_cases(mode):
    out = []
    up, dn = (lambda x: next_up(x, mode)), (lambda x: next_down(x, mode))
    tiny = 2.0 ** -40
    one = lambda: lst(tri(*T0))
    down, obl = (0.0, 0.0, -1.0), (1.0, -2.0, -4.0)
    on = [(1.0, 1.0), (2.0, 0.0), (0.0, 2.0), (2.0, 2.0), (1.0, 3.0), (0.0, 0.0), (4.0, 0.0), (0.0, 4.0)]  # interior, edges, vertices
    rays = []
    for x, y in on:
        rays += [((x, y, 2.0), down), _aimed((x, y, 0.0), obl), _aimed((x, y, 0.0), (-0.5, 0.25, 1.0), 4.0)]  # the last from behind
    out.append(Case("triangle_interior_edges_vertices", one(), rays, expect=["hit"] * len(rays)))
    # 2^-40 off every edge in f64.  The f32 cases step 2^-18: the hypotenuse's edge function of such a point is 8 -+ 2^-16, which a
    # float still holds (2^-40 would round away there, and the case would no longer be exact arithmetic)
    tiny = 2.0 ** -40 if mode == "f64" else 2.0 ** -18
    near = [((2.0, -tiny), "miss"), ((2.0, tiny), "hit"), ((-tiny, 2.0), "miss"), ((tiny, 2.0), "hit"), ((2.0 + tiny, 2.0), "miss"),
            ((2.0 - tiny, 2.0), "hit"), ((2.0, 2.0 + tiny), "miss"), ((1.0, 3.0 - tiny), "hit"), ((-tiny, -tiny), "miss"),
            ((up(4.0), 0.0), "miss"), ((0.0, up(4.0)), "miss")]
    out.append(Case("triangle_one_step_from_the_edges", one(), [((x, y, 2.0), down) for (x, y), _ in near] + [((x, y, -2.0), (0.0, 0.0, 1.0)) for (x, y), _ in near],
                    expect=[e for _, e in near] * 2))
    ray = ((1.0, 1.0, 4.0), (0.0, 0.0, -2.0))
    out.append(Case("triangle_window_tmin", one(), [ray], t_min=2.0, expect=["hit"]))
    out.append(Case("triangle_window_tmin_above", one(), [ray], t_min=up(2.0), expect=["miss"]))
    out.append(Case("triangle_window_tmax", one(), [ray + (2.0,), ray + (dn(2.0),)], t_min=0.0, expect=["hit", "miss"]))
    # |n . d| exactly the build's 0.0001 (a hit at t = 4: o.z = 4 c, d.z = -c), one float below (a miss), and a perpendicular
    # direction of length 2^-14 (a miss: the threshold is on n . d, not on the angle).  The constant differs between the
    # builds, so each gets its own case
    c = threshold(mode)
    cf = float(np.nextafter(np.float32(c), np.float32(0))) if mode == "f32" else float(np.nextafter(c, 0.0))
    out.append(Case("triangle_parallel_threshold_%s" % mode, one(), [((1.0, 1.0, 4.0 * c), (0.0, 0.0, -c)), ((1.0, 1.0, 4.0 * c), (0.0, 0.0, -cf)),
                                                                    ((1.0, 1.0, -4.0 * c), (0.0, 0.0, c)), ((1.0, 1.0, 4.0 * c), (0.25, 0.0, -c)),
                                                                    ((1.0, 1.0, 2.0), (0.0, 0.0, -2.0 ** -14)), ((1.0, 1.0, 2.0), (0.0, 0.0, -2.0 ** -13))],
                    modes=(mode,), t_min=0.0, expect=["hit", "miss", "hit", "hit", "miss", "hit"]))
    # the shared edge: both triangles tie at one t, the later of the list answers
    shared = [(2.0, 2.0), (1.0, 3.0), (3.0, 1.0), (4.0, 0.0), (0.0, 4.0)]
    rays = [((x, y, 2.0), down) for x, y in shared] + [_aimed((x, y, 0.0), obl) for x, y in shared]
    out.append(Case("triangle_shared_edge_list", lst(tri(*T0), tri(*T1)), rays, expect=[("id", 1)] * len(rays)))
    out.append(Case("triangle_shared_edge_list_swapped", lst(tri(*T1), tri(*T0)), rays, expect=[("id", 1)] * len(rays)))
    both = rays + [((1.0, 1.0, 2.0), down), ((3.0, 3.0, 2.0), down), ((5.0, 5.0, 2.0), down)]
    out.append(Case("triangle_shared_edge_bvh", lst(bvh(tri(*T0), tri(*T1))), both, o1=False, ids=False))
    out.append(Case("triangle_shared_edge_bvh_leaf1", lst(bvh(tri(*T0), tri(*T1))), both, o1=False, ids=False, max_leaf=1))
    return out


def translate_lattice_cases(mode):
    """Dyadic offsets: t has the bits of the unwrapped primitive under the shifted ray, p is the child's plus the offset."""
    out = []
    off = (0.5, -2.0, 8.0)
    shift = lambda rays: [(_from(r[0], *off), r[1]) + tuple(r[2:]) for r in rays]
    s_rays = [(_from(C0, 0, 0, -13), (0.0, 0.0, 1.0)), (_from(C0, 5, 0, -8), (0.0, 0.0, 1.0)), (C0, (0.0, 2.0, 0.0))] + \
             [_aimed(_from(C0, 5, 0, 0), d) for d in ((-1.0, 2.0, 2.0), (-3.0, 0.0, 4.0))]
    out.append(Case("translate_sphere", lst(translate(off, sphere(C0, 5.0))), shift(s_rays)))
    r_rays = [_aimed((x, 3.0, y), (1.0, -4.0, -2.0)) for x, y in ((0.0, 1.0), (4.0, 6.0), (2.0, 1.0))] + [((2.0, -1.0, 1.0), (0.0, 1.0, 0.0))]
    out.append(Case("translate_rect", lst(translate(off, rect("xz", 0.0, 4.0, -2.0, 6.0, 3.0))), shift(r_rays)))
    t_rays = [_aimed((x, y, 0.0), (1.0, -2.0, -4.0)) for x, y in ((1.0, 1.0), (2.0, 2.0), (0.0, 0.0))] + [((1.0, 1.0, -2.0), (0.0, 0.0, 1.0))]
    out.append(Case("translate_triangle", lst(translate(off, tri(*T0))), shift(t_rays)))
    out.append(Case("translate_prism_twice", lst(translate((1.0, 0.0, 0.0), translate((-0.5, -2.0, 8.0), prism(*PRISM)))),
                    shift([_aimed((4.0, 2.0, 8.0), (-1.0, -1.0, -1.0)), _aimed((4.0, 2.0, 3.0), (-1.0, -1.0, 0.0)), _aimed((2.0, 2.0, 3.0), (0.5, -1.0, 0.25))])))
    return out


FAMILIES = {"sphere": sphere_lattice_cases, "rect": rect_lattice_cases, "prism": prism_lattice_cases,
            "triangle": triangle_lattice_cases, "translate": translate_lattice_cases}


def lattice_cases(mode):
    return sphere_lattice_cases(mode) + rect_lattice_cases(mode) + prism_lattice_cases(mode) + triangle_lattice_cases(mode) + translate_lattice_cases(mode)


# ---- general-position cases -----------------------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def aimed_rays(n, seed, centre, distance, aims, scale=1.0):
    """n rays from points at `distance` around `centre` towards targets drawn from `aims`: a list of (weight, lo, hi) boxes.
    Directions are not unit vectors (x scale); origins and directions are rounded to float, so both builds read the same ray."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    o = np.asarray(centre) + distance * v / np.linalg.norm(v, axis=1, keepdims=True)
    w = np.array([a[0] for a in aims], dtype=np.float64)
    which = rng.choice(len(aims), size=n, p=w / w.sum())
    lo, hi = np.array([aims[k][1] for k in which], dtype=np.float64), np.array([aims[k][2] for k in which], dtype=np.float64)
    target = lo + rng.uniform(size=(n, 3)) * (hi - lo)
    d = (target - o) * scale * rng.uniform(0.5, 2.0, size=(n, 1))
    o, d = _f32(o), _f32(d)
    return [(tuple(o[r]), tuple(d[r])) for r in range(n)]


def _box(c, h):
    return (tuple(c[i] - h for i in range(3)), tuple(c[i] + h for i in range(3)))


N_GENERAL = 600
F32_SPHERE_HIT_RATIO = 256.0  # the largest |oc| / r (a power of two) at which the f32 bound decides central sphere hits
ANGLES = (0.0, 1e-9, 30.0, 90.0, 180.0, 270.0, 360.0, -90.0, 750.0)
TILTED = [((-1.0, 0.25, 0.5), (1.5, -0.5, 1.0), (0.25, 1.75, -0.75)), ((2.0, 0.5, -1.0), (3.5, 0.0, 0.5), (2.5, 2.0, 0.25)),
          ((-3.0, -1.0, -0.5), (-1.5, -1.25, 1.0), (-2.0, 1.0, 0.75))]


def _zoo(wrap=lambda k, x: x):
    """One primitive of every kind, apart from each other (the container and chain cases put them in different places)."""
    objs = [sphere((-4.0, 1.0, 0.5), 1.25), rect("xy", -1.5, 0.5, 0.0, 2.0, -1.25), rect("xz", 1.0, 3.0, -1.0, 1.5, 0.5),
            rect("yz", 0.25, 2.25, -1.0, 1.0, 4.5), tri(*TILTED[0]), prism((5.5, 0.0, -1.0), (7.0, 1.5, 0.5))]
    return [wrap(k, x) for k, x in enumerate(objs)]


ZOO_AIMS = [(1, (-5.5, -0.5, -1.0), (-2.5, 2.5, 2.0)), (1, (-2.0, -0.5, -1.3), (1.0, 2.5, -1.2)), (1, (0.5, 0.45, -1.5), (3.5, 0.55, 2.0)),
            (1, (4.45, -0.25, -1.5), (4.55, 2.75, 1.5)), (1, (-1.5, -1.0, -1.0), (2.0, 2.0, 1.5)), (1, (5.0, -0.5, -1.5), (7.5, 2.0, 1.0))]


def _moved_aims(wrap, grow=1.4):
    """The zoo's aim boxes carried along by the chain `wrap` puts around object k (cubes around the moved centres)."""
    aims = []
    for k, (w, lo, hi) in enumerate(ZOO_AIMS):
        c = [0.5 * (lo[i] + hi[i]) for i in range(3)]
        h = grow * 0.5 * max(hi[i] - lo[i] for i in range(3))
        _, ops, _ = chain_of(wrap(k, sphere(c, 1.0)))
        for op in reversed(ops):
            if op.kind == "translate":
                c = [c[i] + op.a["off"][i] for i in range(3)]
            else:
                sn, cs = math.sin(math.radians(op.a["deg"])), math.cos(math.radians(op.a["deg"]))
                c = [cs * c[0] + sn * c[2], c[1], -sn * c[0] + cs * c[2]]
        aims.append((w, tuple(x - h for x in c), tuple(x + h for x in c)))
    return aims


def general_cases(mode):
    out = []
    G = lambda name, desc, rays, **kw: out.append(Case(name, desc, rays, kind="general", **kw))
    G("tilted_triangles", lst(*[tri(*t) for t in TILTED]), aimed_rays(N_GENERAL, 11, (0.0, 0.5, 0.0), 9.0, [(1, (-3.5, -1.5, -1.0), (4.0, 2.5, 1.5))], 3.0))
    # spheres seen from |oc| / r of 1 (from the surface's neighbourhood), 10^3 and 10^6.  The discriminant is a difference of
    # terms of size |oc|^2 |d|^2 known to a few u each, so a ray is only decided when it passes the centre within, or clear of
    # the sphere by, a distance the bound leaves: the aim boxes are an inner core and, for the misses, a far shell.  The f32 bound on
    # the discriminant is about 80 x 2^-24 |oc|^2 |d|^2: 5 r^2 at a ratio of 10^3 and 5 10^6 r^2 at 10^6, so in f32 those two
    # ratios are held as "sphere_far_misses" only (no false hit far away), f32 hits are judged at a ratio of 256, the largest power of
    # two the bound decides, and what the f32 core returns beyond it is shown by test_f32_sphere_records_beyond_the_decided_ratio
    if mode == "f32":  # the largest power of two at which the f32 bound still decides hits (test_primitive_cases asserts it)
        G("sphere_oc_over_r_256_f32", lst(sphere((0.0, 0.0, 0.0), 1.0)),
          aimed_rays(N_GENERAL, 19, (0.0, 0.0, 0.0), F32_SPHERE_HIT_RATIO, [(3, (-0.4, -0.4, -0.4), (0.4, 0.4, 0.4)), (1, (3.0, 3.0, 3.0), (8.0, 8.0, 8.0))],
                     1.0 / F32_SPHERE_HIT_RATIO), modes=(mode,))
    for ratio, dist in ((1, 1.0 + 2.0 ** -6), (1000, 1000.0), (1000000, 1000000.0)):
        core, shell = (3, _box((0.0, 0.0, 0.0), 0.4)[0], _box((0.0, 0.0, 0.0), 0.4)[1]), None
        if ratio == 1:
            aims = [(3, (-3.0, -3.0, -3.0), (3.0, 3.0, 3.0))]
        elif mode == "f64":
            aims = [core, (1, (2.0, 2.0, 2.0), (6.0, 6.0, 6.0)), (1, (-6.0, -6.0, -6.0), (-2.0, -2.0, -2.0))]
        elif ratio == 1000:
            aims = [(1, (12.0, 12.0, 12.0), (30.0, 30.0, 30.0)), (1, (-30.0, -30.0, -30.0), (-12.0, -12.0, -12.0))]
        else:
            aims = [(1, (20000.0, 20000.0, 20000.0), (60000.0, 60000.0, 60000.0)), (1, (-60000.0, -60000.0, -60000.0), (-20000.0, -20000.0, -20000.0))]
        far_only = mode == "f32" and ratio > 1  # named for what it holds: no false hit far from the sphere
        G(("sphere_far_misses_1e%d_%s" if far_only else "sphere_oc_over_r_1e%d_%s") % (round(math.log10(ratio)), mode), lst(sphere((0.0, 0.0, 0.0), 1.0)),
          aimed_rays(N_GENERAL, 20 + ratio % 7, (0.0, 0.0, 0.0), dist, aims, 1.0 / max(dist, 1.0)), modes=(mode,))
    # rectangles far from the origin (|p| up to 10^6): 64 wide, hits aimed at the inner quarter, misses well outside
    far = 1000000.0
    big = lst(rect("xz", far - 32.0, far + 32.0, -far - 32.0, -far + 32.0, 5.0), rect("xy", -far - 32.0, -far + 32.0, 1000.0, 1064.0, far),
              rect("yz", 0.0, 64.0, far - 32.0, far + 32.0, -1000.0))
    rays = []
    for seed, (c, h_in, h_out) in enumerate((((far, 5.0, -far), (8.0, 0.0, 8.0), (80.0, 0.0, 80.0)), ((-far, 1032.0, far), (8.0, 8.0, 0.0), (80.0, 80.0, 0.0)),
                                             ((-1000.0, 32.0, far), (0.0, 8.0, 8.0), (0.0, 80.0, 80.0)))):
        inner = (3, tuple(c[i] - h_in[i] for i in range(3)), tuple(c[i] + h_in[i] for i in range(3)))
        outer = (1, tuple(c[i] + 0.75 * h_out[i] for i in range(3)), tuple(c[i] + h_out[i] for i in range(3)))
        rays += aimed_rays(N_GENERAL // 3, 30 + seed, c, 200.0, [inner, outer], 0.01)
    G("rects_far_from_the_origin", big, rays)
    # RotateY at every angle of the list, around three kinds at once; Translate / RotateY chains of 1 to 4 ops in both orders
    for k, deg in enumerate(ANGLES):
        spin = lambda i, x, deg=deg: rotate_y(deg, x)
        G("rotate_y_%g" % deg, lst(*_zoo(spin)), aimed_rays(N_GENERAL, 40 + k, (0.0, 1.0, 0.0), 14.0, _moved_aims(spin), 0.5))
    T = lambda j, x: translate(((0.5, -0.25, 1.5), (-1.25, 0.75, 0.5))[j % 2], x)
    R = lambda j, x: rotate_y((33.0, -17.0)[j % 2], x)
    for k, order in enumerate(("T", "R", "TR", "RT", "TRT", "RTR", "TRTR", "RTRT")):
        def wrap(i, x, order=order):
            for j, op in enumerate(reversed(order)):
                x = (T if op == "T" else R)(j, x)
            return x
        G("chain_%s" % order, lst(*_zoo(wrap)), aimed_rays(N_GENERAL, 60 + k, (0.0, 1.0, 0.0), 16.0, _moved_aims(wrap), 2.0))
    # the RotateY face quirk: under a half turn the rotated ray and the normal rotated back point the same way wherever the
    # horizontal part of the direction dominates, so the reported front_face is the opposite of the geometric one
    G("rotate_y_face_quirk", lst(rotate_y(180.0, sphere((0.0, 0.0, 0.0), 2.0))),
      aimed_rays(300, 80, (0.0, 0.0, 0.0), 9.0, [(1, (-1.2, -0.4, -1.2), (1.2, 0.4, 1.2))], 1.0))
    return out


def geometric_front_face(case, r, rec_p):
    """For the quirk case (a sphere around the origin): whether the outer ray meets the surface from outside."""
    return float(np.dot(case.d[r], rec_p)) < 0.0


# ---- containers ------------------------------------------------------------------------------------------------------------
def container_worlds():
    """The same primitives in every container -> {name: (description, max_leaf, {primitive id in "top": id here})}.  "prism"
    holds the rectangle that is the front face of PRISM as a rectangle of its own in "top"."""
    zoo = _zoo
    worlds = {"top": (lst(*zoo()), 0), "group": (lst(lst(*zoo())), 0), "bvh": (lst(bvh(*zoo())), 0), "bvh_leaf1": (lst(bvh(*zoo())), 1),
              "chain": (lst(*zoo(lambda k, x: translate((0.0, 0.0, 0.0), x))), 0), "instance": (lst(inst(*zoo())), 0),
              "instance_chain": (lst(inst(*zoo(lambda k, x: translate((0.0, 0.0, 0.0), x)))), 0)}
    return worlds


def container_rays():
    rays = aimed_rays(400, 90, (1.0, 1.0, 0.0), 15.0, ZOO_AIMS, 1.5)
    # and oblique lattice rays: onto an edge of each rectangle, through the sphere's centre, onto a box face (a tie between
    # faces is decided by the container: the list order in a prism, the slot order of the flattened leaves in a BVH)
    rays += [_aimed((-1.5, 1.0, -1.25), (0.5, -0.25, -1.0)), _aimed((3.0, 0.5, 1.5), (0.25, -1.0, 0.5)), _aimed((4.5, 2.25, 1.0), (-1.0, 0.5, 0.25)),
             _aimed((-4.0, 1.0, 0.5), (0.5, 0.25, -2.0), 4.0), _aimed((7.0, 1.0, 0.0), (-1.0, -1.0, -1.0))]
    return rays


def container_columns(name, rec, ref):
    """How many columns of core_records a container shares bit for bit with the top-level spelling: all nine, or -- under a
    chain -- the eight before front_face.  A Translate faces its child's record again (hit.rs:810), the normal it is given
    already points against the ray, and so front_face under a chain reads true for every hit, also where the bare primitive
    says false; that is pinned here: every hit under the chain is a front hit, and the bare primitives do see hits from behind."""
    if "chain" not in name:
        return 9
    hit_ = ref[:, 0] == 1.0
    assert (rec[hit_, 8] == 1.0).all() and (ref[hit_, 8] == 0.0).any()
    return 8


PRISM_FACE_WORLDS = {"rect": lst(rect("xy", 0.0, 4.0, 0.0, 2.0, 8.0)), "prism": lst(prism(*PRISM))}


def prism_face_rays():
    """Rays that meet the inside of the front face of PRISM first (from z > 8, heading -z).  The face's own edges are left to
    prism_lattice_cases: there the prism's neighbouring face ties and, being later in the list, answers."""
    rays = aimed_rays(200, 91, (2.0, 1.0, 14.0), 3.0, [(1, (0.0, 0.0, 8.0), (4.0, 2.0, 8.0))], 1.0)
    rays = [r for r in rays if r[1][2] < 0.0 and r[0][2] > 8.5]
    return rays + [_aimed((x, y, 8.0), (0.25, -0.5, -1.0)) for x in (0.5, 2.0, 3.5) for y in (0.25, 1.0, 1.75)]


def core_records(orc, flat, o, d, t_min, t_max, mode):
    """The CPU core's answer per ray as an (n, 9) array: hit, t, p, normal, front_face (zeros on a miss)."""
    probe = orc.core32_world_hit if mode == "f32" else orc.core_world_hit
    ptr = flat.arrays_ptr()
    out = np.zeros((len(o), 9))
    for r in range(len(o)):
        rec = probe(ptr, tuple(o[r]), tuple(d[r]), 0.0, float(t_min), float(t_max[r]))
        if rec is not None:
            out[r] = [1.0, rec["t"], *rec["p"], *rec["normal"], float(rec["front_face"])]
    return out


def device_records(h):
    hit_ = h.ids[:, 0] == 1
    out = np.zeros((h.n, 9))
    out[:, 0] = hit_
    out[:, 1] = np.where(hit_, h.t, 0.0)
    out[:, 2:5], out[:, 5:8], out[:, 8] = h.p, h.normal, h.ids[:, 3]
    return out


def got_of_row(row, prim=None):
    if row[0] != 1.0:
        return None
    return {"t": row[1], "p": row[2:5], "normal": row[5:8], "front_face": bool(row[8]), "id": prim}


# ---- frames through the walkers -----------------------------------------------------------------------------------------------
FRAME_W, FRAME_H, FRAME_SPP, FRAME_BASE = 36, 24, 4, 8.0
FRAME_CAP = {"f64": 0.001, "f32": 0.01}  # undecided samples of a frame


def emit_colour(k):
    """Primitive k emits FRAME_BASE^(k // 3) in channel k % 3: with the base above the spp and a black background, a pixel's sum
    is a number whose base-8 digits are the hit counts of the channel's primitives, exact in f32 and f64."""
    c = [0.0, 0.0, 0.0]
    c[k % 3] = FRAME_BASE ** (k // 3)
    return tuple(c)


def decode_counts(accum, n_prims):
    """(h, w, 3) pixel sums -> (h, w, n_prims) hit counts; every sum must be a whole number below 8^digits."""
    assert np.array_equal(accum, np.round(accum)) and (accum >= 0).all()
    out = np.zeros(accum.shape[:2] + (n_prims,), dtype=np.int64)
    for k in range(n_prims):
        out[:, :, k] = np.floor(accum[:, :, k % 3] / FRAME_BASE ** (k // 3)).astype(np.int64) % int(FRAME_BASE)
    return out


def frame_scenes():
    """The three small scenes: a sphere BVH (the whole world), a triangle-mesh BVH beside top-level rectangles, a list world of
    all three kinds with wrapped members."""
    balls = [sphere((-3.0 + 1.5 * (k % 4) + 0.25 * (k // 4), 0.5 + 1.5 * (k // 4), 0.5 * (k % 3) - 0.5), 0.5 + 0.125 * (k % 3)) for k in range(8)]
    fan = [tri((-3.5 + 1.25 * k, 0.25, 0.5 * (k % 2)), (-2.5 + 1.25 * k, 0.5, -0.25), (-3.0 + 1.25 * k, 2.0 + 0.25 * (k % 3), 0.25)) for k in range(6)]
    return {"sphere_bvh": lst(bvh(*balls)),
            "mesh_and_rects": lst(bvh(*fan), rect("xz", -4.0, 4.0, -2.0, 2.0, -0.25), rect("xy", -3.0, 3.0, 2.5, 3.5, -1.5)),
            "list_world": lst(sphere((-3.0, 1.0, 0.0), 0.75), rect("yz", 0.0, 2.0, -1.0, 1.0, 3.5), tri((-1.5, 0.0, 0.5), (0.0, 0.25, 0.0), (-0.75, 1.75, -0.5)),
                              translate((1.0, 2.5, -1.0), sphere((0.0, 0.0, 0.0), 0.5)), rotate_y(30.0, prism((0.5, 0.0, -0.5), (1.5, 1.0, 0.5))),
                              translate((-1.0, 2.5, 0.0), rotate_y(-50.0, rect("xy", -0.75, 0.75, -0.5, 0.5, 0.0))))}


def frame_cam_cfg(rtsr, max_depth=4, background=(0.0, 0.0, 0.0)):
    """A pinhole.  The shutter is (0, 1): the camera refuses an empty interval, and nothing in these scenes moves."""
    cam = rtsr.Camera.new((0.5, 2.0, 12.0), (0.0, 1.25, 0.0), (0.0, 1.0, 0.0), 36.0, 1.5, 0.0, 12.0, 0.0, 1.0)
    cfg = rtsr.Config.new(1.5, FRAME_W, FRAME_SPP, max_depth, 4, seed=3, background=background)
    assert rtsr.image_height(cfg) == FRAME_H
    return cam, cfg


_FRAME_RAYS = {}


def frame_rays(rtsr, stream):
    """(h, w, spp, 2, 3): origin and direction of every sample's primary ray, the same for every scene (one camera), computed
    once per stream."""
    from features_cases import primary_ray
    key = getattr(stream, "__qualname__", repr(stream))
    if key not in _FRAME_RAYS:
        cam, cfg = frame_cam_cfg(rtsr)
        rays = np.zeros((FRAME_H, FRAME_W, FRAME_SPP, 2, 3))
        for j in range(FRAME_H):
            for i in range(FRAME_W):
                for s_ in range(FRAME_SPP):
                    o, d, _ = primary_ray(stream, cam, cfg, FRAME_H, i, j, s_)
                    rays[j, i, s_, 0], rays[j, i, s_, 1] = o, d
        _FRAME_RAYS[key] = rays
    return _FRAME_RAYS[key]


def expected_counts(rtsr, world, mode, stream):
    """Per pixel the judge's first hit of every sample's primary ray (features_cases.primary_ray on `stream`: rtsr.device_stream
    or features_cases.oracle_stream(orc)) -> (counts (h, w, n_prims), undecided (h, w)).  The f64 ray is the device's own, bit
    for bit.  The f32 build forms its ray in float: the judge takes the f64 ray with an input bound -- one rounding on the origin,
    and on a direction component eight operations on numbers of size |llc| + |horizontal| + |vertical| + |origin| -- and the
    integrator's f32 t_min, 0.001 + 2^-14 max |o| (core/geometry.hpp: ray_t_min)."""
    cam, cfg = frame_cam_cfg(rtsr)
    rays = frame_rays(rtsr, stream)
    counts = np.zeros((FRAME_H, FRAME_W, world.n_prims), dtype=np.int64)
    und = np.zeros((FRAME_H, FRAME_W), dtype=np.int64)
    size = [abs(cam.lower_left_corner[i]) + abs(cam.horizontal[i]) + abs(cam.vertical[i]) + abs(cam.origin[i]) for i in range(3)]
    for j in range(FRAME_H):
        for i in range(FRAME_W):
            for s_ in range(FRAME_SPP):
                o, d = rays[j, i, s_, 0], rays[j, i, s_, 1]
                K = Bounded(mode)
                if mode == "f32":
                    ko = tuple(K.inp(o[a], abs(o[a])) for a in range(3))
                    kd = tuple(K.inp(d[a], 8.0 * size[a]) for a in range(3))
                    t_min = float(np.float32(0.001)) + 2.0 ** -14 * max(abs(x) for x in o)
                else:
                    ko, kd, t_min = _v3(K, o), _v3(K, d), 0.001
                rec = hit(K, world.desc, ko, kd, K.num(t_min), K.num(INF))
                if K.undecided:
                    und[j, i] += 1
                elif rec is not None:
                    counts[j, i, rec["id"]] += 1
    return counts, und


def check_frame_counts(name, got, want, und):
    """A pixel's count per primitive may differ from the expected one by at most that pixel's number of undecided samples."""
    off = np.abs(got - want).max(axis=2)
    bad = np.argwhere(off > und)
    assert len(bad) == 0, "%s: pixel (j, i) = %r: counts %r, the judge %r with %d undecided" % (
        name, tuple(bad[0]), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist(), und[tuple(bad[0])])
