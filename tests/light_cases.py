"""Scenes, vertex points and independent expected radiance for next-event estimation with MIS (a helper module, not a test
file; CPU only).  tests/test_light_cases.py holds the host checker to these values, tests/test_gpu_light_cases.py the kernels,
scripts/mutate_light_sampling.py seeds faults in the estimator and runs the same comparisons.

The world of every case: the floor xz_rect(-50, 50, -50, 50, 0), Lambertian with albedo RHO (unequal channels), a black
background, and rays (0, -1, 0) from y = 0.5 onto the 16 floor points POINTS.  The floor is planar and cannot see itself, the
lights do not scatter and the background is black, so the radiance a floor ray returns is direct light only, at every
max_depth >= 2:  L = RHO / pi * E,  E the irradiance of the floor point.  E is written here in numpy alone:

  a uniform polygon      Lambert's edge formula  E = Le |sum_i theta_i n . (v_i x v_i+1) / |v_i x v_i+1|| / 2  over the unit
                         vectors to the vertices, the polygon first clipped to the floor's upper half-space;
  a sphere above the     E = pi Le (r / d)^2 cos(theta);
  horizon
  a sphere the floor     deterministic quadrature over the cone it subtends (cone_irradiance): the azimuth integral of the
  plane cuts             clipped cosine in closed form, Gauss-Legendre in the polar angle, split where the clip sets in.
                         HORIZON_ORDER = 32 nodes per piece: doubling from 8, order 16 was the first that its double moved
                         by less than 1e-7 relative at every point (horizon_order() redoes that; the test holds the
                         constant to it).

Nothing here reads csrc/.  The texel mapping of `image_rect` restates the reference's ImageTexture::value (u clamped, v flipped,
index = int(u * width) capped at width - 1, colour / 255) and a rectangle's own (u, v) = ((a - a0) / (a1 - a0), (b - b0) /
(b1 - b0)).

Geometry: the cases keep the geometry they were proposed with.  Nothing had to move: no point lies under an occluder's edge
(half_shadow's absorber ends at x = 0, no point has x = 0), and every point of sphere_on_horizon is outside its sphere.  Two
cases were added because a seeded fault survived without them: sphere_axes (a sphere exactly above a point, where the cone
frame's axis choice decides) and image_sphere (a textured sphere light); RED_BLUE and BLACK_RED serve the light draw at exact
cdf values (pick_check)."""
import numpy as np

RHO = np.array([0.8, 0.6, 0.4])
POINTS = [(x, z) for x in (-3.0, -0.7, 0.4, 2.5) for z in (-2.0, 0.3, 1.9, 6.0)]
N_UP = np.array([0.0, 1.0, 0.0])
HORIZON_ORDER = 32   # Gauss-Legendre nodes per piece: orders 16 and 32 agree to 1e-7 at every point (horizon_order() = 16)

# samples per point of the statistical comparisons: REPLICAS rays per point (distinct ray indices: distinct streams) x SPP
# = 2^18; a case whose light sampling needs more to resolve 0.5 % says so (Case.replicas): light_in_front 2^20 (most draws go
# to a ceiling that sends each point little), the half shadows 2^19 (most draws at the edge points are occluded).
REPLICAS, SPP = 64, 4096
SEED = 1
Z_CAP, REL_SE_CAP = 4.5, 0.005


# ---- irradiance in closed form ----------------------------------------------------------------------------------------------
def _clip(V, n, p):
    """Sutherland-Hodgman: the part of polygon V with n . (x - p) >= 0."""
    out = []
    for i in range(len(V)):
        a, b = V[i], V[(i + 1) % len(V)]
        da, db = np.dot(n, a - p), np.dot(n, b - p)
        if da >= 0:
            out.append(a)
        if (da > 0 and db < 0) or (da < 0 and db > 0):
            out.append(a + (b - a) * (da / (da - db)))
    return out


def polygon_form(V, p, n=N_UP):
    """E / Le of a uniform two-sided polygon at point p of a surface with normal n (Lambert's formula)."""
    V = _clip([np.asarray(v, dtype=np.float64) for v in V], n, p)
    if len(V) < 3:
        return 0.0
    U = [(v - p) / np.linalg.norm(v - p) for v in V]
    s = 0.0
    for i in range(len(U)):
        a, b = U[i], U[(i + 1) % len(U)]
        c = np.cross(a, b)
        cn = np.linalg.norm(c)
        if cn == 0:
            continue
        s += np.arctan2(cn, np.dot(a, b)) * np.dot(n, c / cn)
    return abs(s) / 2.0


def rect_vertices(kind, a0, a1, b0, b1, k):
    P = [(a0, b0), (a1, b0), (a1, b1), (a0, b1)]
    if kind == "xy":
        return [(a, b, k) for a, b in P]
    if kind == "xz":
        return [(a, k, b) for a, b in P]
    return [(k, a, b) for a, b in P]


def sphere_form(c, r, p):
    """E / Le of a sphere wholly above the horizon of p."""
    d = np.asarray(c, dtype=np.float64) - p
    dist = np.linalg.norm(d)
    assert d[1] - r >= 0 or dist * dist - r * r > 0
    return np.pi * (r / dist) ** 2 * (d[1] / dist)


def cone_irradiance(c, r, p, order):
    """E / Le of the part of a sphere above the horizon of p (p outside it): the integral of max(0, dir.y) over the cone the
    sphere subtends.  In the frame (w towards the centre, u the upward direction orthogonal to w) dir.y = A + B cos(phi) with
    A = cos(alpha) w.y, B = sin(alpha) u.y >= 0; its positive part integrates over phi in closed form, and the rest is
    Gauss-Legendre in alpha over [0, alpha_max], split at |A| = B where the clip sets in."""
    oc = np.asarray(c, dtype=np.float64) - p
    d = np.linalg.norm(oc)
    assert d > r
    w = oc / d
    uy = np.sqrt(max(0.0, 1.0 - w[1] * w[1]))   # u = (y - (y.w) w) / |.|, so u.y = sqrt(1 - w.y^2)
    amax = np.arcsin(r / d)
    cuts = [0.0, amax]
    if uy > 0:
        a_star = np.arctan2(abs(w[1]), uy)
        if 0.0 < a_star < amax:
            cuts = [0.0, a_star, amax]
    x, wt = np.polynomial.legendre.leggauss(order)
    total = 0.0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        al = 0.5 * (hi - lo) * x + 0.5 * (hi + lo)
        A, B = np.cos(al) * w[1], np.sin(al) * uy
        inner = np.zeros_like(al)
        full = A >= B
        part = (~full) & (A > -B)
        inner[full] = 2.0 * np.pi * A[full]
        phi0 = np.arccos(np.clip(-A[part] / B[part], -1.0, 1.0))
        inner[part] = 2.0 * (A[part] * phi0 + B[part] * np.sin(phi0))
        total += 0.5 * (hi - lo) * np.sum(wt * inner * np.sin(al))
    return total


def horizon_order(c, r, points, tol=1e-7):
    """The first order, doubling from 8, whose value differs from the doubled order's by less than tol relative at every point."""
    order = 8
    prev = np.array([cone_irradiance(c, r, p, order) for p in points])
    while True:
        nxt = np.array([cone_irradiance(c, r, p, 2 * order) for p in points])
        if np.all(np.abs(nxt - prev) <= tol * np.abs(nxt)):
            return order
        order, prev = 2 * order, nxt


# ---- lights and cases -------------------------------------------------------------------------------------------------------
def rect(kind, a0, a1, b0, b1, k, le=None, texels=None, under_translate=False):
    """texels: (2, 2, 3) emitted colours in radiance units, row 0 the first image row (v > 0.5)."""
    return dict(kind=kind, ab=(a0, a1, b0, b1), k=float(k), le=None if le is None else np.array(le, dtype=np.float64),
                texels=None if texels is None else np.array(texels, dtype=np.float64), under_translate=under_translate)


def sphere(c, r, le=None, texels=None):
    return dict(kind="sphere", c=np.array(c, dtype=np.float64), r=float(r), le=None if le is None else np.array(le, dtype=np.float64),
                texels=None if texels is None else np.array(texels, dtype=np.float64), under_translate=False)


def sphere_texel_of(n):
    """(row, column) of the texel a sphere shows at the outward unit normal n, restated from the reference's get_sphere_uv:
    theta = acos(-n.y), phi = atan2(-n.z, n.x) + pi, (u, v) = (phi / 2 pi, theta / pi)."""
    return texel_of((np.arctan2(-n[2], n[0]) + np.pi) / (2.0 * np.pi), np.arccos(-n[1]) / np.pi)


def texel_of(u, v, width=2, height=2):
    """(row, column) of the reference's ImageTexture::value."""
    u, v = min(max(u, 0.0), 1.0), 1.0 - min(max(v, 0.0), 1.0)
    return min(int(v * height), height - 1), min(int(u * width), width - 1)


def rect_irradiance(L, p, window=None):
    """E (3,) of a rectangle light at floor point p; window = (a0, a1, b0, b1): only that part of it is seen.  A textured light
    is the sum of its four quarters, each uniform with the colour of its texel."""
    a0, a1, b0, b1 = L["ab"] if window is None else window
    if L["texels"] is None:
        return L["le"] * polygon_form(rect_vertices(L["kind"], a0, a1, b0, b1, L["k"]), p)
    assert window is None
    E = np.zeros(3)
    am, bm = 0.5 * (a0 + a1), 0.5 * (b0 + b1)
    for qa0, qa1 in ((a0, am), (am, a1)):
        for qb0, qb1 in ((b0, bm), (bm, b1)):
            u, v = (0.5 * (qa0 + qa1) - a0) / (a1 - a0), (0.5 * (qb0 + qb1) - b0) / (b1 - b0)
            j, i = texel_of(u, v)
            E += L["texels"][j, i] * polygon_form(rect_vertices(L["kind"], qa0, qa1, qb0, qb1, L["k"]), p)
    return E


def light_irradiance(L, p):
    return L["le"] * sphere_form(L["c"], L["r"], p) if L["kind"] == "sphere" else rect_irradiance(L, p)


def light_area(L):
    if L["kind"] == "sphere":
        return 4.0 * np.pi * L["r"] ** 2
    a0, a1, b0, b1 = L["ab"]
    return abs(a1 - a0) * abs(b1 - b0)


def texel_colours(L):
    """The colours the texture returns, with its own arithmetic: (1 / 255) * the stored texel (stored as colour * 255)."""
    return (1.0 / 255.0) * (L["texels"] * 255.0)


def centre_colour(L):
    """What the light table weighs a light by: its colour at (u, v) = (0.5, 0.5)."""
    if L["texels"] is None:
        return L["le"]
    j, i = texel_of(0.5, 0.5)
    return L["texels"][j, i]


class Case:
    def __init__(self, name, lights, expected=None, fog=None, rays=None, exact=False, replicas=None, judged_by_plain=False):
        self.name, self.lights, self.fog, self.exact = name, lights, fog, exact
        self.judged_by_plain = judged_by_plain or fog is not None   # no closed form: the plain estimator is the judge
        self.replicas = replicas or REPLICAS   # x SPP samples per point in the statistical comparisons
        self._expected = expected
        self._rays = rays

    def expected(self):
        """(16, 3) radiance of the floor rays, or None where the judge is the plain estimator (fog_vertex, image_sphere)."""
        if self.judged_by_plain:
            return None
        P = [np.array([x, 0.0, z]) for x, z in POINTS]
        if self.exact:   # the radiance itself, with no division
            return np.array([self._expected(p) for p in P])
        if self._expected is not None:
            return np.array([RHO / np.pi * self._expected(p) for p in P])
        return np.array([RHO / np.pi * sum(light_irradiance(L, p) for L in self.lights) for p in P])

    def rays(self):
        """(origins, directions) of the 16 rays."""
        if self._rays is not None:
            return self._rays
        o = np.array([[x, 0.5, z] for x, z in POINTS])
        return o, np.tile([0.0, -1.0, 0.0], (len(o), 1))

    def census(self):
        """What Flat.lights() must report, from the light list alone."""
        sampled = [L for L in self.lights if not L["under_translate"]]
        return dict(n_lights=len(sampled), n_rect_lights=sum(L["kind"] != "sphere" for L in sampled),
                    n_sphere_lights=sum(L["kind"] == "sphere" for L in sampled),
                    n_unsampled_emitters=len(self.lights) - len(sampled), total_area=sum(light_area(L) for L in sampled))

    def pick_weights(self):
        """area x max channel of the centre colour per sampled light, uniform if all are 0 (host/light_table.hpp's rule)."""
        w = np.array([light_area(L) * max(centre_colour(L)) for L in self.lights if not L["under_translate"]])
        return w / w.sum() if w.sum() > 0 else np.full(len(w), 1.0 / max(len(w), 1))

    def build(self, rtsr):
        """(builder, flat) -- keep both alive while the flat scene is in use."""
        b = rtsr.Builder(1)
        lst = b.hittable_list()
        b.list_add(lst, b.xz_rect(-50, 50, -50, 50, 0.0, b.lambertian(tuple(RHO))))
        for L in self.lights:
            emit = tuple(L["le"]) if L["texels"] is None else b.image_from_texels(L["texels"] * 255.0)
            m = b.diffuse_light(emit)
            h = b.sphere(tuple(L["c"]), L["r"], m) if L["kind"] == "sphere" else getattr(b, L["kind"] + "_rect")(*L["ab"], L["k"], m)
            b.list_add(lst, b.translate((0.0, 0.0, 0.0), h) if L["under_translate"] else h)
        if self.fog is not None:
            c, r, density, albedo = self.fog
            b.list_add(lst, b.constant_medium(albedo, density, b.sphere(c, r, b.lambertian((0.5, 0.5, 0.5)))))
        return b, b.flatten(lst)

    def aimed_rays(self):
        """One ray per light that meets it first, from 0.25 away: (origins, directions, the emitted colour at the hit)."""
        o, d, le = [], [], []
        for L in self.lights:
            if L["kind"] == "sphere":
                out = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
                o.append(L["c"] + (L["r"] + 0.25) * out)
                d.append(-out)
                le.append(L["le"] if L["texels"] is None else texel_colours(L)[sphere_texel_of(out)])
                continue
            a0, a1, b0, b1 = L["ab"]
            u, v = 0.3, 0.7
            a, bb = a0 + u * (a1 - a0), b0 + v * (b1 - b0)
            t = {"xy": (a, bb, L["k"]), "xz": (a, L["k"], bb), "yz": (L["k"], a, bb)}[L["kind"]]
            n = {"xy": (0.05, 0.03, 0.25), "xz": (0.05, 0.25, 0.03), "yz": (0.25, 0.05, 0.03)}[L["kind"]]
            o.append(np.array(t) + np.array(n))
            d.append(-np.array(n))
            if L["texels"] is None:
                le.append(L["le"])
            else:
                j, i = texel_of(u, v)
                le.append(texel_colours(L)[j, i])
        return np.array(o), np.array(d), np.array(le)


LE = (4.0, 3.0, 2.0)
XZ = rect("xz", -1, 1, -0.5, 1.5, 2, LE)
CEILING = rect("xz", -30, 30, -30, 30, 9, (0.3, 0.3, 0.9))
SMALL_SPHERE = sphere((0.5, 2.5, 0.2), 0.3, (20, 3, 2))
HORIZON_SPHERE = sphere((-0.2, 0.3, 3.8), 1.0, LE)
# all four texels differ; the centre texel (row 1, column 1) is the brightest in no channel twice
QUAD_TEXELS = [[(4.0, 0.5, 0.5), (0.5, 3.0, 0.2)], [(0.2, 0.4, 5.0), (2.0, 2.0, 1.0)]]
# black centre texel, bright others: pick weight 0
DARK_CENTRE = [[(4.0, 3.0, 2.0), (1.0, 5.0, 2.0)], [(3.0, 1.0, 6.0), (0.0, 0.0, 0.0)]]
ABSORBER_AB, ABSORBER_K = (-20.0, 0.0, -20.0, 20.0), 1.0


def _in_front(p):
    # the sphere hides the ceiling behind it: the ceiling everywhere, plus the sphere with what it adds over the ceiling
    hidden = dict(SMALL_SPHERE, le=SMALL_SPHERE["le"] - CEILING["le"])
    return light_irradiance(CEILING, p) + light_irradiance(hidden, p)


def _half_shadow(p):
    """The absorber (y = ABSORBER_K, parallel to the light) seen from floor point p covers, in the light's plane, its own
    rectangle scaled about p by k_light / k_absorber (similar triangles); what is left of the light must be a rectangle."""
    s = XZ["k"] / ABSORBER_K
    a0, a1, b0, b1 = XZ["ab"]
    x0, x1 = p[0] + (ABSORBER_AB[0] - p[0]) * s, p[0] + (ABSORBER_AB[1] - p[0]) * s
    z0, z1 = p[2] + (ABSORBER_AB[2] - p[2]) * s, p[2] + (ABSORBER_AB[3] - p[2]) * s
    assert z0 < b0 and z1 > b1 and x0 < a0   # only the absorber's x1 edge can cut the light
    assert abs(x1 - a0) > 1e-9 and abs(x1 - a1) > 1e-9
    if x1 <= a0:
        return rect_irradiance(XZ, p)
    if x1 >= a1:
        return np.zeros(3)
    return rect_irradiance(XZ, p, window=(x1, a1, b0, b1))


def _horizon(p):
    return HORIZON_SPHERE["le"] * cone_irradiance(HORIZON_SPHERE["c"], HORIZON_SPHERE["r"], p, HORIZON_ORDER)


def _absorber(under_translate):
    return rect("xz", *ABSORBER_AB, ABSORBER_K, (0.0, 0.0, 0.0), under_translate=under_translate)


def _fog_rays():
    o = np.array([[-4.5, y, z] for y in (0.6, 0.9, 1.2, 1.5) for z in (0.1, 0.4, 0.7, 1.0)])
    return o, np.tile([1.0, 0.05, 0.0], (len(o), 1))


CASES = {c.name: c for c in (
    Case("xz", [XZ]),
    Case("xy", [rect("xy", -1, 1, 0.2, 2.5, -3, LE)]),
    Case("yz_through_floor", [rect("yz", -1, 2, -1, 1.5, -4, LE)]),
    Case("sphere", [sphere((0.5, 2.5, 0.2), 0.8, LE)]),
    Case("multi", [rect("yz", 0.5, 2, -1, 1.5, -4, (1, 8, 2)), sphere((7.5, 2.5, 0.2), 0.3, (20, 3, 2)),
                   rect("xz", -3, 3, -3, 3, 9, (0.3, 0.3, 0.9)), rect("xy", -1, 1, 0.2, 2.5, 12, (0, 0, 0))]),
    Case("light_in_front", [CEILING, SMALL_SPHERE], expected=_in_front, replicas=256),
    Case("inside_sphere", [sphere((0, 0, 0), 20, LE)], expected=lambda p: RHO * np.array(LE), exact=True),
    Case("all_zero_weights", [rect("xz", -1, 1, -0.5, 1.5, 2, texels=DARK_CENTRE), rect("xy", -1, 1, 0.2, 2.5, -3, texels=DARK_CENTRE)]),
    Case("image_rect", [rect("xz", -1, 1, -0.5, 1.5, 2, texels=QUAD_TEXELS)]),
    Case("half_shadow_translated", [XZ, _absorber(True)], expected=_half_shadow, replicas=128),
    Case("half_shadow_top_level", [XZ, _absorber(False)], expected=_half_shadow, replicas=128),
    Case("unsampled", [dict(XZ, under_translate=True)]),
    Case("sphere_on_horizon", [HORIZON_SPHERE], expected=_horizon),
    # both arms of the cone frame's axis choice: one sphere straight above the point (0.4, 0.3), where the direction to its
    # centre is (0, 1, 0) exactly, and one low in +x, seen with |w.x| > 0.9 from every point
    Case("sphere_axes", [sphere((0.4, 2.5, 0.3), 0.5, LE), sphere((6.0, 0.8, 0.3), 0.5, (2, 6, 3))]),
    # a textured sphere light: the (u, v) nee_connect computes for the point it draws on a sphere.  The four quadrants of a
    # sphere have no simple form factor, so the judge is the plain estimator, which shades with the hit's own (u, v); the ray
    # aimed at it pins that mapping's orientation (exact_check)
    Case("image_sphere", [sphere((0.5, 2.5, 0.2), 0.8, texels=QUAD_TEXELS)], judged_by_plain=True),
    Case("fog_vertex", [XZ, sphere((2.5, 1.5, 0.2), 0.3, (20, 3, 2))], fog=((-2.5, 1.0, 0.5), 0.8, 1.5, (0.9, 0.7, 0.5)),
         rays=_fog_rays()),
)}


# ---- tracing and statistics -------------------------------------------------------------------------------------------------
def replicated(o, d, replicas=REPLICAS):
    """Ray r = replica * 16 + point."""
    return np.tile(o, (replicas, 1)), np.tile(d, (replicas, 1))


def mean_and_se(S, Q, spp, n_points=16):
    """Per point and channel: the mean and its standard error over all replicas' samples, from the per-ray sums."""
    S3 = np.asarray(S, dtype=np.float64).reshape(-1, n_points, 3)
    Q3 = np.asarray(Q, dtype=np.float64).reshape(-1, n_points, 3)
    n = spp * S3.shape[0]
    s, q = S3.sum(axis=0), Q3.sum(axis=0)
    var_of_mean = np.maximum(q - s * s / n, 0.0) / (n - 1) / n
    return s / n, np.sqrt(var_of_mean)


def z_scores(mean, se, expected, se_expected=0.0):
    """|mean - expected| in combined standard errors; a difference of exactly 0 scores 0, a non-zero one at zero error inf."""
    d, e = np.abs(mean - expected), np.sqrt(se * se + se_expected * se_expected)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0, 0.0, d / e)


def host_tracer(chk, flat, threads=8):
    """trace(o, d, spp, max_depth, light_sampling) -> (sum, sumsq) by the f64 host checker (trace_rays_cases.checkers), the rays
    cut into chunks traced side by side: ray r keeps the stream of ray index r, so the sums are those of one call."""
    from concurrent.futures import ThreadPoolExecutor
    import trace_rays_cases as tc

    def trace(o, d, spp, max_depth, light_sampling):
        n = len(o)
        S, Q = np.zeros((n, 3)), np.zeros((n, 3))
        cuts = np.linspace(0, n, min(4 * threads, n) + 1).astype(int)

        def part(k):
            lo, hi = cuts[k], cuts[k + 1]
            S[lo:hi], Q[lo:hi] = tc.host_trace(chk, flat, o[lo:hi], d[lo:hi], spp=spp, max_depth=max_depth, background=(0, 0, 0),
                                               seed=SEED, first_ray=int(lo), light_sampling=light_sampling)
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(part, range(len(cuts) - 1)))
        return S, Q
    return trace


def statistical_check(case, trace, depths=(2, 50), spp=SPP):
    """Both estimators of `trace` against the case's expected radiance at every depth -> (lines to print, failed conditions).
    Conditions: every point and channel within Z_CAP standard errors; with light sampling, relative standard error <=
    REL_SE_CAP wherever light arrives (not with an empty light table: that is the plain estimator).  inside_sphere is held
    exactly by exact_check instead.  fog_vertex and image_sphere have no expected value: light sampling against the plain estimator at equal
    spp, in combined standard errors."""
    lines, failed = [], []
    if case.exact:
        return lines, failed
    o, d = replicated(*case.rays(), case.replicas)
    ex = case.expected()
    sampled = case.census()["n_lights"] > 0
    for depth in depths:
        m1, e1 = mean_and_se(*trace(o, d, spp, depth, True), spp)
        m0, e0 = mean_and_se(*trace(o, d, spp, depth, False), spp)
        if ex is None:
            z = z_scores(m1, e1, m0, e0)
            lines.append("%s depth %d: light sampling against plain, max z %.2f" % (case.name, depth, z.max()))
            if not z.max() <= Z_CAP:
                failed.append("%s depth %d: z %.2f against the plain estimator" % (case.name, depth, z.max()))
            continue
        z1, z0 = z_scores(m1, e1, ex), z_scores(m0, e0, ex)
        lit = ex > 0
        rel = float((e1[lit] / ex[lit]).max()) if lit.any() else 0.0
        rel0 = float((e0[lit] / ex[lit]).max()) if lit.any() else 0.0
        lines.append("%s depth %d: light sampling max z %.2f, max relative SE %.4f; plain max z %.2f, max relative SE %.4f"
                     % (case.name, depth, z1.max(), rel, z0.max(), rel0))
        if not z1.max() <= Z_CAP:
            k = np.unravel_index(np.argmax(z1), z1.shape)
            failed.append("%s depth %d light sampling: z %.2f at point %s channel %d (%.6g, expected %.6g)"
                          % (case.name, depth, z1.max(), POINTS[k[0]], k[1], m1[k], ex[k]))
        if sampled and not rel <= REL_SE_CAP:
            failed.append("%s depth %d light sampling: relative SE %.4f" % (case.name, depth, rel))
        if not z0.max() <= Z_CAP:
            failed.append("%s depth %d plain: z %.2f" % (case.name, depth, z0.max()))
    return lines, failed


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def exact_check(case, trace, replicas=64, spp=2):
    """The checks by bit pattern -> failed conditions.  At max_depth 1 a floor ray returns exactly 0 under both estimators (no
    connection at the last allowed vertex) and a ray aimed at a light exactly its emitted colour (the first vertex carries
    weight 1): spp = 2, so the sums are 2 Le and 2 Le^2 without rounding.  inside_sphere: every sample is fl(RHO * Le).  With an
    empty light table (unsampled) light sampling returns the plain estimator's sums."""
    failed = []
    o, d = replicated(*case.rays(), replicas)
    ao, ad, le = case.aimed_rays()
    ao, ad, le = np.tile(ao, (replicas, 1)), np.tile(ad, (replicas, 1)), np.tile(le, (replicas, 1))
    for nee in (True, False):
        S, Q = trace(o, d, spp, 1, nee)
        if case.fog is None and (S.any() or Q.any()):
            failed.append("%s light_sampling %d: floor rays at max_depth 1 are not 0" % (case.name, nee))
        S, Q = trace(ao, ad, spp, 1, nee)
        if not (np.array_equal(_bits(S), _bits(spp * le)) and np.array_equal(_bits(Q), _bits(spp * (le * le)))):
            failed.append("%s light_sampling %d: aimed rays at max_depth 1 are not Le: %s" % (case.name, nee, (S / spp - le)[:len(case.lights)]))
        if case.exact:
            x = np.tile(case.expected(), (replicas, 1))
            for depth in (2, 50):
                S, Q = trace(o, d, spp, depth, nee)
                if not (np.array_equal(_bits(S), _bits(spp * x)) and np.array_equal(_bits(Q), _bits(spp * (x * x)))):
                    failed.append("%s light_sampling %d depth %d: not exactly RHO * Le" % (case.name, nee, depth))
    if case.census()["n_lights"] == 0:
        for depth in (2, 50):
            (S1, Q1), (S0, Q0) = trace(o, d, 64, depth, True), trace(o, d, 64, depth, False)
            if not (np.array_equal(_bits(S1), _bits(S0)) and np.array_equal(_bits(Q1), _bits(Q0)) and S0.any()):
                failed.append("%s depth %d: an empty light table changes the sums" % (case.name, depth))
    return failed


# ---- frames (k_trace_nee against tests/nee_host_check.cpp) ---------------------------------------------------------------------
FRAME_WIDTH, FRAME_SPP, FRAME_SEED = 24, 4, 3


def frame_camera(rtsr):
    """A camera above the floor and the low lights, below the ceilings, looking down at the points."""
    return rtsr.Camera.new((0.4, 7.0, 1.2), (0.3, 0.0, 1.0), (0.0, 0.0, 1.0), 60.0, 1.0, 0.0, 10.0, 0.0, 1.0)


def nee_checker(tmp_path_factory):
    """nee_host_render of tests/nee_host_check.cpp, built with oracle/Makefile's CXXFLAGS (trace_rays_cases.CXXFLAGS)."""
    import ctypes as C
    import os
    import subprocess
    import trace_rays_cases as tc
    out = str(tmp_path_factory.mktemp("nee_host_light_cases") / "nee_host_check.so")
    subprocess.run(["g++"] + tc.CXXFLAGS + ["-shared", os.path.join(tc.ROOT, "tests", "nee_host_check.cpp"), "-o", out], check=True)
    fn = C.CDLL(out).nee_host_render
    D = C.POINTER(C.c_double)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, D, D, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, D]
    return fn


def host_frame(fn, flat, cam, height, max_depth):
    import ctypes as C
    D = C.POINTER(C.c_double)
    camarr = np.frombuffer(bytes(cam), dtype=np.float64).copy()
    bg = np.zeros(3)
    out = np.zeros((height, FRAME_WIDTH, 3))
    rc = fn(flat.arrays_ptr(), camarr.ctypes.data_as(D), bg.ctypes.data_as(D), FRAME_WIDTH, height, FRAME_SPP, max_depth, FRAME_SEED,
            out.ctypes.data_as(D))
    assert rc == 0, rc
    return out


# ---- the light draw at exact cdf values (tests/light_pick_host_check.cpp) ------------------------------------------------------
def pick_checker(out_dir, src=None):
    """light_pick_host built with trace_rays_cases.CXXFLAGS -> pick(flat, p, s0, s1) -> (the light draw, the connection's rgb)."""
    import ctypes as C
    import os
    import subprocess
    import trace_rays_cases as tc
    out = os.path.join(str(out_dir), "light_pick_host_check.so")
    subprocess.run(["g++"] + tc.CXXFLAGS + ["-shared", src or os.path.join(tc.ROOT, "tests", "light_pick_host_check.cpp"), "-o", out], check=True)
    fn = C.CDLL(out).light_pick_host
    D = C.POINTER(C.c_double)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, D, D, C.c_uint64, C.c_uint64, D, D]

    def pick(flat, p, s0, s1):
        p, rho, u, rgb = np.array(p, dtype=np.float64), RHO.copy(), np.zeros(1), np.zeros(3)
        rc = fn(flat.arrays_ptr(), p.ctypes.data_as(D), rho.ctypes.data_as(D), s0, s1, u.ctypes.data_as(D), rgb.ctypes.data_as(D))
        assert rc == 0, rc
        return float(u[0]), rgb
    return pick


# two lights of equal pick weight (area 2 x max channel 4), one red, one blue: cdf = (0.5, 1) exactly, and the colour of a
# connection tells which was drawn; and a light of weight 0 in front of a red one: cdf = (0, 1)
RED_BLUE = Case("red_blue", [rect("xz", -1, 0, -0.5, 1.5, 2, (4, 0, 0)), rect("xz", 0, 1, -0.5, 1.5, 2, (0, 0, 4))])
BLACK_RED = Case("black_red", [rect("xy", -1, 1, 0.2, 2.5, 12, (0, 0, 0)), rect("xz", -1, 0, -0.5, 1.5, 2, (4, 0, 0))])
PICK_VERTEX = (0.1, 0.0, 0.4)


def pick_check(rtsr, pick):
    """The draw u picks the first light with u < cdf, so that cdf differences are the exact pick probabilities on the 2^-53 grid
    of the draws -> failed conditions.  States: s0 + s1 = the wanted 64-bit output (mod 2^64), for several s0."""
    failed = []
    M = 1 << 64
    states = lambda out: [(s0, (out - s0) % M) for s0 in (1, 0x9E3779B97F4A7C15, 0x0123456789ABCDEF, M - 5)]
    b1, red_blue = RED_BLUE.build(rtsr)
    b2, black_red = BLACK_RED.build(rtsr)
    assert list(RED_BLUE.pick_weights()) == [0.5, 0.5] and list(BLACK_RED.pick_weights()) == [0.0, 1.0]
    for want_u, out, flat, channel, what in (
            (0.5 - 2.0 ** -53, (1 << 63) - (1 << 11), red_blue, 0, "u just under cdf[0] = 0.5 draws light 0 (red)"),
            (0.5, 1 << 63, red_blue, 2, "u = cdf[0] = 0.5 draws light 1 (blue)"),
            (0.5, (1 << 63) + 2047, red_blue, 2, "u = cdf[0] = 0.5 (low bits set) draws light 1 (blue)"),
            (0.0, 0, red_blue, 0, "u = 0 draws light 0 (red)"),
            (1.0 - 2.0 ** -53, M - 1, red_blue, 2, "the largest u draws light 1 (blue)"),
            (0.0, 0, black_red, 0, "u = 0 = cdf[0] of a weight-0 light draws the next light (red)"),
            (0.0, 1500, black_red, 0, "u = 0 = cdf[0] of a weight-0 light draws the next light (red)")):
        for s0, s1 in states(out):
            u, rgb = pick(flat, PICK_VERTEX, s0, s1)
            other = [c for c in range(3) if c != channel]
            if u != want_u or not rgb[channel] > 0 or rgb[other].any():
                failed.append("light draw: %s: u = %r, connection %s" % (what, u, rgb))
                break
    return failed
