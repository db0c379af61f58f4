"""Materials and media at their edges: every scatter rule and every boundary rule of ConstantMedium against closed forms (a
helper module, not a test file; all of it runs on the CPU and it reads nothing under csrc/).  tests/test_material_cases.py
proves the cases on the CPU against judges that share no code with the kernels; tests/test_gpu_material_cases.py runs the
device on them; scripts/mutate_materials.py seeds faults in the shared core and runs the CPU file.

The probe.  Every statistical probe is built so that the sum trace_rays returns is an integer count times a pure colour:
emitters and the background carry one channel each, max_depth is 1 or 2 and every albedo is 0, 0.5 or 1 per channel, so a
path contributes exactly one colour (times Case.unit) or exactly 0.  RED is "reflected", BLUE is "refracted" / "transmitted" /
"survived", and GREEN surrounds every target: one green sample is a failure by itself, not a statistic.  Where two surfaces
share a t the target comes later in the list: the later object wins an exact tie (test_list_tie_later_object_wins pins it).

Closed forms (numpy only, longdouble where a threshold is involved, evaluated from the DOUBLES the ray is made of):
  glass     a Dielectric xz_rect at y = 0 (one rectangle is both faces and has no second interface).  Reflect share
            r0 + (1 - r0) (1 - cos)^5, r0 = ((1 - ratio) / (1 + ratio))^2, ratio = 1 / ir from above and ir from below, cos the
            incident cosine on either face (the reference's rule, hit.rs:1095-1118); every sample reflects once ratio sin > 1.
            The reflected ray lands on the strip the mirror rule names, the refracted one on the strip Snell's law names
            (planes y = +-H; half-width 1e-6 of the flight distance).
  metal     fuzz 0: every sample on the mirror strip.  Fuzz f at incident cosine c: the scattered direction is r + f s, s
            uniform in the unit ball, absorbed when (r + f s) . n <= 0, i.e. s_n <= -h with h = c / |f|: the cap fraction
            (1 - h)^2 (2 + h) / 4, and 0 when h >= 1.  Survivors carry the albedo (0.5: a second application would show).
  medium    transmitted share exp(-density L), L the Euclidean length of the chord that lies behind max(rec1.t, t_min, 0):
            the 0.001 of the integrator's t_min is NOT medium for a ray that starts inside or on the boundary.
  casts     one world_hit on the stream of seed + r: with u the FIRST uniform of that stream (the judge's own, through
            oracle_sample_stream) the hit is at t = t1 + (neg_inv_density log u) / |d| when that distance is not greater than
            (t2 - t1) |d| -- restated in numpy operation by operation (medium_hit_restated), with the project's rt_log, and
            held to numpy's own log within 2 ulps.  This covers density -1 (a hit BEFORE t1) with an expected t.
  two media the earlier slot draws first; the later one sees min(rec2, the earlier one's hit) as its far end and skips its
            draw when nothing is left (two_media_shares).

  isotropic a slab of optical depth 2 under a half-space emitter: the share that scatters in the first flight and then leaves
            upward unscattered, a Gauss-Legendre value over (scatter depth, direction cosine, |s|) that includes the 0.001 |s|
            of the second flight t_min exempts; the order doubles until the value moves by less than 1e-7 (slab_order).
  shell     probes along the axis of a hollow glass shell inside the sphere walkers' BVH: four interfaces at normal incidence,
            the share that leaves through the back from a linear system in r0 (shell_back_share).

Lambertian needs no new closed form: tests/light_cases.py holds its cosine law under every light kind.

Statistics: light_cases.py's rule, both caps asserted.  Every share within Z_CAP = 4.5 binomial standard errors of its closed
form, the standard error from the closed form (a share of exactly 0 or 1 is an exact count), and a relative standard error of at
most REL_SE_CAP = 0.5 %.  N = 2^18 samples per point, seeds fixed.  Most shares are counts of one of two outcomes, not
radiance: there the relative error is that of the LARGER of the share and its complement (rel_se says why); the Isotropic slab
reports radiance, holds the cap on the share itself and takes 2^20 samples for it (0.23 %).  The casts' shares follow the same
rule at 2^16 rays per set.  No geometry had to move for a seed.
About 340 statistical points in all: at 4.5 standard errors the chance of a false alarm over the family is below 0.5 %.
At ir = 1.000001 the two critical-angle probes stand 1e-6 rad, not 1e-9 rad, from the threshold (see _glass_pane)."""
import numpy as np

LD = np.longdouble
RED, GREEN, BLUE, BLACK, WHITE = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
REPLICAS, SPP = 64, 4096          # 2^18 samples per point
N_SAMPLES = REPLICAS * SPP
SEED = 1
Z_CAP, REL_SE_CAP = 4.5, 0.005
FRAME_WIDTH, FRAME_HEIGHT, FRAME_SPP, FRAME_DEPTH = 48, 32, 8, 50
F_MEDIUM_GENERAL, F_MEDIUM_SPHERE = 1 << 18, 1 << 19   # the feature bits of a flat scene (restated; oracle_py.flat_features)
IRS = (1.5, 2.4, 1.0, 1.0 / 1.5, 1.000001)
H, BIG = 2.0, 1.0e6               # the target planes y = +-H of the panes; the half-extent of panes and planes


class Point:
    """One probe ray and the closed-form share (of N samples, in units of Case.unit) each channel must show; a share of
    exactly 0 or 1 is an exact count."""

    def __init__(self, o, d, shares, tag, time=0.0, f32=True):
        self.o, self.d, self.shares, self.tag, self.time, self.f32 = tuple(float(x) for x in o), tuple(float(x) for x in d), tuple(shares), tag, time, f32


class Case:
    def __init__(self, name, rtsr, max_depth, background, unit=1.0, seed=31, replicas=None):
        self.name, self.max_depth, self.background, self.unit = name, max_depth, background, unit
        self.replicas = replicas or REPLICAS   # x SPP samples per point; a case that needs more than 2^18 says why
        self.b = rtsr.Builder(seed)
        self.objects, self.points, self.conditions, self.extra = [], [], [], {}
        self.cam = self.cfg = self.world = self.flat = None

    def finish(self, rtsr, lookfrom, lookat, vfov=40.0, vup=(0.0, 1.0, 0.0), extra=None, seed=5):
        beside(self, extra)
        self.world = self.b.hittable_list(self.objects)
        self.flat = self.b.flatten(self.world)
        self.cam = rtsr.Camera.new(lookfrom, lookat, vup, vfov, FRAME_WIDTH / FRAME_HEIGHT, 0.0, 10.0, 0.0, 1.0)
        self.cfg = rtsr.Config.new(FRAME_WIDTH / FRAME_HEIGHT, FRAME_WIDTH, FRAME_SPP, FRAME_DEPTH, 4, seed=seed,
                                   background=self.background if any(self.background) else (0.05, 0.05, 0.08))
        return self

    def rays(self, replicas=1):
        """Ray r = replica * n_points + point: every replica of a point has a stream of its own."""
        o = np.ascontiguousarray(np.tile([q.o for q in self.points], (replicas, 1)), dtype=np.float64)
        d = np.ascontiguousarray(np.tile([q.d for q in self.points], (replicas, 1)), dtype=np.float64)
        t = np.ascontiguousarray(np.tile([q.time for q in self.points], replicas), dtype=np.float64)
        return o, d, t


def beside(c, extra):
    """texture_cases._beside: what stands far from every probe ray to take the world to another walker or stack depth."""
    b = c.b
    if extra is None:
        return
    grey = b.lambertian((0.5, 0.5, 0.5))
    if extra == "gravity":
        c.objects.append(b.gravity_sphere((-5000.0, 40.0, -5000.0), 0.0, 1.0, grey))
    elif extra in ("instance", "hoisted"):
        box = b.rect_prism((0.0, -0.413, 0.0), (1.0, 0.587, 1.0), grey)
        members = [b.translate((-5000.0, 0.0, -5000.0), b.rotate_y(15.0, box)), b.translate((-5003.0, 0.0, -5000.0), box)]
        # ("hoisted": the same two members as plain entries of the world list -- the graph the literal restatement, which has no
        # instance trees, can read)
        c.objects += members if extra == "hoisted" else [b.instance_bvh(b.hittable_list(members))]
    elif extra == "bvh":
        rng = np.random.RandomState(4)
        balls = [b.sphere((-5000.0 + 10 * rng.rand(), 10 * rng.rand(), -5000.0 + 10 * rng.rand()), 0.05 + 0.1 * rng.rand(), grey) for _ in range(200)]
        c.objects.append(b.bvh_from_list(b.hittable_list(balls), 0.0, 1.0))
    else:
        raise ValueError(extra)


# ---------------------------------------------------------------------------------------------------- statistics
def counts_of(case, S):
    """(n_points, 3) counts from the per-ray sums of case.rays(case.replicas) -> (counts, every sum is an integer count times
    the unit)."""
    c = np.asarray(S, dtype=np.float64).reshape(case.replicas, len(case.points), 3) / case.unit
    whole = bool(np.all(c == np.round(c)) and np.all(c >= 0) and np.all(c <= SPP))
    return c.sum(axis=0), whole


def rel_se(p, n):
    """The relative standard error the cap is held on: that of the share or of its complement, whichever is larger.  The two are
    ONE statistic (a count and n minus it), the closed form gives both, and the relative error of the rarer one measures how
    rare it is, not how well the count is known: exp(-5) at 2^18 samples is 2.4 % of itself and 0.016 % of what it leaves."""
    q = max(p, 1.0 - p)
    return float(np.sqrt((1.0 - q) / (q * n)))


def check_counts(case, counts, n=None):
    """Every channel of every point against its closed-form share -> (lines to print, failed conditions): within Z_CAP
    standard errors, and rel_se within REL_SE_CAP (a case marked `radiance` reports its share as radiance: the cap is then
    held on the share itself)."""
    lines, failed = [], []
    n = n or getattr(case, "replicas", REPLICAS) * SPP
    for k, q in enumerate(case.points):
        for ch, p in enumerate(q.shares):
            got = counts[k, ch]
            if p == 0.0 or p == 1.0:
                if got != p * n:
                    failed.append("%s %s channel %d: count %d, expected exactly %d" % (case.name, q.tag, ch, got, p * n))
                continue
            se = np.sqrt(p * (1.0 - p) / n)
            z = abs(got / n - p) / se
            rel = se / p if getattr(case, "radiance", False) else rel_se(p, n)
            lines.append("%s %s channel %d: closed form %.6f, judge %.6f, %.2f standard errors, relative SE %.4f" % (case.name, q.tag, ch, p, got / n, z, rel))
            if not z <= Z_CAP or not rel <= REL_SE_CAP:
                failed.append(lines[-1])
    return lines, failed


def host_sums(chk, case, replicas=None, spp=SPP, threads=16, f32=False, flat=None):
    """The host judge's per-ray sums of case.rays(replicas), the rays cut into chunks traced side by side (ray r keeps the
    stream of ray index r: the sums are those of one call)."""
    from concurrent.futures import ThreadPoolExecutor
    import trace_rays_cases as tc
    o, d, t = case.rays(replicas or case.replicas)
    n = len(o)
    S = np.zeros((n, 3))
    cuts = np.linspace(0, n, min(4 * threads, n) + 1).astype(int)

    def part(k):
        lo, hi = cuts[k], cuts[k + 1]
        S[lo:hi], _ = tc.host_trace(chk, flat or case.flat, o[lo:hi], d[lo:hi], t[lo:hi], spp=spp, max_depth=case.max_depth,
                                    background=case.background, seed=SEED, first_ray=int(lo), f32=f32)
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(part, range(len(cuts) - 1)))
    return S


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------- glass
def unit_dir(theta, down, length=1.0):
    """(sin, -+cos, 0) x length as doubles, the sine and cosine taken in longdouble; theta = 0 gives (0, -+1, 0) exactly."""
    th = LD(theta)
    s, c = (LD(0), LD(1)) if theta == 0 else (np.sin(th), np.cos(th))
    return (float(s * LD(length)), float((-c if down else c) * LD(length)), 0.0)


def glass_closed(d, ir, from_above):
    """From the doubles of direction d and index ir, in longdouble: dict of ratio, cos, sin, the reflect share, the margin
    ratio sin - 1, tan of the refracted angle (None when totally reflected)."""
    dx, dy = LD(d[0]), LD(d[1])
    n = np.sqrt(dx * dx + dy * dy)
    sin, cos = abs(dx) / n, abs(dy) / n
    ratio = LD(1) / LD(ir) if from_above else LD(ir)
    r0 = ((LD(1) - ratio) / (LD(1) + ratio)) ** 2
    margin = ratio * sin - LD(1)
    tir = margin > 0
    share = LD(1) if tir else r0 + (LD(1) - r0) * (LD(1) - cos) ** 5
    sin_t = ratio * sin
    tan_t = None if tir else sin_t / np.sqrt(LD(1) - sin_t * sin_t)
    return dict(ratio=ratio, cos=cos, sin=sin, share=float(share), margin=float(margin), tir=bool(tir), tan_i=sin / cos, tan_t=tan_t)


GLASS_ANGLES = (0.0, 5.0, 15.0, 25.0, 35.0, 45.0, 55.0, 65.0, 75.0, 85.0)


def _glass_pane(rtsr, ir=1.5, extra=None):
    """A Dielectric pane at y = 0, green planes at y = +-H and, later in the list, a red strip where each probe's reflected ray
    lands and a blue strip where its refracted ray lands.  Probes from above travel in the plane z = 0, probes from below in
    z = 10 (for ir near 1 a refracted ray from above and a reflected one from below land on the same x).  Angles of GLASS_ANGLES
    degrees, d = (0, -+1, 0) exactly, directions of length 1e-3 and 7 at 30 degrees, and on the side where ratio > 1 the two
    angles 1e-9 rad either side of ratio sin = 1."""
    c = Case("glass_pane ir=%r" % ir, rtsr, 2, GREEN)
    b = c.b
    c.objects.append(b.xz_rect(-BIG, BIG, -BIG, BIG, 0.0, b.dielectric(ir)))
    for y in (H, -H):
        c.objects.append(b.xz_rect(-BIG, BIG, -BIG, BIG, y, b.diffuse_light(GREEN)))
    red, blue = b.diffuse_light(RED), b.diffuse_light(BLUE)
    strips, margins, landing = [], [], []
    for from_above in (True, False):
        z = 0.0 if from_above else 10.0
        ratio = 1.0 / ir if from_above else ir
        probes = [(np.deg2rad(LD(a)), 1.0, "%g deg" % a) for a in GLASS_ANGLES]
        probes += [(np.deg2rad(LD(30.0)), 1e-3, "30 deg |d|=1e-3"), (np.deg2rad(LD(30.0)), 7.0, "30 deg |d|=7")]
        if ratio > 1.0:
            crit = np.arcsin(LD(1) / LD(ratio))
            # (ir = 1.000001 has its critical angle at 89.92 degrees, where 1e-9 rad is a margin of 1.4e-12 and the refracted ray
            # leaves at cos_t = 1.7e-6, which 1 - |r_perp|^2 no longer resolves to the strip's 1e-6: 1e-6 rad there)
            eps = LD(1e-9) if abs(ratio - 1.0) > 1e-3 else LD(1e-6)
            probes += [(crit - eps, 1.0, "%g below the critical angle" % eps), (crit + eps, 1.0, "%g above the critical angle" % eps)]
        for theta, length, tag in probes:
            d = unit_dir(theta, from_above, length)
            u = unit_dir(theta, from_above, 1.0)
            o = (-u[0], -u[1], z)
            g = glass_closed(d, ir, from_above)
            side = 1.0 if from_above else -1.0
            # (mirror rule: back to the side it came from, same angle; Snell: on to the other side at the refracted angle)
            for colour, mat, tan, y in ((0, red, g["tan_i"], side * H), (2, blue, g["tan_t"], -side * H)):
                if tan is None:
                    continue
                x = LD(H) * tan
                flight = LD(H) * np.sqrt(LD(1) + tan * tan)
                w = float(LD(1e-6) * flight)
                c.objects.append(b.xz_rect(float(x) - w, float(x) + w, z - 1.0, z + 1.0, y, mat))
                strips.append((y, z, float(x) - w, float(x) + w, colour))
                landing.append(abs(LD(float(x)) - x) <= LD(1e-9) * flight)
            c.points.append(Point(o, d, (g["share"], 0.0, 1.0 - g["share"]), ("above " if from_above else "below ") + tag))
            if "critical" in tag:
                margins.append((tag, g["margin"], g["share"]))
    c.extra = dict(ir=ir, margins=margins)
    c.conditions.append(("every closed-form landing is within 1e-9 of the flight distance of its strip's centre", all(landing)))
    clash = [(s, t) for i, s in enumerate(strips) for t in strips[i + 1:] if s[:2] == t[:2] and s[2] <= t[3] and t[2] <= s[3] and s[4] != t[4]]
    c.conditions.append(("no strip overlaps one of the other colour", not clash))
    c.conditions.append(("numpy's own ratio sin - 1 exceeds 1e-12 either side of the threshold, with either sign",
                         all(abs(m) > 1e-12 for _, m, _ in margins) and (not margins or {m > 0 for _, m, _ in margins} == {False, True})))
    c.conditions.append(("below the threshold the split is Schlick's, above it every sample reflects (the rule is discontinuous)",
                         all((s == 1.0) == (m > 0) and (m > 0 or s < 0.999) for _, m, s in margins) and (ir != 1.5 or abs(margins[0][2] - 0.041) < 1e-3)))
    if ir == 1.0:
        c.conditions.append(("ir = 1: no ray totally reflects and r0 = 0", not margins and c.points[0].shares[0] == 0.0))
    else:
        c.conditions.append(("one side of the pane has a critical angle", len(margins) == 2))
    return c.finish(rtsr, (-6.0, 1.2, 5.0), (2.0, 0.0, 5.0), 60.0, extra=extra)


# ---------------------------------------------------------------------------------------------------- metal
def absorbed_share(c, f):
    """The share a Metal of fuzz f absorbs at incident cosine c: the cap s_n <= -h of the unit ball, h = c / |f|."""
    if f == 0.0:
        return 0.0
    h = c / abs(min(f, 1.0))  # the builder clamps the fuzz from above only (hit.rs:1063)
    return 0.0 if h >= 1.0 else (1.0 - h) ** 2 * (2.0 + h) / 4.0


def simulate_absorbed(c, f, n, seed):
    """The rule itself in numpy: r + f s with s uniform in the unit ball by rejection, absorbed when the normal component is
    <= 0 -> (share, its standard error)."""
    rng = np.random.RandomState(seed)
    s = rng.uniform(-1.0, 1.0, (int(n * 2.2), 3))
    s = s[(s * s).sum(axis=1) < 1.0][:n]
    assert len(s) == n
    a = (c + f * s[:, 1] <= 0.0).mean()
    p = absorbed_share(c, f)
    return a, np.sqrt(max(p * (1.0 - p), 1e-12) / n)


METAL_ALBEDO = (0.0, 0.5, 0.5)
MIRROR_ANGLES = (0.0, 10.0, 30.0, 50.0, 70.0, 85.0)
FUZZ_POINTS = ((0.1, 1.0), (0.3, 0.5), (0.05, 0.25), (0.5, 1.0), (0.26, 0.25), (0.1, 1.7), (0.1, float("inf")), (0.3, -0.5))


def _metal_mirror(rtsr, edited=False, extra=None):
    """Fuzz 0: a Metal pane of albedo (0, 0.5, 0.5) under a green plane at y = H with one blue strip per probe where the mirror
    rule lands: every sample is 0.5 blue.  edited: built as another metal and set to this one by set_shading."""
    c = Case("metal_mirror", rtsr, 2, GREEN, unit=0.5)
    b = c.b
    metal = b.metal((0.9, 0.1, 0.3), 0.4) if edited else b.metal(METAL_ALBEDO, 0.0)
    c.objects.append(b.xz_rect(-BIG, BIG, -BIG, BIG, 0.0, metal))
    c.objects.append(b.xz_rect(-BIG, BIG, -BIG, BIG, H, b.diffuse_light(GREEN)))
    blue = b.diffuse_light(BLUE)
    probes = [(a, 1.0) for a in MIRROR_ANGLES] + [(40.0, 1e-3), (40.0, 7.0)]
    for a, length in probes:
        theta = np.deg2rad(LD(a))
        d, u = unit_dir(theta, True, length), unit_dir(theta, True, 1.0)
        g = glass_closed(d, 1.5, True)
        x = float(LD(H) * g["tan_i"])
        w = float(LD(1e-6) * LD(H) * np.sqrt(LD(1) + g["tan_i"] ** 2))
        c.objects.append(b.xz_rect(x - w, x + w, -1.0, 1.0, H, blue))
        c.points.append(Point((-u[0], -u[1], 0.0), d, (0.0, 0.0, 1.0), "%g deg |d|=%g" % (a, length)))
    c.extra = dict(metal=metal, edit=("metal", metal, METAL_ALBEDO, 0.0))
    c.conditions.append(("the probes differ in angle", len({q.d for q in c.points}) == len(c.points)))
    c.finish(rtsr, (-6.0, 1.2, 0.0), (2.0, 0.0, 0.0), 60.0, extra=extra)
    if edited:
        c.flat.set_shading([c.extra["edit"]])
    return c


def _metal_fuzz(rtsr, edited=False, extra=None):
    """One Metal pane per (incident cosine, fuzz) of FUZZ_POINTS, 10 apart in z, under a blue sky: a survivor leaves upwards and
    is 0.5 blue, an absorbed sample is black.  Fuzz 1.7 and +inf are stored as 1, fuzz -0.5 as it is."""
    c = Case("metal_fuzz", rtsr, 2, BLUE, unit=0.5)
    b = c.b
    mats, edits = [], []
    for k, (cos, f) in enumerate(FUZZ_POINTS):
        m = b.metal((0.2, 0.2, 0.2), 0.125) if edited else b.metal(METAL_ALBEDO, f)
        mats.append(m)
        # (an edit must be finite -- include/rtx_abi.h, rtx_flat_set_shading; the builder takes +inf: 1e300 stands in for it)
        edits.append(("metal", m, METAL_ALBEDO, f if np.isfinite(f) else 1e300))
        z = 10.0 * k
        c.objects.append(b.xz_rect(-1.0, 1.0, z - 1.0, z + 1.0, 0.0, m))
        d = (float(np.sqrt(LD(1) - LD(cos) ** 2)), -cos, 0.0)
        c.points.append(Point((-d[0], -d[1], z), d, (0.0, 0.0, 1.0 - absorbed_share(cos, f)), "cos %g fuzz %g" % (cos, f)))
    c.extra = dict(mats=mats)
    c.finish(rtsr, (-3.0, 2.0, 35.0), (0.0, 0.0, 35.0), 90.0, extra=extra)
    if edited:
        c.flat.set_shading(edits)
    stored = [c.flat.material(m)["param"] for m in mats]
    want = [min(f, 1.0) for _, f in FUZZ_POINTS]
    c.conditions.append(("fuzz is clamped from above only: 1.7 and +inf are stored as 1, -0.5 as -0.5", stored == want and want[5] == want[6] == 1.0 and want[7] == -0.5))
    c.conditions.append(("a fuzz sphere that cannot reach the surface absorbs nothing", absorbed_share(0.26, 0.25) == 0.0 and c.points[4].shares[2] == 1.0))
    return c


# ---------------------------------------------------------------------------------------------------- media
LANE = 100.0   # lanes of a media world are this far apart in z
WALL_X = 60.0
ODS = (0.05, 0.5, 1.0, 2.0, 5.0)


def box_mesh(lo, hi):
    """A closed box of 12 triangles (vertices, faces), each face cut along one diagonal."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    v = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    f = [(0, 1, 2), (0, 2, 3), (4, 6, 5), (4, 7, 6), (0, 4, 5), (0, 5, 1), (3, 2, 6), (3, 6, 7), (0, 3, 7), (0, 7, 4), (1, 5, 6), (1, 6, 2)]
    return np.array(v, dtype=np.float64), np.array(f, dtype=np.int64)


def ball_chord(radius, offset):
    return 2.0 * float(np.sqrt(LD(radius) ** 2 - LD(offset) ** 2))


def _transmit(c, o, d, density, length, tag, time=0.0, inside=False):
    """length: the Euclidean chord ahead of the origin; inside: the origin lies in the medium, whose first 0.001 of t (0.001 |d|
    of length) is exempt: t1 = max(rec1.t, t_min)."""
    if inside:
        length = LD(length) - LD(0.001) * np.sqrt(sum(LD(x) ** 2 for x in d))
    c.points.append(Point(o, d, (0.0, 0.0, float(np.exp(-LD(density) * LD(length)))), tag, time=time))


def _media_sphere(rtsr, slab=False, extra=None):
    """Media bounded by ONE plain static sphere each (the flat scene has F_MEDIUM_SPHERE and not F_MEDIUM_GENERAL: the fused
    sphere block of k_trace_world), max_depth = 1, a blue wall behind (x = WALL_X), a green background.  Lane k (z = 100 k)
    holds a ball of radius 2 whose optical depth through the centre is ODS[k]; lane 2 is also crossed off centre, with
    directions of length 1e-3 and 40, and from its centre (rec1.t < 0).  Lane 5: rays from the centre of a ball towards -x
    meet a small blue sphere inside it after s = 0.2 .. 1.7 (the far side of the boundary is hidden: exp(-density (s - 0.001)));
    lane 6 is lane 5 with the blue spheres listed before the medium."""
    c = Case("media_sphere", rtsr, 1, GREEN)
    b = c.b
    skin = b.lambertian((0.5, 0.5, 0.5))
    c.objects.append(b.yz_rect(-50.0, 50.0, -LANE, 8 * LANE, WALL_X, b.diffuse_light(BLUE)))
    for k, od in enumerate(ODS):
        z, rho = LANE * k, od / 4.0
        c.objects.append(b.constant_medium(WHITE, rho, b.sphere((0.0, 0.0, z), 2.0, skin)))
        _transmit(c, (-20.0, 0.0, z), (1.0, 0.0, 0.0), rho, 4.0, "ball od %g" % od)
        if k == 2:
            _transmit(c, (-20.0, 1.2, z), (1.0, 0.0, 0.0), rho, ball_chord(2.0, 1.2), "ball off centre")
            _transmit(c, (-20.0, 0.0, z), (1e-3, 0.0, 0.0), rho, 4.0, "ball |d|=1e-3")
            _transmit(c, (-20.0, 0.0, z), (40.0, 0.0, 0.0), rho, 4.0, "ball |d|=40")
            _transmit(c, (0.0, 0.0, z), (1.0, 0.0, 0.0), rho, 2.0, "ball from its centre", inside=True)
            _transmit(c, (0.0, 0.0, z), (40.0, 0.0, 0.0), rho, 2.0, "ball from its centre |d|=40", inside=True)
    blue = b.diffuse_light(BLUE)
    for lane, surfaces_first in ((5, False), (6, True)):
        z, rho = LANE * lane, 0.9
        fog = b.constant_medium(WHITE, rho, b.sphere((0.0, 0.0, z), 2.0, skin))
        if not surfaces_first:
            c.objects.append(fog)
        for k, s in enumerate((0.2, 0.5, 0.9, 1.3, 1.7)):
            a = np.deg2rad(LD(20.0 * (k - 2)))
            u = (-float(np.cos(a)), float(np.sin(a)), 0.0)
            r = 0.05
            c.objects.append(b.sphere((u[0] * (s + r), u[1] * (s + r), z), r, blue))
            _transmit(c, (0.0, 0.0, z), u, rho, s, "surface inside at %g, listed %s the medium" % (s, "before" if surfaces_first else "after"), inside=True)
        if surfaces_first:
            c.objects.append(fog)
    if slab:   # a general medium beside the sphere media: the world has both feature bits
        z = LANE * 7
        c.objects.append(b.constant_medium(WHITE, 0.7, b.rect_prism((-0.5, -5.0, z - 5.0), (0.5, 5.0, z + 5.0), skin)))
        _transmit(c, (-20.0, 0.25, z + 0.125), (1.0, 0.0, 0.0), 0.7, 1.0, "slab beside the balls")
    c.conditions.append(("optical depths span 0.05 .. 5", (min(ODS), max(ODS)) == (0.05, 5.0)))
    return c.finish(rtsr, (-9.0, 1.0, 2.2 * LANE), (0.0, 0.0, 2.0 * LANE), 40.0, extra=extra)


def _media_general(rtsr, extra=None):
    """Media whose boundary is anything but one plain sphere (F_MEDIUM_GENERAL and not F_MEDIUM_SPHERE): lane 0 a slab
    (rect_prism, thickness 1), crossed obliquely, with three direction lengths, and from inside; lane 1 a ball under a
    translate; lane 2 a moving_sphere ball at ray times 0.25 and 0.75 (the centre, and with it the chord, moves); lane 3 a
    closed box of 12 triangles under bvh_from_list (the two-phase walk).  Two densities on the slab."""
    c = Case("media_general", rtsr, 1, GREEN)
    b = c.b
    skin = b.lambertian((0.5, 0.5, 0.5))
    c.objects.append(b.yz_rect(-50.0, 50.0, -LANE, 8 * LANE, WALL_X, b.diffuse_light(BLUE)))
    for k, rho in enumerate((0.5, 2.0)):
        z = -30.0 + 60.0 * k
        c.objects.append(b.constant_medium(WHITE, rho, b.rect_prism((-0.5, -5.0, z - 5.0), (0.5, 5.0, z + 5.0), skin)))
        _transmit(c, (-20.0, 0.25, z), (1.0, 0.0, 0.0), rho, 1.0, "slab density %g" % rho)
        slant = float(np.sqrt(LD(1) + LD(0.3) ** 2))
        for length in (1e-3, 1.0, 40.0):
            _transmit(c, (-10.0, -3.0, z + 0.125), (length, 0.3 * length, 0.0), rho, slant, "slab oblique |d|=%g" % length)
        _transmit(c, (0.25, 0.3, z + 0.125), (1.0, 0.0, 0.0), rho, 0.25, "slab from inside", inside=True)
        _transmit(c, (0.25, 0.3, z + 0.125), (40.0, 0.0, 0.0), rho, 0.25, "slab from inside |d|=40", inside=True)
    z = LANE
    c.objects.append(b.constant_medium(WHITE, 0.4, b.translate((0.0, 0.0, z), b.sphere((0.0, 0.0, 0.0), 2.0, skin))))
    _transmit(c, (-20.0, 0.0, z), (1.0, 0.0, 0.0), 0.4, 4.0, "translated ball")
    _transmit(c, (-20.0, 1.2, z), (40.0, 0.0, 0.0), 0.4, ball_chord(2.0, 1.2), "translated ball off centre |d|=40")
    z = 2 * LANE
    c.objects.append(b.constant_medium(WHITE, 0.6, b.moving_sphere((0.0, -1.0, z), (0.0, 1.0, z), 0.0, 1.0, 2.0, skin)))
    for time in (0.25, 0.75):
        cy = -1.0 + 2.0 * time
        _transmit(c, (-20.0, 1.25, z), (1.0, 0.0, 0.0), 0.6, ball_chord(2.0, 1.25 - cy), "moving ball at time %g" % time, time=time)
    z = 3 * LANE
    v, f = box_mesh((-1.0, -2.0, z - 2.0), (0.5, 2.0, z + 2.0))
    c.objects.append(b.constant_medium(WHITE, 0.8, b.bvh_from_list(b.triangle_mesh(v, f, skin), 0.0, 1.0)))
    _transmit(c, (-20.0, 0.3, z + 0.9), (1.0, 0.0, 0.0), 0.8, 1.5, "mesh box")
    _transmit(c, (-20.0, 0.3, z + 0.9), (40.0, 0.0, 0.0), 0.8, 1.5, "mesh box |d|=40")
    _transmit(c, (0.0, 0.3, z + 0.9), (1.0, 0.0, 0.0), 0.8, 0.5, "mesh box from inside", inside=True)
    c.conditions.append(("the two chords of the moving ball differ", c.points[-5].shares != c.points[-4].shares))
    return c.finish(rtsr, (-12.0, 2.0, 1.6 * LANE), (0.0, 0.0, 1.5 * LANE), 60.0, extra=extra)


def _surface_in_front(rtsr, medium=True, after=False, ball=True, extra=None):
    """A white Lambertian wall (x = -5, facing -x) wholly in front of a medium (a ball or a slab at x >= -2), max_depth = 2: the
    scattered ray lands on a red (y >= 0) or a blue (y < 0) emitter at x = -12, so the colour of a sample tells the stream.
    With the wall listed BEFORE the medium the medium sees t1 >= t2 and must not draw: every sample equals that of the world
    without the medium (medium=False).  Listed AFTER it the medium draws first, the wall still wins every ray."""
    c = Case("surface_in_front", rtsr, 2, GREEN)
    b = c.b
    wall = b.yz_rect(-50.0, 50.0, -50.0, 50.0, -5.0, b.lambertian(WHITE))
    skin = b.lambertian((0.5, 0.5, 0.5))
    fog = None
    if medium:
        boundary = b.sphere((0.0, 0.0, 0.0), 2.0, skin) if ball else b.rect_prism((-2.0, -9.0, -9.0), (2.0, 9.0, 9.0), skin)
        fog = b.constant_medium(WHITE, 0.7, boundary)
    c.objects += [b.yz_rect(0.0, 1.0e4, -1.0e4, 1.0e4, -12.0, b.diffuse_light(RED)), b.yz_rect(-1.0e4, 0.0, -1.0e4, 1.0e4, -12.0, b.diffuse_light(BLUE))]
    c.objects += ([fog, wall] if after else [wall, fog]) if medium else [wall]
    rng = np.random.RandomState(21)
    for k in range(16):
        y, z = rng.uniform(-1.0, 1.0, 2)
        c.points.append(Point((-8.0, y, z), (1.0, 0.1 * y, 0.1 * z), (), "wall ray %d" % k))  # (no closed form: bit comparisons only)
    return c.finish(rtsr, (-11.0, 0.5, 6.0), (0.0, 0.0, 0.0), 50.0, extra=extra)


# ---------------------------------------------------------------------------------------------------- the Isotropic phase
SLAB_ORDER = 64   # Gauss-Legendre nodes per axis: orders 64 and 128 agree to 1e-7 (slab_order() redoes that)


def slab_value(order, density=2.0):
    """The share of samples that scatter in their first flight straight down through a slab of unit thickness and then leave
    upward unscattered: Gauss-Legendre over the scatter depth x (density exp(-density x)), the direction cosine mu of the
    second flight (uniform on the sphere: 1 / 2 on [-1, 1], only mu > 0 leaves upward) and the length r = |s| of the
    un-normalised sphere sample (3 r^2).  The second flight starts IN the medium: its first 0.001 of t -- 0.001 r of length,
    since Isotropic leaves the direction un-normalised -- is exempt, so it crosses max(x / mu - 0.001 r, 0)."""
    x, w = np.polynomial.legendre.leggauss(order)
    x, w = 0.5 * (x + 1.0), 0.5 * w
    X, M, R = np.meshgrid(x, x, x, indexing="ij")
    W = w[:, None, None] * w[None, :, None] * w[None, None, :]
    f = density * np.exp(-density * X) * 0.5 * 3.0 * R * R * np.exp(-density * np.maximum(X / M - 0.001 * R, 0.0))
    return float((W * f).sum())


def slab_order(tol=1e-7):
    """The first order, doubling from 8, whose value differs from the doubled order's by less than tol relative."""
    order, prev = 8, slab_value(8)
    while True:
        nxt = slab_value(2 * order)
        if abs(nxt - prev) <= tol * abs(nxt):
            return order
        order, prev = 2 * order, nxt


def _isotropic_slab(rtsr, extra=None):
    """A slab medium y in [0, 1] of density 2 (optical depth 2) and albedo (0, 0, 1) under a blue sky (the half-space emitter:
    the background), a black emitter below, max_depth = 2, rays straight down from y = 5: a sample is blue when it scatters in
    the first flight and its second flight leaves upward unscattered (slab_value), else black.  The value is reported as
    radiance (albedo x Le x the share): REL_SE_CAP is held on the share itself, which takes 2^20 samples."""
    c = Case("isotropic_slab", rtsr, 2, BLUE, replicas=4 * REPLICAS)
    c.radiance = True
    b = c.b
    c.objects.append(b.constant_medium(BLUE, 2.0, b.rect_prism((-BIG, 0.0, -BIG), (BIG, 1.0, BIG), b.lambertian((0.5, 0.5, 0.5)))))
    c.objects.append(b.xz_rect(-BIG, BIG, -BIG, BIG, -1.0, b.diffuse_light(BLACK)))
    v = slab_value(SLAB_ORDER)
    for k, length in enumerate((1.0, 1e-3, 40.0)):
        c.points.append(Point((0.5 * k, 5.0, 0.25), (0.0, -length, 0.0), (0.0, 0.0, v), "straight down |d|=%g" % length))
    c.conditions.append(("the 0.001 |s| of the second flight is in the value: it is e^(0.002 E|s|) = e^0.0015 above the value without it",
                         abs(v / 0.15230586 - np.exp(0.0015)) < 2e-5))
    return c.finish(rtsr, (0.0, 4.0, 9.0), (0.0, 0.5, 0.0), 40.0, extra=extra)


# ---------------------------------------------------------------------------------------------------- casts
class CastSet:
    """n rays (o, d, time 0) through one slab medium [x0, x1] of a casts world under (t_min, t_max), ray r on the stream of
    seed + r; density and the closed-form verdict: "never", "at_t1", "restated" (medium_hit_restated decides every ray)."""

    def __init__(self, tag, slot, density, x0, x1, ox, dx, lane, t_min=0.001, t_max=float("inf"), n=256, verdict="restated", share=None):
        self.tag, self.slot, self.density, self.x0, self.x1, self.ox, self.dx, self.lane = tag, slot, density, x0, x1, ox, dx, lane
        self.t_min, self.t_max, self.n, self.verdict, self.share = t_min, t_max, n, verdict, share
        self.first = 0   # first ray of the set in the case's batch: its stream is seed + first + r

    def rays(self):
        o = np.tile([self.ox, 0.25, self.lane + 0.125], (self.n, 1)).astype(np.float64)
        d = np.tile([self.dx, 0.0, 0.0], (self.n, 1)).astype(np.float64)
        return np.ascontiguousarray(o), np.ascontiguousarray(d)


def first_uniforms(orc, seed, n):
    """The first uniform of the streams seed .. seed + n - 1 (pixel 0, sample 0): what a cast's medium draws."""
    import ctypes as C
    lib = orc.load()
    out = np.zeros(n)
    one = (C.c_double * 1)()
    for r in range(n):
        lib.oracle_sample_stream(seed + r, 0, 0, 1, one)
        out[r] = one[0]
    return out


def medium_hit_restated(orc, cs, u):
    """hit.rs:955-986 for the slab of a CastSet in float64, operation by operation, from the rays' first uniforms u ->
    (hit (n,) bool, t (n,), t1 (n,), t2 (n,)).  The slab is entered through the yz rectangle at x0 or x1: t = (k - o.x) / d.x.
    The logarithm is the project's rt_log."""
    f = np.float64
    with np.errstate(all="ignore"):
        n = len(u)
        ta, tb = (f(cs.x0) - f(cs.ox)) / f(cs.dx), (f(cs.x1) - f(cs.ox)) / f(cs.dx)
        rec1, rec2 = min(ta, tb), max(ta, tb)
        ok = rec2 >= rec1 + f(0.0001)            # the second query starts at rec1.t + 0.0001
        t1, t2 = max(rec1, f(cs.t_min)), min(rec2, f(cs.t_max))
        ok = ok and not t1 >= t2
        t1c = f(0.0) if t1 < 0 else t1
        length = np.sqrt(f(cs.dx) * f(cs.dx) + f(0.0) + f(0.0))
        inside = (t2 - t1c) * length
        neg_inv = f(-1.0) / f(cs.density)
        dist = neg_inv * orc.rt_math("log", u)
        hit = np.full(n, bool(ok)) & ~(dist > inside)
        t = t1c + dist / length
    return hit, np.where(hit, t, np.inf), np.full(n, t1c), np.full(n, t2)


def _casts(rtsr, extra=None):
    """Slab media of every density and chord the casts hold, one per lane (z = 100 k), each a rect_prism from x0 to x1, 10 x 10
    across.  See CastSet; the sets are built in the order of the slabs."""
    c = Case("casts", rtsr, 1, GREEN)
    b = c.b
    skin = b.lambertian((0.5, 0.5, 0.5))
    inf = float("inf")
    plan = [
        # tag, density, x0, x1, ox, dx, t_min, t_max, n, verdict, share of rays that hit (None: not a statistic)
        ("chord 0.00009 by geometry", 1.0e4, 0.0, 0.00009, -1.0, 1.0, 0.001, inf, 256, "never", None),
        ("chord 0.00009 by geometry, density inf", inf, 0.0, 0.00009, -1.0, 1.0, 0.001, inf, 64, "never", None),
        ("chord 0.00011 by geometry", 1.0e4, 0.0, 0.00011, -1.0, 1.0, 0.001, inf, 1 << 16, "restated", 1.0 - np.exp(-1.0e4 * 0.00011)),
        ("chord 0.00009 by |d| = 1000", 10.0, 0.0, 0.09, -1.0, 1000.0, 0.00001, inf, 256, "never", None),
        ("chord 0.00011 by |d| = 1000", 10.0, 0.0, 0.11, -1.0, 1000.0, 0.00001, inf, 1 << 16, "restated", 1.0 - np.exp(-10.0 * 0.11)),
        ("chord 0.09 at |d| = 1e-3: 90 in t", 10.0, 0.0, 0.09, -1.0, 1e-3, 0.001, inf, 1 << 16, "restated", 1.0 - np.exp(-10.0 * 0.09)),
        ("negative t_min, origin inside", 1.5, -1.0, 1.0, 0.5, 1.0, -5.0, inf, 1 << 16, "restated", 1.0 - np.exp(-1.5 * 0.5)),
        ("t_min inside the slab", 1.5, -1.0, 1.0, -3.0, 1.0, 2.5, inf, 1 << 16, "restated", 1.0 - np.exp(-1.5 * 1.5)),
        ("t_max inside the slab", 1.5, -1.0, 1.0, -3.0, 1.0, 0.001, 2.75, 1 << 16, "restated", 1.0 - np.exp(-1.5 * 0.75)),
        ("t_max before the slab", 1.5, -1.0, 1.0, -3.0, 1.0, 0.001, 1.5, 256, "never", None),
        ("density 0", 0.0, -1.0, 1.0, -3.0, 1.0, 0.001, inf, 1024, "never", None),
        ("density 1e-300", 1e-300, -1.0, 1.0, -3.0, 1.0, 0.001, inf, 1024, "never", None),
        ("density inf", inf, -1.0, 1.0, -3.0, 1.0, 0.001, inf, 1024, "at_t1", None),
        ("density 1e300", 1e300, -1.0, 1.0, -3.0, 1.0, 0.001, inf, 1024, "at_t1", None),
        ("density -1", -1.0, -1.0, 1.0, -3.0, 1.0, 0.001, inf, 1024, "restated", None),
        ("16 bins", 1.25, -1.0, 1.0, -3.0, 1.0, 0.001, inf, 1 << 16, "restated", 1.0 - np.exp(-1.25 * 2.0)),
    ]
    slabs, sets = {}, []
    for tag, density, x0, x1, ox, dx, t_min, t_max, n, verdict, share in plan:
        key = (density, x0, x1)
        if key not in slabs:
            lane = LANE * len(slabs)
            slabs[key] = (len(c.objects), lane)
            c.objects.append(b.constant_medium(WHITE, density, b.rect_prism((x0, -5.0, lane - 5.0), (x1, 5.0, lane + 5.0), skin)))
        slot, lane = slabs[key]
        sets.append(CastSet(tag, slot, density, x0, x1, ox, dx, lane, t_min, t_max, n, verdict, None if share is None else float(share)))
    first = 0
    for cs in sets:
        cs.first, first = first, first + cs.n
    c.extra = dict(sets=sets)
    # (for rays(): bit comparisons only)
    c.points.append(Point((-3.0, 0.25, 0.125), (1.0, 0.0, 0.0), (), "through the first slab"))
    c.points.append(Point((-3.0, 0.25, sets[6].lane + 0.125), (1.0, 0.0, 0.0), (), "through the slab of density 1.5"))
    c.points.append(Point((-3.0, 0.25, sets[14].lane + 0.125), (1.0, 0.0, 0.0), (), "through the slab of density -1"))
    return c.finish(rtsr, (-14.0, 3.0, 4.5 * LANE), (0.0, 0.0, 4.0 * LANE), 70.0, extra=extra)


def cast_records(orc, case, sets=None, seed=SEED):
    """core_world_hit of every ray of the sets, one call each -> {tag: (hit (n,) bool, t (n,))}."""
    out = {}
    ptr = case.flat.arrays_ptr()
    for cs in sets if sets is not None else case.extra["sets"]:
        o, d = cs.rays()
        hit, t = np.zeros(cs.n, dtype=bool), np.full(cs.n, np.inf)
        for r in range(cs.n):
            rec = orc.core_world_hit(ptr, o[r], d[r], 0.0, cs.t_min, cs.t_max, rng_seed=seed + cs.first + r)
            if rec is not None:
                hit[r], t[r] = True, rec["t"]
        out[cs.tag] = (hit, t)
    return out


def truncated_bins(t, t1, t2, rate, n_bins=16):
    """The bin 0 .. n_bins - 1 of every hit distance under the exponential of `rate` (per unit t) truncated to [t1, t2]: bins of
    equal probability (the cdf cut into n_bins)."""
    x = (np.asarray(t, dtype=LD) - LD(t1)) * LD(rate)
    cdf = (LD(1) - np.exp(-x)) / (LD(1) - np.exp(-LD(rate) * (LD(t2) - LD(t1))))
    return np.minimum((cdf * n_bins).astype(np.int64), n_bins - 1)


# ---------------------------------------------------------------------------------------------------- two media
def two_media_shares(rho_a, a1, a2, rho_b, b1, b2):
    """Who scatters a ray first under the reference's rule when medium A (the EARLIER slot, [a1, a2] along a unit ray) and
    medium B ([b1, b2], a1 < b1 < a2 < b2) overlap -> (share A, share B, share neither).  A draws first and, when it hits at x,
    leaves B the interval [b1, min(b2, x)]: B skips its draw when x <= b1, else B hits (and wins: it is closer) with
    1 - exp(-rho_b (x - b1)).  When A misses, B has all of [b1, b2]."""
    ra, rb = LD(rho_a), LD(rho_b)
    a1, a2, b1, b2 = LD(a1), LD(a2), LD(b1), LD(b2)
    assert a1 < b1 < a2 < b2
    miss_a = np.exp(-ra * (a2 - a1))
    a_before_b = LD(1) - np.exp(-ra * (b1 - a1))
    # A hits at x in (b1, a2]: density ra exp(-ra (x - a1)); B then hits with 1 - exp(-rb (x - b1))
    a_in_overlap = np.exp(-ra * (b1 - a1)) - miss_a
    both = ra * np.exp(-ra * (b1 - a1)) * (LD(1) - np.exp(-(ra + rb) * (a2 - b1))) / (ra + rb)   # A hits in the overlap and B does NOT
    share_b = miss_a * (LD(1) - np.exp(-rb * (b2 - b1))) + (a_in_overlap - both)
    share_a = a_before_b + both
    return float(share_a), float(share_b), float(LD(1) - share_a - share_b)


def later_first_shares(rho_a, a1, a2, rho_b, b1, b2):
    """The same two media with B the EARLIER slot: B draws over all of [b1, b2]; A then has [a1, min(a2, B's hit)] -- B's hit
    lies behind b1 > a1, so A always draws -- and wins when it hits."""
    ra, rb = LD(rho_a), LD(rho_b)
    a1, a2, b1, b2 = LD(a1), LD(a2), LD(b1), LD(b2)
    miss_b = np.exp(-rb * (b2 - b1))
    # B hits at x in [b1, b2] with density rb exp(-rb (x - b1)); A hits within min(a2, x) - a1
    # x in [b1, a2]: A hits with 1 - exp(-ra (x - a1)); x in (a2, b2]: with 1 - exp(-ra (a2 - a1))
    full_a = LD(1) - np.exp(-ra * (a2 - a1))
    b_near = LD(1) - np.exp(-rb * (a2 - b1))
    a_miss_and_b_near = rb * np.exp(-ra * (b1 - a1)) * (LD(1) - np.exp(-(ra + rb) * (a2 - b1))) / (ra + rb)
    share_a = miss_b * full_a + (b_near - a_miss_and_b_near) + (LD(1) - miss_b - b_near) * full_a
    share_b = a_miss_and_b_near + (LD(1) - miss_b - b_near) * (LD(1) - full_a)
    return float(share_a), float(share_b), float(LD(1) - share_a - share_b)


TWO = dict(rho_a=0.6, ca=0.0, ra=2.0, rho_b=0.9, cb=2.5, rb=1.5)   # ball A at x = 0 (radius 2), ball B at x = 2.5 (radius 1.5)


def _two_media(rtsr, b_first=False, extra=None):
    """Two overlapping balls of different density and colour on the x axis, A = [-2, 2] and B = [1, 4]; the rays run along the
    axis from x = -6.  Who scatters first is read from a cast's ids (the material of the hit), in either list order."""
    c = Case("two_media", rtsr, 2, BLACK)
    b = c.b
    skin = b.lambertian((0.5, 0.5, 0.5))
    fa = b.constant_medium(RED, TWO["rho_a"], b.sphere((TWO["ca"], 0.0, 0.0), TWO["ra"], skin))
    fb = b.constant_medium(BLUE, TWO["rho_b"], b.sphere((TWO["cb"], 0.0, 0.0), TWO["rb"], skin))
    c.objects += [fb, fa] if b_first else [fa, fb]
    c.extra = dict(slot_a=1 if b_first else 0, slot_b=0 if b_first else 1, interval_a=(4.0, 8.0), interval_b=(7.0, 10.0))
    c.points.append(Point((-6.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 0.0), "along the axis"))
    c.points.append(Point((-6.0, 0.4, 0.3), (1.0, -0.02, 0.01), (0.0, 0.0, 0.0), "beside the axis"))
    return c.finish(rtsr, (-7.0, 1.0, 4.0), (1.0, 0.0, 0.0), 50.0, extra=extra)


# ---------------------------------------------------------------------------------------------------- pairs
PAIR_KINDS = ("same", "last_bit", "negative_radius", "slot_between", "second_behind", "medium_first")


def _pair(rtsr, kind="same", extra=None):
    """Book-2's ball-in-ball pattern: a glass ball (radius 2 at the origin) and a medium bounded by a sphere of its own, next
    in the list, with a small blue sphere at the centre (a surface inside the medium) and a red wall far behind the probe's
    origin (what a reflected sample sees), max_depth = 2.
      same             the medium's sphere equals the ball bit for bit: the device pairs them (WD_PAIR)
      last_bit         its radius is the next double: no pair
      negative_radius  its radius is -2: no pair (the same surface, normals turned)
      slot_between     another object between the two: no pair
      second_behind    a second medium, in a larger sphere, behind the pair in the list
      medium_first     the medium before the ball: no pair (the rule is about order)
    A probe along the axis meets the glass first (the medium sees t1 >= t2: no draw), reflects with r0 to the red wall, else
    refracts straight on and flies s = 1.9 to the blue sphere: the medium starts at t_min = 0.001 behind the boundary the
    ray starts ON, so the blue share is (1 - r0) exp(-density (s - 0.001)); with the second medium behind, times its
    exp(-density2 (s - 0.001)) as well."""
    c = Case("pair " + kind, rtsr, 2, GREEN)
    b = c.b
    glass = b.dielectric(1.5)
    rho, rho2, s = 0.5, 0.3, 1.9
    radius = {"last_bit": float(np.nextafter(2.0, 3.0)), "negative_radius": -2.0}.get(kind, 2.0)
    ball = b.sphere((0.0, 0.0, 0.0), 2.0, glass)
    # (media of albedo 0: a sample that scatters in one contributes nothing, wherever its second flight ends)
    fog = b.constant_medium(BLACK, rho, b.sphere((0.0, 0.0, 0.0), radius, glass))
    c.objects.append(b.yz_rect(-1.0e4, 1.0e4, -1.0e4, 1.0e4, -12.0, b.diffuse_light(RED)))
    c.objects.append(b.sphere((0.0, 0.0, 0.0), 0.1, b.diffuse_light(BLUE)))
    if kind == "medium_first":
        c.objects += [fog, ball]
    elif kind == "slot_between":
        c.objects += [ball, b.sphere((0.0, 30.0, 0.0), 1.0, b.metal((0.5, 0.5, 0.5), 0.0)), fog]
    else:
        c.objects += [ball, fog]
    if kind == "second_behind":
        c.objects.append(b.constant_medium(BLACK, rho2, b.sphere((0.0, 0.0, 0.0), 3.0, glass)))
    r0 = ((LD(1) - LD(1) / LD(1.5)) / (LD(1) + LD(1) / LD(1.5))) ** 2
    inside = np.exp(-LD(rho) * (LD(s) - LD(0.001)))
    for length in (1.0, 40.0):
        if kind == "second_behind":
            # the probe starts at x = -2.5, inside the outer medium (radius 3): 0.5 to the glass less the 0.001 |d| it is exempt
            # from; inside the ball both media draw over s - 0.001 (the refracted direction is a unit vector); a reflected
            # sample starts ON the ball, leaves the pair's medium without a draw (t1 >= t2) and has 1 - 0.001 of the outer one
            way_in = np.exp(-LD(rho2) * (LD(0.5) - LD(0.001) * LD(length)))
            shares = (float(way_in * r0 * np.exp(-LD(rho2) * (LD(1) - LD(0.001)))), 0.0,
                      float(way_in * (LD(1) - r0) * inside * np.exp(-LD(rho2) * (LD(s) - LD(0.001)))))
            o = (-2.5, 0.0, 0.0)
        else:
            shares = (float(r0), 0.0, float((LD(1) - r0) * inside))
            o = (-6.0, 0.0, 0.0)
        c.points.append(Point(o, (length, 0.0, 0.0), shares, "axis |d|=%g" % length))
    c.extra.update(kind=kind, pairs=kind in ("same", "second_behind"))
    # the camera sits ON the ball's boundary: the lanes of one wave split between rays that start inside, outside, culled and paired
    return c.finish(rtsr, (0.0, 2.0, 0.0), (3.0, 0.5, 1.0), 100.0, extra=extra)


# ---------------------------------------------------------------------------------------------------- the sphere walkers
def shell_back_share(ir):
    """A ray on the axis of a hollow shell meets four interfaces at normal incidence, each reflecting with r0 and passing with
    1 - r0 (r0 is the same from either side).  f(region, direction) = the share that leaves through the back, regions 0 (in
    front) .. 4 (behind): f(i, +) = (1 - r0) f(i + 1, +) + r0 f(i, -), f(i, -) = (1 - r0) f(i - 1, -) + r0 f(i, +), f(4, +) = 1,
    f(0, -) = 0 -- eight unknowns, solved here; the answer is (1 - r0) / (1 + 3 r0), which the CPU test also asserts.
    Truncation at max_depth 50: a path still inside after n interface events has reflected at least (n - 3) / 4 times (no more
    than three passages lie between two reflections), so what 49 events cut off is below C(49, 12) r0^12 < 2e-6 of the
    samples, a 400th of a standard error."""
    r0 = float(((LD(1) - LD(ir)) / (LD(1) + LD(ir))) ** 2)
    idx = {}
    for i in range(5):
        for s in (+1, -1):
            idx[(i, s)] = len(idx)
    A, rhs = np.zeros((10, 10)), np.zeros(10)
    for (i, s), k in idx.items():
        A[k, k] = 1.0
        if (i, s) == (4, +1):
            rhs[k] = 1.0
        elif (i, s) == (0, -1) or (i, s) == (4, -1):
            rhs[k] = 0.0   # (4, -) is never entered
        else:
            A[k, idx[(i + s, s)]] -= 1.0 - r0
            A[k, idx[(i, -s)]] -= r0
    return float(np.linalg.solve(A, rhs)[idx[(0, +1)]])


def _glass_balls(rtsr, extra=None):
    """ONE BVH of 40 spheres, so that k_trace_lds, k_trace_vote and k_wf_trace take it: glass of every index of IRS, a hollow
    shell (radius 1 around radius -0.9), metals of fuzz 0 / 0.3 / 1.7, Lambertian over a solid colour and over a checker,
    under a sky.  The probes run along the shell's axis (y = 3.5, towards +x, nothing else on that line but a black Lambertian
    sphere behind their origin): every interface is met at normal incidence, where reflect and refract are exact, so the path
    stays on the axis and what leaves through the back into the blue sky is shell_back_share."""
    c = Case("glass_balls", rtsr, 50, BLUE)
    b = c.b
    mats = [b.dielectric(ir) for ir in IRS] + [b.metal((0.8, 0.8, 0.7), f) for f in (0.0, 0.3, 1.7)] + \
           [b.lambertian((0.7, 0.3, 0.2)), b.lambertian(b.checker_from_colors((0.9, 0.9, 0.1), (0.1, 0.2, 0.7)))]
    balls = []
    for n in range(36):
        balls.append(b.sphere((2.2 * (n % 9) - 8.8, 1.0, 2.2 * (n // 9) - 3.3), 1.0, mats[n % len(mats)]))
    balls.append(b.sphere((-30.0, 3.5, 0.0), 2.0, b.lambertian(BLACK)))   # behind the probes' origin: what leaves through the front ends here, black
    balls.append(b.sphere((0.0, 3.5, 0.0), 1.0, mats[0]))   # the shell: ir 1.5 around a sphere of radius -0.9
    balls.append(b.sphere((0.0, 3.5, 0.0), -0.9, mats[0]))
    balls.append(b.sphere((0.0, -500.0, 0.0), 500.0, mats[-1]))
    c.objects.append(b.bvh_from_list(b.hittable_list(balls), 0.0, 1.0))
    c.extra = dict(n_spheres=len(balls))
    back = shell_back_share(1.5)
    for length in (1.0, 40.0):
        c.points.append(Point((-20.0, 3.5, 0.0), (length, 0.0, 0.0), (0.0, 0.0, back), "along the shell's axis |d|=%g" % length))
    c.conditions.append(("about 40 spheres in one BVH", len(balls) == 40))
    return c.finish(rtsr, (9.0, 6.0, 12.0), (0.0, 1.0, 0.0), 40.0, extra=extra)


# ---------------------------------------------------------------------------------------------------- scatter probes
def threshold_direction():
    """An incident direction d (coming from below onto the back face: hit normal (0, -1, 0)) and an index ir for which the
    core's own ratio * sqrt(1 - cos^2) is 1.0 EXACTLY -> (d, ir, sin) or None.  (ir = 2 with sin = 0.5 has no such double: no
    neighbour of sqrt(3) / 2 squares to 0.75.)  unit() and the two expressions are restated in float64; ir is the double
    nearest 1 / sin or one of its neighbours."""
    f = np.float64
    for sx, cy in ((0.6, 0.8), (0.5, 0.75), (0.7, 0.6), (0.45, 0.8), (0.3, 0.4), (0.55, 0.6)):
        sx, cy = f(sx), f(cy)
        length = np.sqrt(sx * sx + cy * cy + f(0.0))
        ux, uy = sx / length, cy / length
        cos = min(ux * f(0.0) + uy * f(1.0) + f(0.0), f(1.0))   # dot(-unit, normal)
        sin = np.sqrt(f(1.0) - cos * cos)
        for ir in (f(1.0) / sin, np.nextafter(f(1.0) / sin, f(0.0)), np.nextafter(f(1.0) / sin, f(9.0))):
            if ir * sin == f(1.0):
                return (float(sx), float(cy), 0.0), float(ir), float(sin)
    return None


CASES = ("glass_pane", "metal_mirror", "metal_fuzz", "media_sphere", "media_general", "surface_in_front", "casts", "two_media", "pair", "isotropic_slab", "glass_balls")
# every list world with the variants its tests use (name, variant)
LIST_WORLDS = [("glass_pane", {"ir": ir}) for ir in IRS] + [("metal_mirror", {}), ("metal_fuzz", {}), ("media_sphere", {}), ("media_general", {}),
              ("surface_in_front", {}), ("surface_in_front", {"after": True}), ("surface_in_front", {"ball": False}), ("casts", {}), ("isotropic_slab", {}),
              ("two_media", {}), ("two_media", {"b_first": True})] + [("pair", {"kind": k}) for k in PAIR_KINDS]
STATISTICAL = [(n, v) for n, v in LIST_WORLDS if n in ("glass_pane", "metal_mirror", "metal_fuzz", "media_sphere", "media_general", "pair", "isotropic_slab")] + \
              [("metal_mirror", {"edited": True}), ("metal_fuzz", {"edited": True}), ("glass_balls", {})]
_built = {}


def build(rtsr, name, **variant):
    """The named case, built once per variant."""
    key = (name,) + tuple(sorted(variant.items()))
    if key not in _built:
        _built[key] = globals()["_" + name](rtsr, **variant)
    return _built[key]


def case_id(v):
    return v if isinstance(v, str) else ("-".join("%s=%s" % kv for kv in sorted(v.items())) or "plain")
