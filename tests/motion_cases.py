"""Moving spheres under every kind of time interval: a sphere's own (time0, time1), the interval of the BvhNode above it and
the camera's shutter, each offset, negative, far from 0, reversed, empty, nested either way or mixed within one BVH.

build(rtsr, case_id, ...) returns (builder, world, cam, cfg, movers): a world of ONE bvh_from_list over about 120 spheres in a
box of 8 x 1.5 x 8 (every fourth static, a checkered ground sphere; Lambertian, metal and dielectric only, so the scene stays
k_trace_lds's), or with as_list the first 40 of the same objects as a plain HittableList (k_trace_world's);
movers: one (c0, c1, time0, time1, r) per MovingSphere, in list order.  Coordinates come from a seeded numpy RandomState, so the
same objects can be rebuilt in another Builder.  Frames: 96 x 64, 4 spp, depth 20.

expected_variant says which k_trace_lds instantiation the launcher must report for a case (RtxRenderStats.trace_variant).
tests/test_motion_cases.py proves the cases on the CPU; tests/test_gpu_motion_cases.py runs the device on them."""
import numpy as np

SKY = (0.6, 0.7, 0.9)
N_BVH, N_LIST = 120, 40
TIME_BOXES, ONE_AXIS, COMMON_RATIO = 1, 2, 4  # bits of RtxRenderStats.trace_variant

# id -> (sphere intervals, taken by k % len; the BVH's interval; the shutters; the axes the movers move along)
CASES = {
    "unit": ([(0.0, 1.0)], (0.0, 1.0), [(0.0, 1.0)], "xyz"),
    "offset": ([(2.0, 3.5)], (2.0, 3.5), [(2.25, 3.25), (2.0, 3.5)], "xyz"),
    "negative": ([(-1.5, -0.25)], (-1.5, -0.25), [(-1.5, -0.25)], "xyz"),
    "far_offset": ([(1000.0, 1000.5)], (1000.0, 1000.5), [(1000.0, 1000.5)], "xyz"),
    "bvh_narrower": ([(0.0, 1.0)], (0.25, 0.75), [(0.3, 0.7)], "xyz"),
    "bvh_wider": ([(0.25, 0.5)], (0.0, 1.0), [(0.0, 1.0)], "xyz"),
    "mixed": ([(0.0, 1.0), (0.25, 0.5), (-1.0, 2.0)], (0.0, 1.0), [(0.0, 1.0)], "xyz"),
    "reversed": ([(1.0, 0.0)], (0.0, 1.0), [(0.0, 1.0)], "xyz"),
    "reversed_bvh": ([(0.0, 1.0)], (1.0, 0.0), [(0.0, 1.0)], "xyz"),
    "x_only": ([(2.0, 3.5)], (2.0, 3.5), [(2.25, 3.25)], "x"),
    "z_only": ([(2.0, 3.5)], (2.0, 3.5), [(2.25, 3.25)], "z"),
    "y_only_offset": ([(2.0, 3.5)], (2.0, 3.5), [(2.25, 3.25)], "y"),
    "straddle": ([(2.0, 3.5)], (2.0, 3.5), [(3.0, 4.0), (1.0, 2.5)], "xyz"),
    "degenerate": ([(0.5, 0.5)], (0.0, 1.0), [(0.0, 1.0)], "xyz"),
}
PARITY = [c for c in CASES if c not in ("straddle", "degenerate")]  # the cases with one frame through a BVH
SHUTTERS = [(c, k) for c in CASES for k in range(len(CASES[c][2]))]


def shutter_inside(case_id, shutter=0):
    """The time-aware boxes apply: the BVH's interval is ordered and holds the whole shutter."""
    (b0, b1), (s0, s1) = CASES[case_id][1], CASES[case_id][2][shutter]
    return b0 < b1 and b0 <= s0 and s1 <= b1


def expected_variant(case_id, shutter=0, env=None):
    """RtxRenderStats.trace_variant of a k_trace_lds render of the BVH form, under the RTX_* switches named in env."""
    env = env or {}
    motion = shutter_inside(case_id, shutter) and env.get("RTX_MOTION") != "0"
    one_axis = motion and case_id == "y_only_offset" and env.get("RTX_MOTION_AXIS") != "0"
    common = case_id not in ("mixed", "degenerate") and env.get("RTX_MV_COMMON") != "0"
    return (TIME_BOXES if motion else 0) | (ONE_AXIS if one_axis else 0) | (COMMON_RATIO if common else 0)


def _objects(case_id, n, with_movers=True):
    """[(kind, c0, c1, t0, t1, r, material index)] of the first n objects: the ground, then spheres, every fourth static."""
    intervals, _, _, axes = CASES[case_id]
    rng = np.random.RandomState(20)
    out = [("ground", (0.0, -300.0, 0.0), None, 0.0, 0.0, 300.0, 3)]
    for k in range(n - 1):
        c0 = np.array([8.0 * rng.rand() - 4.0, 0.25 + 1.5 * rng.rand(), 8.0 * rng.rand() - 4.0])
        r = 0.12 + 0.2 * rng.rand()
        # every axis a mover moves along by 0.25 .. 1.0 either way: no mover travels less than 0.25
        step = (0.25 + 0.75 * rng.rand(3)) * np.where(rng.rand(3) < 0.5, -1.0, 1.0)
        step[1] = abs(step[1]) if c0[1] < 1.0 else step[1]  # (not into the ground)
        if k % 4 == 0:
            out.append(("static", tuple(c0), None, 0.0, 0.0, r, k % 3))
        elif with_movers:
            c1 = c0 + np.array([step[a] if "xyz"[a] in axes else 0.0 for a in range(3)])
            t0, t1 = intervals[k % len(intervals)]
            out.append(("mover", tuple(c0), tuple(c1), t0, t1, r, k % 3))
    return out


def build(rtsr, case_id, shutter=0, as_list=False, with_movers=True):
    intervals, bvh, shutters, _ = CASES[case_id]
    b = rtsr.Builder(21)
    mats = [b.lambertian((0.7, 0.3, 0.3)), b.metal((0.8, 0.8, 0.7), 0.1), b.dielectric(1.5),
            b.lambertian(b.checker_from_colors((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))]
    objs, movers = [], []
    for kind, c0, c1, t0, t1, r, m in _objects(case_id, N_LIST if as_list else N_BVH, with_movers):
        if kind == "mover":
            objs.append(b.moving_sphere(c0, c1, t0, t1, r, mats[m]))
            movers.append((c0, c1, t0, t1, r))
        else:
            objs.append(b.sphere(c0, r, mats[m]))
    if as_list:
        world = b.hittable_list(objs)
    else:
        world = b.hittable_list([b.bvh_from_list(b.hittable_list(objs), bvh[0], bvh[1])])
    s0, s1 = shutters[shutter]
    cam = rtsr.Camera.new((7.0, 3.0, 8.0), (0.0, 0.8, 0.0), (0.0, 1.0, 0.0), 35.0, 1.5, 0.05, 10.0, s0, s1)
    cfg = rtsr.Config.new(1.5, 96, 4, 20, 4, seed=9, background=SKY)
    return b, world, cam, cfg, movers


def centre(mover, t):
    """c(t) = c0 + (t - time0) / (time1 - time0) * (c1 - c0) in numpy.longdouble, from the table."""
    c0, c1, t0, t1, _ = mover
    L = np.longdouble
    ratio = (L(t) - L(t0)) / (L(t1) - L(t0))
    return np.array([L(c0[a]) + ratio * (L(c1[a]) - L(c0[a])) for a in range(3)])


FRACTIONS = (0.0, 0.3125, 0.5, 1.0)
DIRECTIONS = ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, -1.0))


def instants(case_id):
    """The instants t0b + f * (t1b - t0b) of the BVH's interval the closed-form rays are cast at."""
    b0, b1 = CASES[case_id][1]
    return [b0 + f * (b1 - b0) for f in FRACTIONS]


def centre_rays(case_id, movers):
    """For every instant: (t, origins (n, 3) f64, directions (n, 3), radii (n,), blocked (n,) bool) of the rays from every
    mover's centre c(t) along +y, +x and -z.  Such a ray leaves its own sphere at distance r exactly.  blocked: another
    sphere of the scene (worked out here in longdouble, from the table) is met before that, between the integrator's t_min
    of 0.001 and r (1 + 1e-6): a neighbour that overlaps the sphere answers first, and the ray claims nothing."""
    L = np.longdouble
    objs = _objects(case_id, N_BVH)
    out = []
    for t in instants(case_id):
        cs, rs = [], []
        k = 0
        for kind, c0, c1, t0, t1, r, _ in objs:
            if kind == "mover":
                cs.append(centre(movers[k], t))
                k += 1
            else:
                cs.append(np.array([L(x) for x in c0]))
            rs.append(L(r))
        cs, rs = np.array(cs), np.array(rs)
        own = [i for i, o in enumerate(objs) if o[0] == "mover"]
        origins, dirs, radii, blocked = [], [], [], []
        for i in own:
            for d in DIRECTIONS:
                d = np.array([L(x) for x in d])
                oc = cs[i] - cs  # origin - centres
                half_b = oc @ d
                disc = half_b * half_b - ((oc * oc).sum(axis=1) - rs * rs)
                root = np.sqrt(np.where(disc > 0, disc, 0))
                hit = np.zeros(len(cs), dtype=bool)
                for t_hit in (-half_b - root, -half_b + root):
                    hit |= (disc > 0) & (t_hit > L(0.001) * (1 - L(1e-6))) & (t_hit < rs[i] * (1 + L(1e-6)))
                hit[i] = False
                origins.append(cs[i].astype(np.float64))
                dirs.append(d.astype(np.float64))
                radii.append(float(rs[i]))
                blocked.append(bool(hit.any()))
        out.append((t, np.ascontiguousarray(origins), np.ascontiguousarray(dirs), np.array(radii), np.array(blocked)))
    return out
