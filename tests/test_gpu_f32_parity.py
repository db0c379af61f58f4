"""The f32 fast mode, sample by sample, against the float CPU oracle O2f (oracle/o2_flat_f32.cpp).

O2f is the product's core headers compiled for the host with real = float -- the four defines of render_f32.hip in front of
O2's loop -- over the scene narrowed by the product's own converter.  Both sides are built without fast-math and with
-ffp-contract=off, and float + - * / sqrt are correctly rounded on gfx950 and x86-64 alike (pinned below, denormals
included).  The only arithmetic that differs is the five platform functions core/rt_math.hpp calls under RT_F32.

The rule that sorts the scenes (read off the core's call sites, not found by trial):
    sinf    shading.hpp  noise texture (F_NOISE); checker texture through rt_sin_sign, which keeps only the SIGN
    logf    geometry.hpp / trace_world.inc  free path of a constant medium (F_MEDIUM)
    acosf, atan2f   geometry.hpp get_sphere_uv, only for materials whose texture tree holds an image (needs_uv)
    cosf    integrator.hpp nee_connect only -- light sampling is refused for f32 scenes, so no f32 kernel reaches it
A scene with no noise texture, no medium and no image texture reaches no platform function value: tier A, bit-exact.  The
checker stays in tier A because any faithful sinf (error below one ulp of a result that is never 0 for x != 0) has the
sign of sin x, and the sign is all rt_sin_sign returns.  Everything else is tier B: values drift by ulps and a few samples
take another branch, held to a cap on the share of unequal pixels that is derived from the CPU alone
(REFERENCE_ALONE_UNEQUAL).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# name, scene id, aspect, width, spp, depth, seed, catalogue options
EXACT_CASES = [
    ("book1", 100, 1.5, 120, 6, 50, 7, {}),
    ("book1_head", 13, 16.0 / 9.0, 128, 6, 50, 7, {}),                      # checker (sign of sinf only) + moving spheres
    ("cornell_box", 4, 1.0, 96, 8, 50, 7, {}),
    ("triangle_test", 10, 16.0 / 9.0, 96, 8, 50, 7, {}),
    ("dragon_room", 11, 16.0 / 9.0, 128, 4, 50, 7, {"mesh_triangles": 20000}),
    ("random_moving", 8, 16.0 / 9.0, 128, 4, 50, 7, {}),
]
EXACT_KERNEL = {"book1": "k_trace_lds", "book1_head": "k_trace_lds", "cornell_box": "k_trace_world",
                "triangle_test": None, "dragon_room": "k_trace_vote", "random_moving": None}
PLATFORM_CASES = [
    ("two_perlin", 1, 1.5, 120, 6, 50, 7, {}),
    ("earth", 2, 1.5, 120, 6, 50, 7, {}),
    ("cornell_smoke", 5, 1.0, 96, 8, 50, 7, {}),
    ("book2_final", 6, 1.0, 96, 6, 50, 7, {"book2_boxes_per_side": 4, "book2_spheres": 50}),
]
# Reference-alone flip rate: pixels on which the two CPU builds of O2f disagree (pixels_equal below) -- glibc's float
# functions against the same five computed in double and rounded, the kind of last-place disagreement the device has with
# glibc -- at exactly the frames above.  Measured by tests/test_oracle_f32.py::test_reference_alone_flip_rate (CPU only):
#     scene            pixels   unequal   rate
#     two_perlin         9600         0     0 % (4394 pixels differ in the last places)
#     earth              9600         0     0 % (bit-identical)
#     cornell_smoke      9216         0     0 % (bit-identical)
#     book2_final        9216         0     0 % (13 pixels differ in the last places)
# (bit differences are those between the two CPU builds.)  cap = max(4 x unequal, 5 pixels): the device functions may differ
# from BOTH builds, by up to 2 ulp (MATH_ULP below).  glibc's float functions are so nearly correctly rounded that the two
# builds never part by a visible amount at these frames, so every cap is the floor of 5 pixels.  Measured on an MI355X against
# O2f: two_perlin 0 unequal (4394 pixels differ in the last places), earth 0 (bit-identical), cornell_smoke 0
# (bit-identical), book2_final 0 (13 pixels differ in the last places); frame means agree to 1e-9.
REFERENCE_ALONE_UNEQUAL = {"two_perlin": 0, "earth": 0, "cornell_smoke": 0, "book2_final": 0}


def cap_pixels(name, n_pixels):
    cap = max(4 * REFERENCE_ALONE_UNEQUAL[name], 5)
    assert REFERENCE_ALONE_UNEQUAL[name] <= 0.02 * n_pixels and cap <= 0.08 * n_pixels, name
    return cap


def pixels_equal(got, ref, spp):
    """Per pixel: every channel of the f64 accumulator within 1e-4 |ref| + 1e-5 spp (about a thousand float ulps, far below
    any one-sample flip)."""
    return (np.abs(got - ref) <= 1e-4 * np.abs(ref) + 1e-5 * spp).all(axis=2)


def setup_case(rtsr, case, **flatten_kw):
    name, sid, aspect, width, spp, depth, seed, opts = case
    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(sid, **opts)
    flat = b.flatten(world, **flatten_kw)
    cfg = rtsr.Config.new(aspect, width, spp, depth, 10, seed=seed, background=bg)
    return b, flat, cam, cfg


_o2f_cache = {}


def _o2f(rtsr, orc, case):
    """The oracle's frame of a case, rendered once per session: (accum, rgb8)."""
    if case[0] not in _o2f_cache:
        b, flat, cam, cfg = setup_case(rtsr, case)
        _o2f_cache[case[0]] = orc.o2f_render(flat.arrays_ptr(), cam, cfg, rtsr.image_height(cfg), threads=16)
    return _o2f_cache[case[0]]


def _first_difference(rtsr, orc, flat, scene, cam, cfg, got, ref):
    """Where a frame first leaves the oracle: the first differing pixel (row-major), then the first sample count at which a
    progressive f32 frame of that scene differs from the oracle's running sum there, with the oracle's sample."""
    bad = np.argwhere((got != ref).any(axis=2))
    j, i = int(bad[0][0]), int(bad[0][1])
    h = rtsr.image_height(cfg)
    msg = "%d of %d pixels differ; first (i, j) = (%d, %d): gpu %r, o2f %r" % (len(bad), got.shape[0] * got.shape[1], i, j,
                                                                              got[j, i].tolist(), ref[j, i].tolist())
    try:
        prog = scene.progressive(cam, cfg)
        s = np.zeros(3)
        for k in range(cfg.samples_per_pixel):
            prog.add(1)
            x = orc.o2f_sample(flat.arrays_ptr(), cam, cfg, h, i, j, k)
            prev, s = s, s + x
            g = prog.screen().accum[j, i]
            if not np.array_equal(g, s):
                return msg + "; first differing sample %d: gpu %r, o2f %r" % (k, (g - prev).tolist(), x.tolist())
    except Exception as e:  # the diagnosis must not hide the failure itself
        msg += " (no per-sample diagnosis: %r)" % (e,)
    return msg


EXACT_VARIANTS = [
    ("default", {}),
    ("simple", {"RTX_TRACE_KERNEL": "simple"}),
    ("world", {"RTX_TRACE_KERNEL": "world"}),
    ("vote", {"RTX_TRACE_KERNEL": "vote"}),
    ("wavefront", {"RTX_TRACE_KERNEL": "wavefront"}),
    ("wide0", {"RTX_WIDE": "0"}),
    ("wide1", {"RTX_WIDE": "1"}),
    ("ring0", {"RTX_RING": "0"}),
    ("ring1", {"RTX_RING": "1"}),
]


@pytest.mark.parametrize("vname,env", EXACT_VARIANTS, ids=[v[0] for v in EXACT_VARIANTS])
@pytest.mark.parametrize("case", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_f32_kernels_equal_the_float_oracle(rtsr, orc, monkeypatch, case, vname, env):
    """Tier A: every f32 trace kernel's accumulator and picture equal O2f's bit for bit -- and so each other's."""
    name, spp = case[0], case[4]
    ref_accum, ref_rgb8 = _o2f(rtsr, orc, case)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    b, flat, cam, cfg = setup_case(rtsr, case)
    scene = flat.upload(f32=True)
    assert scene.is_f32
    kernel = rtsr.trace_kernel_name(scene.render_device(cam, cfg, want_stats=True).trace_kernel)
    if vname == "default" and EXACT_KERNEL[name]:
        assert kernel == EXACT_KERNEL[name]
    if vname == "simple":
        assert kernel == "k_trace_simple"
    if vname == "world":
        assert kernel == "k_trace_world"
    if vname in ("ring0", "ring1") and EXACT_KERNEL[name] == "k_trace_lds":
        assert kernel == "k_trace_lds"
    screen = scene.render(cam, cfg)
    print("%s %s: kernel %s, %d pixels differ" % (name, vname, kernel, int((screen.accum != ref_accum).any(axis=2).sum())))
    if not np.array_equal(screen.accum, ref_accum):
        pytest.fail("%s through %s (%s): %s" % (name, vname, kernel, _first_difference(rtsr, orc, flat, scene, cam, cfg, screen.accum, ref_accum)))
    assert np.array_equal(screen.rgb8, ref_rgb8)


def test_f32_dragon_room_through_the_gpu_built_tree(rtsr, orc):
    """The GPU-built tree is another tree over the same triangles: O2f walks the flat scene it is given, so it must agree
    with the kernels on this tree too, and the two trees must give one picture."""
    case = [c for c in EXACT_CASES if c[0] == "dragon_room"][0]
    b, flat, cam, cfg = setup_case(rtsr, case, gpu_builder=True)
    ref_accum, ref_rgb8 = orc.o2f_render(flat.arrays_ptr(), cam, cfg, rtsr.image_height(cfg), threads=16)
    screen = flat.upload(f32=True).render(cam, cfg)
    assert np.array_equal(screen.accum, ref_accum) and np.array_equal(screen.rgb8, ref_rgb8)
    host_accum, _ = _o2f(rtsr, orc, case)
    assert np.array_equal(ref_accum, host_accum)


def test_f32_shards_progressive_and_adaptive_equal_the_float_oracle(rtsr, orc):
    from test_gpu_progressive import _rel_err, _with
    case = EXACT_CASES[0]
    b, flat, cam, cfg = setup_case(rtsr, case)
    h = rtsr.image_height(cfg)
    ref_accum, ref_rgb8 = _o2f(rtsr, orc, case)
    # three row-interleaved shards, each against the oracle's own rendering of that shard
    parts = rtsr.MultiScene(flat, 3, device_ids=[0, 0, 0], f32=True).render(cam, cfg)
    assert np.array_equal(parts.accum, ref_accum) and np.array_equal(parts.rgb8, ref_rgb8)
    for idx in range(3):
        rows, _ = orc.o2f_render(flat.arrays_ptr(), cam, cfg, h, shard=(idx, 3, 1), threads=16)
        assert np.array_equal(rows, ref_accum[idx::3])
    # one progressive handle, 1 + 3 + 4 samples; the oracle continues its sums the same way
    scene = flat.upload(f32=True)
    cfg8 = _with(rtsr, cfg, samples_per_pixel=8)
    prog = scene.progressive(cam, cfg8)
    acc, done = None, 0
    for n in (1, 3, 4):
        prog.add(n)
        acc, rgb = orc.o2f_render(flat.arrays_ptr(), cam, _with(rtsr, cfg, samples_per_pixel=n), h, threads=16, first_sample=done, accum=acc)
        done += n
        got = prog.screen()
        assert np.array_equal(got.accum, acc) and np.array_equal(got.rgb8, rgb), done
        if done == 4:
            snap = acc
    one_shot, _ = orc.o2f_render(flat.arrays_ptr(), cam, cfg8, h, threads=16)
    assert np.array_equal(acc, one_shot)
    # one adaptive round: the pixels retired at the check hold the oracle's sums at that count, the others at the budget
    prog = scene.progressive(cam, cfg8)
    prog.add_adaptive(4, 2, 0.0)
    S, Q = prog.moments()
    assert np.array_equal(S, snap)
    target = float(np.median(_rel_err(S, Q, 4)))
    prog.add_adaptive(4, 2, target)
    counts = prog.pixel_spp()
    assert 0 < int((counts == 4).sum()) < counts.size and set(np.unique(counts).tolist()) == {4, 8}
    S, _ = prog.moments()
    assert np.array_equal(S[counts == 4], snap[counts == 4])
    assert np.array_equal(S[counts == 8], one_shot[counts == 8])


@pytest.mark.parametrize("case", PLATFORM_CASES, ids=[c[0] for c in PLATFORM_CASES])
def test_f32_platform_function_scenes_stay_within_the_flip_cap(rtsr, orc, case):
    """Tier B: scenes whose samples go through sinf / logf / acosf / atan2f."""
    name, spp = case[0], case[4]
    ref_accum, _ = _o2f(rtsr, orc, case)
    b, flat, cam, cfg = setup_case(rtsr, case)
    screen = flat.upload(f32=True).render(cam, cfg)
    unequal = ~pixels_equal(screen.accum, ref_accum, spp)
    rel = abs(screen.accum.mean() - ref_accum.mean()) / ref_accum.mean()
    cap = cap_pixels(name, unequal.size)
    print("%s: %d of %d pixels unequal (cap %d), %d bit-different, frame means differ by %.3g"
          % (name, int(unequal.sum()), unequal.size, cap, int((screen.accum != ref_accum).any(axis=2).sum()), rel))
    assert int(unequal.sum()) <= cap, (name, int(unequal.sum()), cap)
    assert rel <= 1e-3, (name, rel)


# ---- the building blocks themselves --------------------------------------------------------------------------------------
def _ulps(got, want):
    """Distance in float32 steps between two float32 arrays (+0 and -0 are 0 apart; NaN against NaN is 0, against a number a
    huge count)."""
    def key(a):
        i = a.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(got) - key(want))
    both_nan = np.isnan(got) & np.isnan(want)
    one_nan = np.isnan(got) != np.isnan(want)
    return np.where(both_nan, 0, np.where(one_nan, 1 << 40, d))


def _f32(fn_values):
    return np.asarray(fn_values, dtype=np.float64).astype(np.float32)


EDGES = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38, 1.0 - 2.0 ** -24, 1.0, -1.0, np.inf, -np.inf,
                  np.nan], dtype=np.float32)
# The largest distance, in float32 ulps, between the device's function (OCML on gfx950, called through the f32 compilation's
# rt_sin ...) and numpy's float64 function rounded to float32, measured on an MI355X over the sweeps below, plus one ulp of
# headroom for a ROCm point release.  Measured (ROCm 7.2): sinf 2, cosf 2, logf 2, acosf 1, atan2f 2.
MATH_ULP = {"sinf": 3, "cosf": 3, "logf": 3, "acosf": 2, "atan2f": 3}


def _sweeps():
    rng = np.random.default_rng(11)
    n = 400000
    f = np.float32
    # sinf / cosf: the noise texture's scale * p.z + 10 * turbulence (|.| up to a few thousand on the r = 1000 ground), the
    # checker's 10 * p (|p| up to ~1e4 where a ray still sees the ground), a light sample's angle 2 pi u, and small arguments
    trig = np.concatenate([rng.uniform(-8, 8, n), rng.uniform(-5000, 5000, n), rng.uniform(-1e5, 1e5, n),
                           rng.uniform(0, 2 * np.pi, n), rng.uniform(-1e-3, 1e-3, n)]).astype(f)
    trig = np.concatenate([trig, EDGES])
    # logf: rng_f64 values k 2^-24 (k = 0 gives -inf), the top of the range densely, and any float of (0, 1]
    k = rng.integers(0, 1 << 24, n)
    logx = np.concatenate([(k * 2.0 ** -24).astype(f), ((1 << 24) - 1 - np.arange(1 << 16)) * f(2.0 ** -24),
                           np.arange(1 << 12).astype(f) * f(2.0 ** -24), rng.uniform(0, 1, n).astype(f), EDGES])
    acosx = np.concatenate([rng.uniform(-1, 1, n).astype(f), np.nextafter(f(1), f(0)) - np.arange(4096).astype(f) * f(2.0 ** -24),
                            -1 + np.arange(4096).astype(f) * f(2.0 ** -24), EDGES, np.array([1.0000001, -1.0000001], dtype=f)])
    ay = np.concatenate([rng.uniform(-1, 1, n), rng.normal(0, 1e-3, n), rng.uniform(-1, 1, n)]).astype(f)
    ax = np.concatenate([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.normal(0, 1e-3, n)]).astype(f)
    ey, ex = np.meshgrid(EDGES, EDGES)
    ay, ax = np.concatenate([ay, ey.ravel()]), np.concatenate([ax, ex.ravel()])
    return trig, logx, acosx, ay, ax


def test_f32_platform_functions_within_measured_ulps(rtsr):
    trig, logx, acosx, ay, ax = _sweeps()
    with np.errstate(all="ignore"):
        jobs = [("sinf", trig, None, _f32(np.sin(trig.astype(np.float64)))),
                ("cosf", trig, None, _f32(np.cos(trig.astype(np.float64)))),
                ("logf", logx, None, _f32(np.log(logx.astype(np.float64)))),
                ("acosf", acosx, None, _f32(np.arccos(acosx.astype(np.float64)))),
                ("atan2f", ay, ax, _f32(np.arctan2(ay.astype(np.float64), ax.astype(np.float64))))]
    worst = {}
    for fn, x, y, want in jobs:
        got = rtsr.device_math(fn, x, y).astype(np.float32)
        d = _ulps(got, want)
        worst[fn] = int(d.max())
        k = int(d.argmax())
        print("%s: max %d ulp at x = %r%s (device %r, float64 rounded %r)"
              % (fn, worst[fn], x[k], "" if y is None else ", y = %r" % y[k], got[k], want[k]))
    for fn in worst:
        assert worst[fn] <= MATH_ULP[fn], (fn, worst[fn])
    # exact where IEEE 754 / C Annex F say so
    f = np.float32
    one = rtsr.device_math
    assert one("logf", f([1.0]))[0] == 0.0 and not np.signbit(one("logf", f([1.0]))[0])
    assert one("logf", f([0.0, -0.0])).tolist() == [-np.inf, -np.inf]
    assert one("acosf", f([1.0]))[0] == 0.0 and not np.signbit(one("acosf", f([1.0]))[0])
    z = one("atan2f", f([0.0, -0.0, 0.0, -0.0]), f([1.0, 1.0, 1e-40, np.inf]))
    assert (z == 0.0).all() and np.signbit(z).tolist() == [False, True, False, True]
    nan = f([np.nan])
    for fn in ("sinf", "cosf", "logf", "acosf"):
        assert np.isnan(one(fn, nan)[0]), fn
    assert np.isnan(one("atan2f", nan, f([1.0]))[0]) and np.isnan(one("atan2f", f([1.0]), nan)[0])
    assert np.isnan(one("sinf", f([np.inf]))[0]) and np.isnan(one("cosf", f([-np.inf]))[0])
    assert np.isnan(one("logf", f([-1.0]))[0]) and np.isnan(one("acosf", f([1.0000001]))[0])


def test_f32_sin_sign_is_the_sign_of_sin(rtsr):
    """What keeps the checker texture in tier A: the device's rt_sin_sign (sinf's sign) equals the sign of sin x computed in
    double, over the checker's arguments 10 p and next to every multiple of pi up to 1e5."""
    rng = np.random.default_rng(13)
    k = np.arange(1, 31831)
    near = (k * np.pi).astype(np.float32)
    x = np.concatenate([rng.uniform(-1e5, 1e5, 400000).astype(np.float32), near, np.nextafter(near, np.float32(np.inf)),
                        np.nextafter(near, np.float32(0)), -near, np.float32([0.0, -0.0, 1e-45, -1e-45, 1e-30])])
    got = rtsr.device_math("sin_signf", x)
    want = np.sign(np.sin(x.astype(np.float64)))
    assert np.array_equal(got, want), int((got != want).sum())
    assert rtsr.device_math("sin_signf", np.float32([np.inf, np.nan])).tolist() == [2.0, 2.0]


def test_f32_sqrt_and_division_are_correctly_rounded(rtsr):
    """What tier A rests on: float sqrt and division of the f32 compilation equal numpy float32 -- correctly rounded,
    denormal operands and results kept."""
    rng = np.random.default_rng(17)
    n = 400000
    f = np.float32
    with np.errstate(all="ignore"):
        p = np.concatenate([np.abs(rng.normal(0, 1e3, n)) ** rng.uniform(0.1, 3, n), rng.uniform(0, 1e-38, n), rng.uniform(0, 1e-44, 64),
                            [0.0, -0.0, 1e-45, 1.1754942e-38, 3.4028235e38, np.inf, -1.0, np.nan]]).astype(f)
        got = rtsr.device_math("sqrtf", p).astype(f)
        assert np.array_equal(got.view(np.uint32)[~np.isnan(got)], np.sqrt(p).view(np.uint32)[~np.isnan(got)])
        assert np.array_equal(np.isnan(got), np.isnan(np.sqrt(p)))
        q = np.concatenate([rng.normal(0, 10, n), rng.normal(0, 1e-30, n), rng.normal(0, 1e-38, n), rng.normal(0, 1, n)]).astype(f)
        d = np.concatenate([rng.normal(0, 10, n), rng.normal(0, 1e8, n), rng.normal(0, 1, n), rng.normal(0, 1e-38, n)]).astype(f)
        eq, ed = np.meshgrid(EDGES, EDGES)
        q, d = np.concatenate([q, eq.ravel()]), np.concatenate([d, ed.ravel()])
        got = rtsr.device_math("divf", q, d).astype(f)
        want = q / d
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok]), int((got.view(np.uint32)[ok] != want.view(np.uint32)[ok]).sum())
    assert int(((want != 0) & (np.abs(want) < 1.17549435e-38)).sum()) > 1000   # denormal results are in the set


def test_f32_rng_forms_equal_numpy_restatements(rtsr):
    """The three float RNG forms of core/rng.hpp on the device, from raw 64-bit draws covering all 2^23 mantissas (and all 2^24
    unit floats), against numpy restatements: every step is exact or one correctly rounded float operation."""
    f = np.float32
    m = np.arange(1 << 24, dtype=np.uint64)
    low = (m * np.uint64(0x9E3779B97F4A7C15)) & np.uint64((1 << 40) - 1)     # the bits below must not matter
    raw = (m << np.uint64(40)) | low                                        # top 24 bits = m: every unit float
    got = rtsr.device_math("rng_f32", raw.view(np.float64))
    assert np.array_equal(got, m.astype(np.float64) * 2.0 ** -24)
    mant = ((raw >> np.uint64(41)).astype(np.uint32))                       # every 23-bit mantissa, twice
    assert np.unique(mant).size == 1 << 23
    got = rtsr.device_math("rng_range_pm1_f32", raw.view(np.float64)).astype(f)
    want = (mant | np.uint32(0x40000000)).view(f) + f(-3.0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert want.min() == -1.0 and want.max() < 1.0
    for lo, hi in ((-1.0, 1.0), (0.0, 1.0), (0.5, 1.0), (0.0, 0.5), (-11.0, 11.0), (0.0, 165.0)):   # the ranges the scenes draw from
        lohi = np.full(raw.size, np.uint64(f(lo).view(np.uint32)) | (np.uint64(f(hi).view(np.uint32)) << np.uint64(32)), dtype=np.uint64)
        got = rtsr.device_math("rng_range_f32", raw.view(np.float64), lohi.view(np.float64)).astype(f)
        scale = f(hi) - f(lo)
        want = (mant | np.uint32(0x3F800000)).view(f) * scale + (f(lo) - scale)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (lo, hi)


# (finite slopes are powers of two here: the device's v_rcp_f32 is exact on them, so host and device can be held to one table)
SLOPE_CAP_IN = np.float32([0.0, -0.0, np.nan, np.inf, -np.inf, 2.0 ** -100, -2.0 ** -100, 1e-45, -1e-45, 2.0 ** -60, 2.0 ** -61, 0.5, -4.0])
SLOPE_CAP_OUT = [2.0 ** 60, -2.0 ** 60, -2.0 ** 60, 0.0, -0.0, 2.0 ** 100, -2.0 ** 100, 2.0 ** 60, -2.0 ** 60, 2.0 ** 60, 2.0 ** 61, 2.0, -0.25]


def test_f32_slope_cap_is_the_same_on_host_and_device(rtsr, orc):
    """core/cull32.hpp replaces a slope 1 / d that is not finite by +-2^60 and keeps every finite one, however steep (a clamp
    into +-2^60 culled boxes a ray with a component below 2^-60 enters: tests/test_cull_conservative.py).  Host and device must
    agree where that is not plain arithmetic: d = +-0 (+-inf -> +-2^60), NaN (-2^60), +-inf (a zero slope keeps its sign), a
    denormal d (its reciprocal overflows on the host and is flushed on the device: +-2^60 both), 2^-60, and 2^-61 and 2^-100,
    which stay 2^61 and 2^100."""
    want = np.float32(SLOPE_CAP_OUT)
    host = orc.core32_math("slope_capf", SLOPE_CAP_IN).astype(np.float32)
    dev = rtsr.device_math("slope_capf", SLOPE_CAP_IN).astype(np.float32)
    assert host.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert dev.view(np.uint32).tolist() == want.view(np.uint32).tolist()
