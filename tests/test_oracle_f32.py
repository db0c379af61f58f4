"""The float CPU oracle O2f (oracle/o2_flat_f32.cpp) against the double one, without a GPU.

O2f is what tests/test_gpu_f32_parity.py holds the f32 kernels to, so it has to be right on its own: the scene it walks
is the product's narrowing of the f64 one (checked field by field here), it renders the same picture as O2 by the bars
tests/test_gpu_f32.py holds the GPU's f32 frames to, it does not depend on threads or shards, and the three hazards of
single-precision rays are pinned as single-ray cases.  The share of pixels on which its two builds
disagree -- glibc's float functions against the same functions computed in double -- is the reference-alone flip rate the
GPU tests' caps come from.
"""
import numpy as np
import pytest

from test_gpu_f32_parity import EXACT_CASES, PLATFORM_CASES, REFERENCE_ALONE_UNEQUAL, cap_pixels, pixels_equal, setup_case

ALL_CASES = EXACT_CASES + PLATFORM_CASES


# ---- the converter -------------------------------------------------------------------------------------------------------
def _fields(desc):
    """A descriptor string laid out again, independently: [(kind, offset64, offset32)] per scalar, size64, size32."""
    out, o64, o32, a64, a32 = [], 0, 0, 1, 1
    for tok in desc.split():
        kind, count = tok[0], int(tok[1:])
        w64 = 4 if kind == "i" else 8
        w32 = 4 if kind in "rdu" else w64
        o64 = -(-o64 // w64) * w64
        o32 = -(-o32 // w32) * w32
        for _ in range(count):
            out.append((kind, o64, o32))
            o64 += w64
            o32 += w32
        a64, a32 = max(a64, w64), max(a32, w32)
    return out, -(-o64 // a64) * a64, -(-o32 // a32) * a32


def _narrow(kind, x):
    """numpy's statement of the three roundings."""
    with np.errstate(over="ignore"):
        f = x.astype(np.float32)
        if kind == "d":
            f = np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f)
        if kind == "u":
            f = np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f)
    return f.astype(np.float32)


def _check_descriptor(orc, name, desc, raw64, elem64):
    fields, size64, size32 = _fields(desc)
    assert size64 == elem64, (name, desc, size64, elem64)
    out, e32 = orc.f32_convert(desc, raw64, elem64)
    assert e32 == size32, (name, e32, size32)
    n = raw64.size // elem64
    src, dst = raw64.reshape(n, elem64), out.reshape(n, size32)
    covered = np.zeros(size32, dtype=bool)
    for kind, o64, o32 in fields:
        if kind in "il":
            w = 4 if kind == "i" else 8
            assert np.array_equal(dst[:, o32:o32 + w], src[:, o64:o64 + w]), (name, kind, o64)   # integers are untouched
            covered[o32:o32 + w] = True
            continue
        x = np.ascontiguousarray(src[:, o64:o64 + 8]).view(np.float64).ravel()
        y = np.ascontiguousarray(dst[:, o32:o32 + 4]).view(np.float32).ravel()
        covered[o32:o32 + 4] = True
        want = _narrow(kind, x)
        ok = ~np.isnan(x)
        assert np.array_equal(y.view(np.uint32)[ok], want.view(np.uint32)[ok]), (name, kind, o64)   # sign of zero included
        assert np.isnan(y[~ok]).all()
        yd = y.astype(np.float64)
        with np.errstate(over="ignore"):
            up, down = np.nextafter(y, np.float32(np.inf)).astype(np.float64), np.nextafter(y, np.float32(-np.inf)).astype(np.float64)
        if kind == "d":   # never above the f64 value, and the next float up is: at most one ulp away
            assert (yd[ok] <= x[ok]).all() and (up[ok & (y < np.inf)] > x[ok & (y < np.inf)]).all()
        if kind == "u":
            assert (yd[ok] >= x[ok]).all() and (down[ok & (y > -np.inf)] < x[ok & (y > -np.inf)]).all()
    assert (dst[:, ~covered] == 0).all()   # padding is zeroed


SPECIAL = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, -(1.0 + 2.0 ** -24), 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -30,
                    -(1.0 + 2.0 ** -30), 16777217.0, -16777217.0, 0.1, -0.1, 1e-300, -1e-300, 1e-45, 2.0 ** -150, -2.0 ** -150, 2.0 ** -149,
                    1e300, -1e300, 3.4028234663852886e38, 3.4028235677973366e38, -3.4028235677973366e38, np.inf, -np.inf, np.nan,
                    -555.0000001, -554.9999999, 1000.0000001])


def test_every_descriptor_narrows_like_numpy(rtsr, orc):
    """r fields round to nearest, d fields never land above and u fields never below their f64 value (each within one float
    ulp), integers and the sign of zero pass through -- on the arrays of catalogue scenes and on elements made of values that
    are exactly representable, halfway between floats, +-0, beyond float's range, denormal, and negative box planes."""
    descs = orc.f32_descs()
    assert len(descs) == 12
    seen = set()
    for sid, opts in ((6, {"book2_boxes_per_side": 4, "book2_spheres": 50}), (13, {}), (11, {"mesh_triangles": 2000}), (2, {})):
        b = rtsr.Builder(1)
        world, cam, bg = b.get_world_cam(sid, **opts)
        flat = b.flatten(world)
        for name, desc in descs:
            raw, elem = orc.flat_array(flat.arrays_ptr(), name)
            if raw.size:
                _check_descriptor(orc, name, desc, raw, elem)
                seen.add(name)
    assert {"spheres", "moving_spheres", "rects", "triangles", "nodes", "entries", "materials", "textures", "perlins", "texels"} <= seen
    rng = np.random.default_rng(3)
    for name, desc in descs:   # synthetic elements: every real field walks through SPECIAL, every integer field holds random bits
        fields, size64, _ = _fields(desc)
        n = SPECIAL.size * 3
        raw = np.zeros((n, size64), dtype=np.uint8)
        for k, (kind, o64, _) in enumerate(fields):
            if kind in "il":
                w = 4 if kind == "i" else 8
                raw[:, o64:o64 + w] = rng.integers(0, 256, (n, w), dtype=np.uint8)
            else:
                vals = np.roll(np.tile(SPECIAL, 3), k)
                raw[:, o64:o64 + 8] = vals.view(np.uint8).reshape(n, 8)
        _check_descriptor(orc, name, desc, raw.ravel(), size64)
    assert orc.f32_convert("r4 i2", np.zeros(48, dtype=np.uint8), 48)[1] == 0   # a descriptor that does not fit its struct is refused


# ---- the same picture as the double oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_o2f_renders_the_same_picture_as_o2(rtsr, orc, case):
    """The bars of tests/test_gpu_f32.py::test_f32_renders_the_same_picture, on the CPU: frame mean within 0.5 %, 90 % of the
    pixels within 5 % + 0.02, no non-finite pixel the f64 frame does not have."""
    name, spp = case[0], case[4]
    b, flat, cam, cfg = setup_case(rtsr, case)
    h = rtsr.image_height(cfg)
    a64, _ = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=16)
    a32, rgb = orc.o2f_render(flat.arrays_ptr(), cam, cfg, h, threads=16)
    assert not np.array_equal(a32, a64)   # it really is the other arithmetic
    a, c = a64 / spp, a32 / spp
    assert np.isfinite(c).all() or not np.isfinite(a).all()
    rel = abs(c.mean() - a.mean()) / a.mean()
    la, lc = a.mean(axis=2), c.mean(axis=2)
    close = np.abs(la - lc) <= 0.05 * np.abs(la) + 0.02
    print("%s: mean rel %.3g, close %.4f" % (name, rel, close.mean()))
    assert rel < 5e-3, (name, rel)
    assert close.mean() > 0.90, (name, close.mean())
    # the picture is the float tone map of the float-cast sum (k_tonemap)
    want = np.floor(np.float32(255.9) * np.clip(np.sqrt(a32.astype(np.float32) * (np.float32(1.0) / np.float32(spp))), 0, 1)).astype(np.uint8)
    assert np.array_equal(rgb, want)


def test_o2f_is_deterministic_and_independent_of_threads_shards_and_splits(rtsr, orc):
    from test_gpu_progressive import _with
    case = EXACT_CASES[1]   # moving spheres + checker
    b, flat, cam, cfg = setup_case(rtsr, case)
    h, p = rtsr.image_height(cfg), flat.arrays_ptr()
    one, rgb1 = orc.o2f_render(p, cam, cfg, h, threads=1)
    for threads in (3, 16):
        a, r = orc.o2f_render(p, cam, cfg, h, threads=threads)
        assert np.array_equal(a, one) and np.array_equal(r, rgb1)
    for count, block in ((3, 1), (2, 4)):
        whole = np.zeros_like(one)
        for idx in range(count):
            rows = [j for j in range(h) if (j // block) % count == idx]
            part, _ = orc.o2f_render(p, cam, cfg, h, shard=(idx, count, block), threads=5)
            whole[rows] = part
        assert np.array_equal(whole, one)
    # a frame added in pieces continues the same ordered sums, and one sample is what the frame adds
    acc, done = None, 0
    for n in (1, 3, case[4] - 4):
        acc, rgb = orc.o2f_render(p, cam, _with(rtsr, cfg, samples_per_pixel=n), h, threads=7, first_sample=done, accum=acc)
        done += n
    assert np.array_equal(acc, one) and np.array_equal(rgb, rgb1)
    for i, j in ((0, 0), (64, 30), (127, h - 1)):
        s = np.zeros(3)
        for k in range(case[4]):
            s = s + orc.o2f_sample(p, cam, cfg, h, i, j, k)
        assert np.array_equal(s, one[j, i])


@pytest.mark.parametrize("case", PLATFORM_CASES, ids=[c[0] for c in PLATFORM_CASES])
def test_reference_alone_flip_rate(rtsr, orc, case):
    """O2f built with glibc's sinf cosf logf acosf atan2f against O2f built with those five computed in double and rounded:
    the share of unequal pixels at the GPU tests' own frames is what REFERENCE_ALONE_UNEQUAL records, and it stays below the
    2 % at which a scene would need a smaller depth or another seed."""
    name, spp = case[0], case[4]
    b, flat, cam, cfg = setup_case(rtsr, case)
    h = rtsr.image_height(cfg)
    f, _ = orc.o2f_render(flat.arrays_ptr(), cam, cfg, h, threads=16)
    g, _ = orc.o2f_render(flat.arrays_ptr(), cam, cfg, h, threads=16, via_f64=True)
    unequal = int((~pixels_equal(g, f, spp)).sum())
    print("%s: %d of %d pixels unequal between the two CPU builds (%d bit-different)" % (name, unequal, f.shape[0] * f.shape[1],
                                                                                       int((f != g).any(axis=2).sum())))
    assert unequal == REFERENCE_ALONE_UNEQUAL[name]
    assert unequal <= 0.02 * f.shape[0] * f.shape[1]
    assert cap_pixels(name, f.shape[0] * f.shape[1]) >= 5


@pytest.mark.parametrize("case", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_exact_tier_scenes_do_not_depend_on_the_platform_functions(rtsr, orc, case):
    """The rule of test_gpu_f32_parity's tier A, checked where it can be: swapping the five platform functions for another
    faithful implementation changes no bit of these frames."""
    b, flat, cam, cfg = setup_case(rtsr, case)
    h = rtsr.image_height(cfg)
    f, rf = orc.o2f_render(flat.arrays_ptr(), cam, cfg, h, threads=16)
    g, rg = orc.o2f_render(flat.arrays_ptr(), cam, cfg, h, threads=16, via_f64=True)
    assert np.array_equal(f, g) and np.array_equal(rf, rg)


# ---- the float building blocks on the host -----------------------------------------------------------------------------------
def test_host_rng_forms_equal_numpy_restatements(orc):
    f = np.float32
    m = np.arange(1 << 24, dtype=np.uint64)
    raw = (m << np.uint64(40)) | ((m * np.uint64(0x9E3779B97F4A7C15)) & np.uint64((1 << 40) - 1))
    assert np.array_equal(orc.core32_math("rng_f32", raw.view(np.float64)), m.astype(np.float64) * 2.0 ** -24)
    mant = (raw >> np.uint64(41)).astype(np.uint32)
    got = orc.core32_math("rng_range_pm1_f32", raw.view(np.float64)).astype(f)
    assert np.array_equal(got.view(np.uint32), ((mant | np.uint32(0x40000000)).view(f) + f(-3.0)).view(np.uint32))
    for lo, hi in ((-1.0, 1.0), (0.5, 1.0), (0.0, 165.0)):
        lohi = np.full(raw.size, np.uint64(f(lo).view(np.uint32)) | (np.uint64(f(hi).view(np.uint32)) << np.uint64(32)), dtype=np.uint64)
        got = orc.core32_math("rng_range_f32", raw.view(np.float64), lohi.view(np.float64)).astype(f)
        scale = f(hi) - f(lo)
        want = (mant | np.uint32(0x3F800000)).view(f) * scale + (f(lo) - scale)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (lo, hi)


def test_host_slope_cap_handles_nan_and_infinities_like_v_med3(orc):
    """core/cull32.hpp's replacement of a slope that is not finite by +-2^60 (finite slopes stay, however steep), on the host, on
    the inputs where it could part from the device: +-0, NaN, +-inf, denormals, 2^-60, 2^-61, 2^-100;
    tests/test_gpu_f32_parity.py holds the device to the same table."""
    from test_gpu_f32_parity import SLOPE_CAP_IN, SLOPE_CAP_OUT
    got = orc.core32_math("slope_capf", SLOPE_CAP_IN).astype(np.float32)
    assert got.view(np.uint32).tolist() == np.float32(SLOPE_CAP_OUT).view(np.uint32).tolist()


# ---- the three hazards of single-precision rays ------------------------------------------------------------------
def test_hazard_zero_direction_component(rtsr, orc):
    """A direction component of exactly 0: the slope is capped at 2^60 (finite), the axis stays out of the error term, and
    the ray is still culled and still hits what the double oracle hits."""
    q = orc.core32_ray32((13.0, 2.0, 3.0), (0.0, -1.0, 0.25))
    assert q["ix"] == 2.0 ** 60 and np.isfinite(q["oix"]) and np.isfinite(q["err2"]) and q["err2"] < 1e-3
    q = orc.core32_ray32((13.0, 2.0, 3.0), (-0.0, -1.0, 0.0))
    assert q["ix"] == -2.0 ** 60 and q["iz"] == 2.0 ** 60 and np.isfinite(q["err2"])
    for sid, opts, o in ((100, {}, (4.0, 6.0, 0.5)), (11, {"mesh_triangles": 2000}, None), (4, {}, (278.0, 278.0, -800.0))):
        b = rtsr.Builder(1)
        world, cam, bg = b.get_world_cam(sid, **opts)
        flat = b.flatten(world)
        o = o if o is not None else tuple(cam.origin)
        n_hit = 0
        for d in ((0.0, -1.0, 0.0), (0.0, -1.0, 0.125), (0.0, 0.0, 1.0), (0.25, -1.0, 0.0), (0.0, -0.5, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 0.25, 1.0),
                  (0.25, 0.0, 1.0)):
            h64 = orc.core_world_hit(flat.arrays_ptr(), o, d)
            h32 = orc.core32_world_hit(flat.arrays_ptr(), o, d)
            assert (h64 is None) == (h32 is None), (sid, d)
            if h64 is not None:
                n_hit += 1
                assert abs(h32["t"] - h64["t"]) <= 1e-4 * abs(h64["t"]) + 1e-3, (sid, d, h32["t"], h64["t"])
        assert n_hit >= 2, sid


def test_hazard_shallow_exit_from_the_ground_sphere(rtsr, orc):
    """A ray leaving the r = 1000 ground sphere of Book-1 at a shallow angle from a single-precision hit point must not find
    that sphere again a hair's breadth away: no hit below t = 0.5 over a sweep of hit points and grazing angles (the scene's
    other spheres are far from these points)."""
    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(100)
    flat = b.flatten(world)
    rng = np.random.default_rng(5)
    n_checked = 0
    for _ in range(1500):
        r, phi = rng.uniform(20.0, 600.0), rng.uniform(0, 2 * np.pi)
        x, z = r * np.cos(phi), r * np.sin(phi)
        down = orc.core32_world_hit(flat.arrays_ptr(), (x, 50.0, z), (0.0, -1.0, 0.0))   # a single-precision point on the ground
        assert down is not None and down["p"][1] <= 0.0
        p, n = np.array(down["p"]), np.array(down["normal"])
        t = np.cross(n, rng.normal(size=3))
        t /= np.linalg.norm(t)
        d = t + n * 10.0 ** rng.uniform(-6, -1.5)   # grazing: 1e-6 .. 3e-2 of the way up
        hit = orc.core32_world_hit(flat.arrays_ptr(), p, d)
        assert hit is None or hit["t"] > 0.5, (tuple(p), tuple(d), hit)
        n_checked += 1
    assert n_checked == 1500


def test_hazard_non_finite_ray_ends_its_path(orc):
    fin = ((1.0, 2.0, 3.0), (0.0, -1.0, 0.5))
    assert not orc.core32_path_ends(*fin, depth=50)
    assert orc.core32_path_ends(*fin, depth=0)          # the depth rule itself
    for bad in (np.nan, np.inf, -np.inf, 1e39):         # 1e39 narrows to inf
        for k in range(3):
            o, d = list(fin[0]), list(fin[1])
            o[k] = bad
            assert orc.core32_path_ends(o, fin[1], depth=50), (bad, k)
            d[k] = bad
            assert orc.core32_path_ends(fin[0], d, depth=50), (bad, k)
