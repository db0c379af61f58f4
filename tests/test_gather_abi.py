"""Gather queries' C ABI and Python surface, and their judge, without a GPU: struct layout and defaults, the argument checks of
rtx_scene_gather / rtx_scene_gather_device (which return before any device call), Scene.gather's own checks,
rtx_gather_directions, and the host checker (tests/gather_host_check.cpp) held to closed forms, to its own splitting rule, to
every statistical condition of the GPU test, and to a sanitizer run as a stand-alone program."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import gather_cases as gc
import trace_rays_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rtx_gather_points_defaults", "rtx_scene_gather", "rtx_scene_gather_device", "rtx_gather_directions"]


@pytest.fixture(scope="module")
def chk(orc, tmp_path_factory):
    return gc.checkers(tmp_path_factory)


def test_symbols_are_declared_exported_and_bound(rtsr):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx_abi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(rtsr.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in rtsr.ABI, name
    blob = open(rtsr.LIB_PATH, "rb").read()
    for kernel in (b"8k_gather", b"19k_reduce_samples_sh"):  # both compilations carry the kernels
        assert b"_ZN3rtx" + kernel in blob and b"_ZN5rtx32" + kernel in blob, kernel
    assert callable(rtsr.Scene.gather) and callable(rtsr.gather_directions)


def test_struct_layout_and_defaults(rtsr):
    q = rtsr.RtxGatherPoints
    assert C.sizeof(q) == 112
    assert [(n, getattr(q, n).offset) for n, _ in q._fields_] == [
        ("n", 0), ("position", 8), ("normal", 16), ("time", 24), ("first_point", 32), ("first_sample", 40), ("samples", 44),
        ("max_depth", 48), ("accumulate", 52), ("seed", 56), ("background", 64), ("light_sampling", 88), ("sh_order", 92),
        ("sample_buffer_bytes", 96), ("reserved", 104)]
    r = q(7, 1, 2, 3, 4, 5, 6, 7, 1, 9, (1.0, 2.0, 3.0), 1, 2, 99, (5, 6))
    rtsr.lib.rtx_gather_points_defaults(C.byref(r))
    assert (r.n, r.position, r.normal, r.time, r.first_point, r.first_sample, r.accumulate) == (0, None, None, None, 0, 0, 0)
    assert (r.samples, r.max_depth, r.seed, tuple(r.background)) == (1, 50, 1, (0.7, 0.8, 1.0))
    assert (r.light_sampling, r.sh_order, r.sample_buffer_bytes, tuple(r.reserved)) == (0, 0, 0, (0, 0))
    rtsr.lib.rtx_gather_points_defaults(None)  # a no-op


def _query(rtsr, **kw):
    q = rtsr.RtxGatherPoints()
    rtsr.lib.rtx_gather_points_defaults(C.byref(q))
    o = np.zeros((4, 3))
    q.n, q.position = 4, o.ctypes.data
    for k, v in kw.items():
        if k == "background":
            q.background[:] = v
        elif k == "reserved":
            q.reserved[:] = v
        else:
            setattr(q, k, v)
    return q, o


@pytest.mark.parametrize("entry", ["rtx_scene_gather", "rtx_scene_gather_device"])
def test_argument_errors_before_any_device_call(rtsr, entry):
    fn = getattr(rtsr.lib, entry)
    call = (lambda s, q, S, Q: fn(s, q, S, Q, None, None)) if entry.endswith("_device") else (lambda s, q, S, Q: fn(s, q, S, Q, None))
    bogus = C.c_void_p(1)  # never dereferenced: every case below is refused by the argument checks
    sums = np.zeros((4, 9, 3))
    S = sums.ctypes.data
    good, keep = _query(rtsr)
    cases = [(None, C.byref(good), S, "scene"), (bogus, None, S, "points"), (bogus, C.byref(good), None, "sum")]
    for field, kw in (("n", {"n": -1}), ("position", {"position": None}),
                      ("samples", {"samples": 0}), ("samples", {"samples": -3}), ("max_depth", {"max_depth": 0}),
                      ("reserved", {"reserved": (1, 0)}), ("reserved", {"reserved": (0, 7)}),
                      ("light_sampling", {"light_sampling": 2}), ("light_sampling", {"light_sampling": -1}),
                      ("accumulate", {"accumulate": 2}), ("accumulate", {"accumulate": -1}),
                      ("sh_order", {"sh_order": 3}), ("sh_order", {"sh_order": -1}),
                      ("sh_order", {"sh_order": 1, "normal": keep.ctypes.data}), ("sh_order", {"sh_order": 2, "normal": keep.ctypes.data}),
                      ("background", {"background": (0.1, math.nan, 0.2)}), ("background", {"background": (math.nan, 0.0, 0.0)}),
                      ("first_sample", {"first_sample": 2 ** 32 - 1, "samples": 2})):
        bad, _ = _query(rtsr, **kw)
        cases.append((bogus, C.byref(bad), S, field))
    for s, q, sp, field in cases:
        assert call(s, q, sp, None) == rtsr.RTX_EINVAL, field
        msg = rtsr.last_error()
        assert entry + ":" in msg and field in msg, (field, msg)
    # the last sample index 2^32 - 1 itself is legal; n = 0 is legal whatever the point pointers are: RTX_OK, nothing launched
    edge, _ = _query(rtsr, n=0, position=None, first_sample=2 ** 32 - 1, samples=1)
    assert call(bogus, C.byref(edge), S, None) == rtsr.RTX_OK
    before = sums.copy()
    for kw in ({}, {"sh_order": 2}, {"normal": 8}):
        empty, _ = _query(rtsr, n=0, position=None, **kw)
        assert call(bogus, C.byref(empty), S, S) == rtsr.RTX_OK and np.array_equal(sums, before)


def test_device_entry_names_a_misaligned_pointer(rtsr):
    bogus = C.c_void_p(1)
    sums = np.zeros((5, 3))
    S = sums.ctypes.data
    good, keep = _query(rtsr)
    fn = rtsr.lib.rtx_scene_gather_device
    for field, args in (("sum", (S + 4, None)), ("sumsq", (S, S + 2))):
        assert fn(bogus, C.byref(good), args[0], args[1], None, None) == rtsr.RTX_EINVAL, field
        msg = rtsr.last_error()
        assert "rtx_scene_gather_device:" in msg and field in msg and "aligned" in msg, (field, msg)
    for field in ("position", "normal", "time"):
        bad, _ = _query(rtsr, **{field: keep.ctypes.data + 4})
        assert fn(bogus, C.byref(bad), S, None, None, None) == rtsr.RTX_EINVAL, field
        assert "points->" + field in rtsr.last_error() and "aligned" in rtsr.last_error()


def test_python_rejects_bad_arguments(rtsr):
    s = object.__new__(rtsr.Scene)  # owns no handle: Scene.gather checks its arguments before it touches the handle
    s._p = None
    p, nn = np.zeros((8, 3)), np.ones((8, 3))
    other = rtsr.GatherSums(7, 2, np.zeros((7, 3)), None, True, 0)
    mine = rtsr.GatherSums(8, 2, np.zeros((8, 3)), None, True, 0)
    probe = rtsr.GatherSums(8, 2, np.zeros((8, 4, 3)), None, False, 1)
    bad = [
        ("points", dict(points=p.astype(np.float32))),
        ("points", dict(points=[[0.0, 0.0, 0.0]] * 8)),
        ("points", dict(points=np.zeros((8, 2)))),
        ("normals", dict(points=p, normals=np.asfortranarray(nn))),
        ("normals", dict(points=p, normals=np.ones((7, 3)))),
        ("times", dict(points=p, times=np.zeros(9))),
        ("times", dict(points=p, times=np.zeros((8, 1)))),
        ("spp", dict(points=p, spp=0)),
        ("spp", dict(points=p, spp=1.5)),
        ("max_depth", dict(points=p, max_depth=0)),
        ("first_sample", dict(points=p, first_sample=-1)),
        ("first_sample", dict(points=p, first_sample=2 ** 32 - 1, spp=2)),
        ("first_point", dict(points=p, first_point=-2)),
        ("sh_order", dict(points=p, sh_order=3)),
        ("sh_order", dict(points=p, normals=nn, sh_order=1)),
        ("background", dict(points=p, background=(0.0, math.nan, 0.0))),
        ("background", dict(points=p, background=(0.0, 1.0))),
        ("stream", dict(points=p, stream=5)),                                   # numpy arrays take the blocking host entry
        ("out", dict(points=p, normals=nn, out=np.zeros((8, 3)))),
        ("out", dict(points=p, normals=nn, out=other, first_sample=2)),         # another batch's sums
        ("out", dict(points=p, normals=nn, out=mine, first_sample=0)),          # first_sample must be out.spp
        ("out", dict(points=p, out=mine, first_sample=2)),                      # surface sums, a probe call
        ("out", dict(points=p, sh_order=2, out=probe, first_sample=2)),         # another order's sums
    ]
    for name, kw in bad:
        with pytest.raises(ValueError) as e:
            s.gather(**kw)
        assert str(e.value).startswith(name + ":"), (name, str(e.value))
    for name, kw in (("n", dict(n=-1)), ("spp", dict(n=4, spp=0)), ("normals", dict(n=4, normals=np.ones((3, 3)))),
                     ("first_sample", dict(n=4, first_sample=2 ** 32 - 1, spp=2))):
        with pytest.raises(ValueError) as e:
            rtsr.gather_directions(**kw)
        assert str(e.value).startswith(name + ":"), (name, str(e.value))
    sums = rtsr.GatherSums(2, 4, np.full((2, 3), 8.0), None, True, 0)
    assert sums.form == "surface" and sums.sh is None and np.array_equal(sums.mean, np.full((2, 3), 2.0))
    assert np.array_equal(sums.irradiance, np.full((2, 3), 8.0) * (np.pi / 4))
    assert probe.form == "probe" and probe.irradiance is None and probe.sh.shape == (8, 4, 3)


# ---- rtx_gather_directions
def test_directions_are_the_stated_rule(rtsr):
    """Probe directions are unit vectors (the reference's rejection loop, normalised); surface directions are normal + that
    same unit vector, with the normal taken as given; a range is cut by first_point and first_sample without changing a
    direction; the float arithmetic gives the float neighbours of the f64 directions; errors name the field."""
    n, spp = 37, 5
    u = rtsr.gather_directions(n, spp=spp, seed=9, first_point=3, first_sample=2)
    assert u.shape == (n, spp, 3) and np.abs(np.linalg.norm(u, axis=2) - 1.0).max() < 1e-15
    assert abs(u.mean()) < 0.1 and len(np.unique(u.reshape(-1, 3), axis=0)) == n * spp
    normals = np.ascontiguousarray(np.random.default_rng(2).normal(size=(n, 3)) * 3.0)
    d = rtsr.gather_directions(n, normals, spp=spp, seed=9, first_point=3, first_sample=2)
    assert np.array_equal(d, normals[:, None, :] + u)  # one separately rounded add per component
    part = rtsr.gather_directions(10, np.ascontiguousarray(normals[20:30]), spp=2, seed=9, first_point=23, first_sample=4)
    assert np.array_equal(part, d[20:30, 2:4])
    assert not np.array_equal(rtsr.gather_directions(n, spp=spp, seed=10, first_point=3, first_sample=2), u)
    u32 = rtsr.gather_directions(n, spp=spp, seed=9, first_point=3, first_sample=2, f32=True)
    assert np.array_equal(u32, u32.astype(np.float32).astype(np.float64)) and np.abs(u32 - u).max() < 1e-6
    assert rtsr.gather_directions(0).shape == (0, 1, 3)
    q, _ = _query(rtsr)
    out = np.zeros((4, 1, 3))
    for field, args in (("points", (None, 0, out.ctypes.data)), ("dir", (C.byref(q), 0, None)), ("f32", (C.byref(q), 2, out.ctypes.data))):
        assert rtsr.lib.rtx_gather_directions(*args) == rtsr.RTX_EINVAL
        assert "rtx_gather_directions:" in rtsr.last_error() and field in rtsr.last_error()
    for field, kw in (("n", {"n": -1}), ("samples", {"samples": 0}), ("first_sample", {"first_sample": 2 ** 32 - 1, "samples": 2})):
        bad, _ = _query(rtsr, **kw)
        assert rtsr.lib.rtx_gather_directions(C.byref(bad), 0, out.ctypes.data) == rtsr.RTX_EINVAL and field in rtsr.last_error()


# ---- the judge alone
def test_checker_empty_world_is_the_background(rtsr, orc, chk):
    """Every sample is the background exactly: plain sums are samples * background, and the SH sums equal sum_s Y_i(dir_s) * bg
    recomputed in numpy, in the stated order, from rtx_gather_directions."""
    b = rtsr.Builder(1)
    world, cam, _ = b.get_world_cam(rtsr.SCENE_EMPTY)
    flat = b.flatten(world)
    n, spp = 300, 5
    p = np.random.default_rng(4).uniform(-2.0, 2.0, (n, 3))
    nrm = np.random.default_rng(5).normal(size=(n, 3))
    bg = np.array([0.25, 0.5, 3.0])
    for nee in (False, True):
        for normals in (None, nrm):
            S, Q = gc.host_gather(chk, flat, p, normals, spp=spp, background=bg, light_sampling=nee)
            assert np.array_equal(S, np.tile(5 * bg, (n, 1)))  # (sums of 5 equal terms of these values are exact)
            assert np.array_equal(Q, np.tile(5 * bg * bg, (n, 1)))
        for order in (1, 2):
            S, Q = gc.host_gather(chk, flat, p, spp=spp, background=bg, light_sampling=nee, sh_order=order, first_point=7, first_sample=3)
            d = rtsr.gather_directions(n, spp=spp, seed=gc.SEED, first_point=7, first_sample=3)
            S2, Q2 = gc.sh_sums_in_stated_order(d, np.broadcast_to(bg, (n, spp, 3)), order)
            assert S.shape == (n, (order + 1) ** 2, 3)
            assert gc.same_bits(S, S2).all() and gc.same_bits(Q, Q2).all()
            # and against the basis written from its definition: equal up to rounding
            assert np.abs(S - (gc.sh_basis(d)[:, :, :(order + 1) ** 2, None] * bg).sum(axis=1)).max() < 1e-13


def test_checker_f32_directions_enter_the_basis_widened(rtsr, orc, chk):
    b = rtsr.Builder(1)
    world, cam, _ = b.get_world_cam(rtsr.SCENE_EMPTY)
    flat = b.flatten(world)
    n, spp = 64, 3
    p = np.zeros((n, 3))
    bg = np.array([0.25, 0.5, 3.0])
    S, Q = gc.host_gather(chk, flat, p, spp=spp, background=bg, sh_order=2, f32=True)
    d = rtsr.gather_directions(n, spp=spp, seed=gc.SEED, f32=True)
    S2, Q2 = gc.sh_sums_in_stated_order(d, np.broadcast_to(bg, (n, spp, 3)), 2)
    assert gc.same_bits(S, S2).all() and gc.same_bits(Q, Q2).all()


@pytest.mark.parametrize("name,surface,nee,order", [("cornell_smoke", True, False, 0), ("cornell_smoke", True, True, 0),
                                                    ("cornell_smoke", False, True, 2), ("book2", False, False, 1)])
def test_checker_sums_do_not_depend_on_the_cut(rtsr, orc, chk, name, surface, nee, order):
    c = tc.case(rtsr, orc, name)
    n = 300
    p, nrm, t = gc.points_of(c, n)
    if not surface:
        nrm = None
    cut = lambda a, lo, hi: None if a is None else a[lo:hi]
    kw = dict(light_sampling=nee, sh_order=order)
    S, Q = gc.host_gather(chk, c.flat, p, nrm, t, spp=4, first_point=11, **kw)
    S2, Q2 = np.zeros_like(S), np.zeros_like(Q)
    for lo, hi in ((0, 70), (70, 193), (193, n)):
        part = gc.host_gather(chk, c.flat, p[lo:hi], cut(nrm, lo, hi), t[lo:hi], spp=3, first_point=11 + lo, **kw)
        part = gc.host_gather(chk, c.flat, p[lo:hi], cut(nrm, lo, hi), t[lo:hi], spp=1, first_sample=3, first_point=11 + lo, into=part, **kw)
        S2[lo:hi], Q2[lo:hi] = part
    assert gc.same_bits(S, S2).all() and gc.same_bits(Q, Q2).all()
    assert np.isfinite(S).all() and (S != 0).any()
    # and the key is what the contract says: another first_point gives other sums
    S3, _ = gc.host_gather(chk, c.flat, p, nrm, t, spp=4, first_point=12, **kw)
    assert not gc.same_bits(S, S3).all()


@pytest.mark.parametrize("name", list(gc.SURFACE_CASES))
def test_checker_meets_the_surface_closed_forms(rtsr, orc, chk, name):
    """The statistical conditions of the GPU test's surface cases, by the judge alone."""
    b, flat = gc.SURFACE_CASES[name].build(rtsr)
    lines, failed = gc.surface_check(name, gc.host_gatherer(chk, flat))
    print("\n".join(lines))
    assert not failed, failed


def test_checker_meets_the_probe_closed_form(rtsr, orc, chk):
    b, flat = gc.probe_scene(rtsr)
    lines, failed = gc.probe_check(gc.host_gatherer(chk, flat))
    print("\n".join(lines))
    assert not failed, failed


def test_closed_forms_are_what_they_say():
    """The expected values against brute-force quadrature in numpy: the form factor of the xz light at one point, and the
    projection of a cap onto the nine basis functions."""
    case = gc.SURFACE_CASES["xz"]
    L = case.lights[0]
    p = gc.FLOOR_POINTS[5]
    a0, a1, b0, b1 = L["ab"]
    m = 1500
    xs, zs = a0 + (np.arange(m) + 0.5) * (a1 - a0) / m, b0 + (np.arange(m) + 0.5) * (b1 - b0) / m
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    v = np.stack([X - p[0], np.full_like(X, L["k"] - p[1]), Z - p[2]], axis=-1)
    r2 = (v * v).sum(-1)
    F = ((v[..., 1] / np.sqrt(r2)) ** 2 / r2).sum() * (a1 - a0) * (b1 - b0) / (m * m) / np.pi
    assert abs(gc.surface_expected(case)[5, 0] / L["le"][0] - F) < 1e-5 * F
    d = np.array([0.3, -0.5, 0.81])
    d /= np.linalg.norm(d)
    c = 0.8
    k = 400000
    i = np.arange(k) + 0.5
    z, phi = 1.0 - 2.0 * i / k, np.pi * (1.0 + 5.0 ** 0.5) * i   # a Fibonacci lattice on the sphere
    w = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], axis=-1)
    inside = (w @ d) >= c
    quad = (gc.sh_basis(w) * inside[:, None]).sum(axis=0) * (4.0 * np.pi / k)
    assert np.abs(quad - gc.cap_coefficients([1.0, 1.0, 1.0], d, c)[:, 0]).max() < 2e-4
    # orthonormality of the restated basis
    G = gc.sh_basis(w).T @ gc.sh_basis(w) * (4.0 * np.pi / k)
    assert np.abs(G - np.eye(9)).max() < 1e-4


def test_checker_runs_clean_under_the_sanitizers(tmp_path):
    """The checker plus its own main (two catalogue scenes, both forms, both estimators, SH sums, a split batch) as a stand-alone
    program built with AddressSanitizer and UndefinedBehaviorSanitizer, run as its own process."""
    exe = str(tmp_path / "gather_host_check_san")
    subprocess.run(["g++"] + tc.SANFLAGS + ["-DGATHER_HOST_MAIN", gc.SRC] + tc.HOST_SOURCES + ["-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "sanitizer run clean" in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
