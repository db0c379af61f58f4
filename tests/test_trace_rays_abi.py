"""Radiance queries' C ABI and Python surface, and their judge, without a GPU: struct layout and defaults, the argument checks
of rtx_scene_trace_rays / rtx_scene_trace_rays_device (which return before any device call), Scene.trace_rays' own checks, and
the host checker (tests/rays_host_check.cpp) held to closed forms, to its own splitting rule, to the input condition of the GPU
test's estimator comparison, and to a sanitizer run as a stand-alone program."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cast_rays_cases as cc
import trace_rays_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rtx_radiance_rays_defaults", "rtx_scene_trace_rays", "rtx_scene_trace_rays_device"]


@pytest.fixture(scope="module")
def chk(orc, tmp_path_factory):
    return tc.checkers(tmp_path_factory)


def test_symbols_are_declared_exported_and_bound(rtsr):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx_abi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(rtsr.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in rtsr.ABI, name
    blob = open(rtsr.LIB_PATH, "rb").read()
    assert b"_ZN3rtx12k_trace_rays" in blob and b"_ZN5rtx3212k_trace_rays" in blob  # both compilations carry the kernel
    assert "RTX_TRACE_HOST_SLICE 262144" in text and re.search(r"RTX_KERNEL_RAYS = 9\b", text)
    assert rtsr.RTX_KERNEL_RAYS == 9 and rtsr.trace_kernel_name(9) == "k_trace_rays"


def test_struct_layout_and_defaults(rtsr):
    q = rtsr.RtxRadianceRays
    assert C.sizeof(q) == 104
    assert [(n, getattr(q, n).offset) for n, _ in q._fields_] == [
        ("n", 0), ("origin", 8), ("direction", 16), ("time", 24), ("first_ray", 32), ("first_sample", 40), ("samples", 44),
        ("max_depth", 48), ("accumulate", 52), ("seed", 56), ("background", 64), ("light_sampling", 88), ("reserved", 92),
        ("sample_buffer_bytes", 96)]
    r = q(7, 1, 2, 3, 4, 5, 6, 7, 1, 9, (1.0, 2.0, 3.0), 1, 5, 99)
    rtsr.lib.rtx_radiance_rays_defaults(C.byref(r))
    assert (r.n, r.origin, r.direction, r.time, r.first_ray, r.first_sample, r.accumulate) == (0, None, None, None, 0, 0, 0)
    assert (r.samples, r.max_depth, r.seed, tuple(r.background)) == (1, 50, 1, (0.7, 0.8, 1.0))
    assert (r.light_sampling, r.reserved, r.sample_buffer_bytes) == (0, 0, 0)
    rtsr.lib.rtx_radiance_rays_defaults(None)  # a no-op


def _query(rtsr, **kw):
    q = rtsr.RtxRadianceRays()
    rtsr.lib.rtx_radiance_rays_defaults(C.byref(q))
    o = np.zeros((4, 3))
    q.n, q.origin, q.direction = 4, o.ctypes.data, o.ctypes.data
    for k, v in kw.items():
        if k == "background":
            q.background[:] = v
        else:
            setattr(q, k, v)
    return q, o


@pytest.mark.parametrize("entry", ["rtx_scene_trace_rays", "rtx_scene_trace_rays_device"])
def test_argument_errors_before_any_device_call(rtsr, entry):
    fn = getattr(rtsr.lib, entry)
    call = (lambda s, q, S, Q: fn(s, q, S, Q, None, None)) if entry.endswith("_device") else (lambda s, q, S, Q: fn(s, q, S, Q, None))
    bogus = C.c_void_p(1)  # never dereferenced: every case below is refused by the argument checks
    sums = np.zeros((4, 3))
    S = sums.ctypes.data
    good, keep = _query(rtsr)
    cases = [(None, C.byref(good), S, "scene"), (bogus, None, S, "rays"), (bogus, C.byref(good), None, "sum_rgb")]
    for field, kw in (("n", {"n": -1}), ("origin", {"origin": None}), ("direction", {"direction": None}),
                      ("samples", {"samples": 0}), ("samples", {"samples": -3}), ("max_depth", {"max_depth": 0}),
                      ("reserved", {"reserved": 1}), ("light_sampling", {"light_sampling": 2}),
                      ("light_sampling", {"light_sampling": -1}), ("accumulate", {"accumulate": 2}),
                      ("background", {"background": (0.1, math.nan, 0.2)}), ("background", {"background": (math.nan, 0.0, 0.0)}),
                      ("first_sample", {"first_sample": 2 ** 32 - 1, "samples": 2})):
        bad, _ = _query(rtsr, **kw)
        cases.append((bogus, C.byref(bad), S, field))
    for s, q, sp, field in cases:
        assert call(s, q, sp, None) == rtsr.RTX_EINVAL, field
        msg = rtsr.last_error()
        assert entry + ":" in msg and field in msg, (field, msg)
    # the last sample index 2^32 - 1 itself is legal; n = 0 is legal whatever the ray pointers are: RTX_OK, nothing launched
    edge, _ = _query(rtsr, n=0, origin=None, direction=None, first_sample=2 ** 32 - 1, samples=1)
    assert call(bogus, C.byref(edge), S, None) == rtsr.RTX_OK
    before = sums.copy()
    empty, _ = _query(rtsr, n=0, origin=None, direction=None)
    assert call(bogus, C.byref(empty), S, S) == rtsr.RTX_OK and np.array_equal(sums, before)


def test_device_entry_names_a_misaligned_pointer(rtsr):
    bogus = C.c_void_p(1)
    sums = np.zeros((5, 3))
    S = sums.ctypes.data
    good, keep = _query(rtsr)
    fn = rtsr.lib.rtx_scene_trace_rays_device
    for field, args in (("sum_rgb", (S + 4, None)), ("sumsq_rgb", (S, S + 2))):
        assert fn(bogus, C.byref(good), args[0], args[1], None, None) == rtsr.RTX_EINVAL, field
        msg = rtsr.last_error()
        assert "rtx_scene_trace_rays_device:" in msg and field in msg and "aligned" in msg, (field, msg)
    for field in ("origin", "direction", "time"):
        bad, _ = _query(rtsr, **{field: keep.ctypes.data + 4})
        assert fn(bogus, C.byref(bad), S, None, None, None) == rtsr.RTX_EINVAL, field
        assert "rays->" + field in rtsr.last_error() and "aligned" in rtsr.last_error()


def test_python_rejects_bad_arguments(rtsr):
    s = object.__new__(rtsr.Scene)  # owns no handle: Scene.trace_rays checks its arguments before it touches the handle
    s._p = None
    o, d = np.zeros((8, 3)), np.ones((8, 3))
    other = rtsr.RadianceSums(7, 2, np.zeros((7, 3)), None)
    mine = rtsr.RadianceSums(8, 2, np.zeros((8, 3)), None)
    bad = [
        ("origins", dict(origins=o.astype(np.float32), directions=d)),
        ("directions", dict(origins=o, directions=np.asfortranarray(d))),
        ("directions", dict(origins=o, directions=np.ones((7, 3)))),
        ("times", dict(origins=o, directions=d, times=np.zeros(9))),
        ("times", dict(origins=o, directions=d, times=np.zeros((8, 1)))),
        ("origins", dict(origins=[[0.0, 0.0, 0.0]] * 8, directions=d)),
        ("spp", dict(origins=o, directions=d, spp=0)),
        ("spp", dict(origins=o, directions=d, spp=1.5)),
        ("max_depth", dict(origins=o, directions=d, max_depth=0)),
        ("first_sample", dict(origins=o, directions=d, first_sample=-1)),
        ("first_sample", dict(origins=o, directions=d, first_sample=2 ** 32 - 1, spp=2)),
        ("first_ray", dict(origins=o, directions=d, first_ray=-2)),
        ("background", dict(origins=o, directions=d, background=(0.0, math.nan, 0.0))),
        ("background", dict(origins=o, directions=d, background=(0.0, 1.0))),
        ("out", dict(origins=o, directions=d, out=np.zeros((8, 3)))),
        ("out", dict(origins=o, directions=d, out=other, first_sample=2)),      # another batch's sums
        ("out", dict(origins=o, directions=d, out=mine, first_sample=0)),       # first_sample must be out.spp
        ("out", dict(origins=o, directions=d, out=mine, first_sample=2, sumsq=True)),  # no sumsq to continue
    ]
    for name, kw in bad:
        with pytest.raises(ValueError) as e:
            s.trace_rays(**kw)
        assert str(e.value).startswith(name + ":"), (name, str(e.value))


# ---- the judge alone
def test_checker_empty_world_is_the_background(rtsr, orc, chk):
    b = rtsr.Builder(1)
    world, cam, _ = b.get_world_cam(rtsr.SCENE_EMPTY)
    flat = b.flatten(world)
    o, d = cc.sphere_rays(300, 3, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 2.0)
    bg = np.array([0.25, 0.5, 3.0])
    for nee in (False, True):
        S, Q = tc.host_trace(chk, flat, o, d, spp=5, background=bg, light_sampling=nee)
        assert np.array_equal(S, np.tile(5 * bg, (300, 1)))  # (sums of 5 equal terms of these values are exact)
        assert np.array_equal(Q, np.tile(5 * bg * bg, (300, 1)))


def test_checker_depth_one_is_background_or_first_hit_emission(rtsr, orc, chk):
    """max_depth = 1 on the Cornell box (no medium): a ray's every sample is the background where oracle_core_world_hit misses
    and the material's emission at the first hit where it hits -- (15, 15, 15) on the ceiling light (the only emitter: the
    rectangle y = 554, 213 <= x <= 343, 227 <= z <= 332), 0 elsewhere."""
    b = rtsr.Builder(1)
    world, cam, _ = b.get_world_cam(rtsr.SCENE_CORNELL_BOX)
    flat = b.flatten(world)
    o, d = cc.sphere_rays(1500, 5, (-250.0, -250.0, -250.0), (805.0, 805.0, 805.0), 0.9)
    # a fan from inside the room towards the ceiling, so that some first hits are on the light
    o2 = np.tile([278.0, 100.0, 278.0], (300, 1))
    d2 = np.column_stack([np.linspace(-150.0, 150.0, 300), np.full(300, 454.0), np.linspace(120.0, -90.0, 300)])
    o, d = np.ascontiguousarray(np.concatenate([o, o2])), np.ascontiguousarray(np.concatenate([d, d2]))
    bg = np.array([0.7, 0.8, 1.0])
    expect = np.zeros((len(o), 3))
    n_miss = n_light = 0
    for r in range(len(o)):
        rec = orc.core_world_hit(flat.arrays_ptr(), tuple(o[r]), tuple(d[r]))
        if rec is None:
            expect[r] = 3 * bg
            n_miss += 1
        else:
            x, y, z = rec["p"]
            if abs(y - 554.0) < 1e-9 and 213.0 <= x <= 343.0 and 227.0 <= z <= 332.0:
                expect[r] = 45.0
                n_light += 1
    print("depth 1: %d rays, %d miss, %d end on the light" % (len(o), n_miss, n_light))
    assert n_miss >= 100 and n_light >= 20
    S, _ = tc.host_trace(chk, flat, o, d, spp=3, max_depth=1, background=bg)
    assert np.array_equal(S, expect)


@pytest.mark.parametrize("name,nee", [("cornell_smoke", False), ("cornell_smoke", True), ("book2", False)])
def test_checker_sums_do_not_depend_on_the_cut(rtsr, orc, chk, name, nee):
    c = tc.case(rtsr, orc, name)
    n = 600
    o, d, t = c.o[:n], c.d[:n], c.time[:n]
    kw = dict(light_sampling=nee)
    S, Q = tc.host_trace(chk, c.flat, o, d, t, spp=4, first_ray=11, **kw)
    S2, Q2 = np.zeros((n, 3)), np.zeros((n, 3))
    for lo, hi in ((0, 130), (130, 385), (385, n)):
        part = tc.host_trace(chk, c.flat, o[lo:hi], d[lo:hi], t[lo:hi], spp=3, first_ray=11 + lo, **kw)
        part = tc.host_trace(chk, c.flat, o[lo:hi], d[lo:hi], t[lo:hi], spp=1, first_sample=3, first_ray=11 + lo, into=part, **kw)
        S2[lo:hi], Q2[lo:hi] = part
    assert tc.same_bits(S, S2).all() and tc.same_bits(Q, Q2).all()
    # and the key is what the contract says: another first_ray gives other sums
    S3, _ = tc.host_trace(chk, c.flat, o, d, t, spp=4, first_ray=12, **kw)
    assert not tc.same_bits(S, S3).all()


def test_checker_meets_the_estimator_agreement_condition(rtsr, orc, chk):
    """The input condition of the GPU test: on Cornell smoke's 2000 rays at 64 spp, depth 8, the two estimators' batch-mean
    radiance differ by at most 4 combined standard errors per channel -- by the reference alone."""
    c = tc.case(rtsr, orc, "cornell_smoke")
    cc.check_mix(c.name, c.first_hits)
    stats = [tc.batch_mean_and_se(*tc.host_trace(chk, c.flat, c.o, c.d, c.time, spp=64, light_sampling=nee), 64) for nee in (False, True)]
    (m0, e0), (m1, e1) = stats
    se = np.sqrt(e0 * e0 + e1 * e1)
    print("means %s / %s, combined SE %s, difference in SE %s" % (m0, m1, se, np.abs(m0 - m1) / se))
    assert np.all(m0 > 0) and np.all(se > 0)
    assert np.all(np.abs(m0 - m1) <= 4.0 * se)


def test_light_sampling_case_has_a_sphere_light(rtsr, orc):
    c = tc.case(rtsr, orc, "simple_light")
    cc.check_mix(c.name, c.first_hits)
    assert c.flat.lights()["n_sphere_lights"] >= 1
    assert tc.case(rtsr, orc, "book1").flat.lights()["n_lights"] == 0


def test_checker_runs_clean_under_the_sanitizers(tmp_path):
    """The checker plus its own main (two catalogue scenes, both estimators, a split batch) as a stand-alone program built with
    AddressSanitizer and UndefinedBehaviorSanitizer, run as its own process."""
    exe = str(tmp_path / "rays_host_check_san")
    subprocess.run(["g++"] + tc.SANFLAGS + ["-DRAYS_HOST_MAIN", tc.SRC] + tc.HOST_SOURCES + ["-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "sanitizer run clean" in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
