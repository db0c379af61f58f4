"""The inputs and the judge of occlusion queries, without a GPU (tests/occlusion_cases.py, tests/occlusion_host_check.cpp): the
judge's "blocked" against the oracle's hit flag on every media-free case, its optical depths against closed forms in numpy
longdouble, exp(-tau) against the share of the oracle's streams that report no hit, the input condition of the GPU test's
media ray set, and a sanitizer run of the judge as a stand-alone program."""
import subprocess

import numpy as np
import pytest

import cast_rays_cases as cc
import occlusion_cases as oc

# The largest relative error of the judge against the closed forms measured on the CPU (f64 judge, all closed-form cases of
# occlusion_cases.closed_form_cases): 4.5e-13, on fog_sphere_cut (t_max a few per cent of the chord behind the entry point: the
# difference t_max - rec1.t cancels; every other case stays below 1.2e-14).  The asserted bound is four times that.  Nothing
# here comes from a GPU result.
MEASURED_REL_ERR = 4.5e-13
REL_ERR_BOUND = 4.0 * MEASURED_REL_ERR


@pytest.fixture(scope="module")
def chk(orc, tmp_path_factory):
    return oc.checkers(tmp_path_factory)


# ---- consequence 1: on a world whose media cannot hit, blocked == the closest-hit walk's hit flag, ray for ray
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(oc.MEDIA_FREE))
def test_blocked_equals_the_oracles_hit_flag(rtsr, orc, chk, name, f32):
    """(The float oracle answers every 83rd ray of the two GravitySphere cases: occlusion_cases.GRAVITY_F32_STRIDE says why.)"""
    c = oc.case(rtsr, orc, name)
    rays = oc.oracle_rays(c, f32)
    hit = oc.oracle_hit_flags(orc, c, f32)
    if len(rays) == c.n:
        cc.check_mix(c.name + (" f32" if f32 else ""), hit.astype(np.float64).reshape(-1, 1))
    tau = oc.host_tau(chk, c.flat, c.o, c.d, c.time, c.t_max, f32=f32)
    assert not np.isnan(tau).any()
    tau = tau[rays]
    bad = np.flatnonzero(np.isinf(tau) != hit)
    assert len(bad) == 0, "%s: ray %d: tau %r, oracle hit %r" % (c.name, bad[0], tau[bad[0]], bool(hit[bad[0]]))
    # a ray that is not blocked is exactly clear: +0.0, whether the world has no medium or media of density 0
    clear = tau[~hit]
    assert np.all(clear == 0.0) and not np.signbit(clear).any()


# ---- closed forms
def test_depths_equal_the_closed_forms(rtsr, orc, chk):
    """Fog sphere: density x chord; fog box: density x slab length; two overlapping spheres: the sum; a start inside the fog;
    t_max inside the fog; a wall behind / in front of / inside the fog in either slot order: +inf; density 0: +0;
    Translate(RotateY(box)).  Largest relative error measured on the CPU: 4.5e-13 (MEASURED_REL_ERR); asserted: four times that."""
    worst = 0.0
    names = set()
    for c in oc.closed_form_cases(rtsr):
        tau = oc.host_tau(chk, c.flat, c.o, c.d, None, c.t_max, t_min=c.t_min)
        err, rest_equal = oc.relative_error(tau, c.expected)
        n_pos = int((np.isfinite(c.expected) & (c.expected > 0)).sum())
        print("%-40s %3d rays, %3d with a depth, %3d blocked, relative error %.3g" % (c.name, len(tau), n_pos, int(np.isinf(c.expected).sum()), err))
        assert rest_equal, c.name   # +inf where a wall blocks, +0.0 where nothing lies on the segment
        assert err <= REL_ERR_BOUND, (c.name, err)
        if c.name.startswith("wall_") and c.name != "wall_past_t_max":
            assert np.all(np.isposinf(tau))
        elif c.name != "fog_sphere_density0":
            assert 2 * n_pos >= len(tau), c.name  # the case is about depths: most rays have one
        worst = max(worst, err)
        names.add(c.name)
    print("largest relative error %.3g (bound %.3g)" % (worst, REL_ERR_BOUND))
    assert {"fog_sphere", "fog_box", "two_fog_spheres", "fog_sphere_from_inside", "fog_sphere_from_inside_t_min_behind",
            "fog_sphere_cut", "fog_sphere_density0", "fog_box_moved", "wall_past_t_max"} <= names
    assert {"wall_%s_%s" % (w, o) for w in ("behind", "in_front", "inside") for o in ("wall_first", "fog_first")} <= names


# ---- the media ray set of the GPU test, and consequence 2
def _media_set(rtsr, orc, chk):
    c = oc.case(rtsr, orc, "cornell_smoke")
    a, b = oc.segments()
    return c, a, b, oc.segment_tau(chk, c.flat, a, b)


def test_media_segments_meet_the_input_condition(rtsr, orc, chk):
    """2000 segments between uniform point pairs of a box a little larger than the Cornell room: by the judge alone at least
    10 % run through fog (0 < tau < inf), at least 10 % are blocked and at least 10 % are exactly clear."""
    c, a, b, tau = _media_set(rtsr, orc, chk)
    fog, blocked, clear = int(((tau > 0) & np.isfinite(tau)).sum()), int(np.isinf(tau).sum()), int((tau == 0).sum())
    print("media segments: %d through fog, %d blocked, %d clear of %d" % (fog, blocked, clear, len(tau)))
    assert fog + blocked + clear == len(tau) == 2000
    assert 10 * fog >= len(tau) and 10 * blocked >= len(tau) and 10 * clear >= len(tau)
    # the float judge sees the same three classes (not necessarily on the same rays at a grazing edge)
    tau32 = oc.segment_tau(chk, c.flat, a, b, f32=True)
    assert 10 * int(((tau32 > 0) & np.isfinite(tau32)).sum()) >= len(tau) and 10 * int(np.isinf(tau32).sum()) >= len(tau)


STREAMS = 4096


def _check_streams(orc, flat, a, b, tau, label, time=0.0):
    pick = np.flatnonzero(np.isfinite(tau) & (np.exp(-tau) > 0.05) & (np.exp(-tau) < 0.95))[:8]
    assert len(pick) == 8, (label, len(pick))
    for r in pick:
        p = float(np.exp(-tau[r]))
        share = oc.stream_miss_share(orc, flat, a[r], b[r], STREAMS, seed=1000 * int(r) + 1, time=time)
        se = np.sqrt(p * (1.0 - p) / STREAMS)
        print("%s segment %4d: tau %.6f, exp(-tau) %.4f, no-hit share %.4f, %.2f standard errors" % (label, r, tau[r], p, share, abs(share - p) / se))
        assert abs(share - p) <= 4.5 * se, (label, int(r), p, share)


def test_transmittance_is_the_share_of_streams_without_a_hit_cornell_smoke(rtsr, orc, chk):
    """8 segments through Cornell smoke's two fog boxes, no surface in the way by the judge: of 4096 streams of core_world_hit
    the share without any hit lies within 4.5 binomial standard errors of exp(-tau) (the margin of tests/light_cases.py)."""
    c, a, b, tau = _media_set(rtsr, orc, chk)
    assert len(oc.medium_slots(c.flat)) == 2
    _check_streams(orc, c.flat, a, b, tau, "cornell_smoke")


def test_transmittance_is_the_share_of_streams_without_a_hit_book2(rtsr, orc, chk):
    """The same through reduced Book-2's fog (the smoke ball inside the scene-wide mist: overlapping media, the product)."""
    c = oc.case(rtsr, orc, "book2")
    assert len(oc.medium_slots(c.flat)) == 2
    a, b = oc.segments(600, seed=22, lo=-100.0, hi=600.0)
    tau = oc.segment_tau(chk, c.flat, a, b, time=np.zeros(len(a)))
    _check_streams(orc, c.flat, a, b, tau, "book2")


# ---- the judge's own plumbing
def test_judge_time_limit_and_split(rtsr, orc, chk):
    """A ray later than the GravitySpheres' limit is NaN, one at the limit is tested; a batch cut in three equals the whole."""
    import trace_rays_cases as tc
    c = oc.case(rtsr, orc, "gravity_t0.37")
    limit = tc.gravity_time_limit()
    time = np.concatenate([np.full(4, limit), np.full(4, np.nextafter(limit, np.inf))])
    o, d = np.concatenate([c.o[:4], c.o[:4]]), np.concatenate([c.d[:4], c.d[:4]])
    tau = oc.host_tau(chk, c.flat, o, d, time)
    assert not np.isnan(tau[:4]).any() and np.isnan(tau[4:]).all()
    s = oc.case(rtsr, orc, "cornell_smoke")
    whole = oc.host_tau(chk, s.flat, s.o, s.d, s.time, s.t_max)
    parts = np.concatenate([oc.host_tau(chk, s.flat, s.o[lo:hi], s.d[lo:hi], s.time[lo:hi], s.t_max[lo:hi])
                            for lo, hi in ((0, 517), (517, 1300), (1300, s.n))])
    assert oc.same_bits(whole, parts).all()


def test_judge_runs_clean_under_the_sanitizers(tmp_path):
    """The judge plus its own main (two catalogue scenes, a split batch) as a stand-alone program built with AddressSanitizer
    and UndefinedBehaviorSanitizer, run as its own process."""
    exe = str(tmp_path / "occlusion_host_check_san")
    subprocess.run(["g++"] + oc.SANFLAGS + ["-DOCCLUSION_HOST_MAIN", oc.SRC] + oc.HOST_SOURCES + ["-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "sanitizer run clean" in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
