"""Radiance queries on the device (Scene.trace_rays, rtx_scene_trace_rays*): k_trace_rays gives the sums the host checker
(tests/rays_host_check.cpp) gives, bit for bit, however the batch is cut.

Every comparison is by bit pattern with NaN equal to NaN (cast_rays_cases.same_bits).  Scenes and rays: tests/cast_rays_cases.py
through tests/trace_rays_cases.py -- 2000 rays x 4 spp x depth 8 per case; the checker's sums are computed once per use."""
import numpy as np
import pytest

import cast_rays_cases as cc
import trace_rays_cases as tc

pytestmark = pytest.mark.gpu
_SCENES = {}
_PLAIN = {}


@pytest.fixture(scope="module")
def chk(orc, tmp_path_factory):
    return tc.checkers(tmp_path_factory)


def _case(rtsr, orc, name):
    c = tc.case(rtsr, orc, name)
    if name not in _SCENES:
        _SCENES[name] = c.flat.upload(f32=c.f32)
    return c, _SCENES[name]


def _trace(scene, c, n=None, **kw):
    n = c.n if n is None else n
    kw.setdefault("spp", tc.SPP)
    cut = lambda a: np.ascontiguousarray(a[:n])
    return scene.trace_rays(cut(c.o), cut(c.d), cut(c.time), max_depth=tc.DEPTH, background=tc.BACKGROUND, seed=tc.SEED, sumsq=True, **kw)


def _plain(rtsr, orc, name, spp):
    """One plain call over the case's whole batch at `spp` (default sample buffer, first_ray 0): what every cut is held to."""
    if (name, spp) not in _PLAIN:
        c, scene = _case(rtsr, orc, name)
        _PLAIN[name, spp] = _trace(scene, c, spp=spp)
    return _PLAIN[name, spp]


def _assert_same(what, got_S, got_Q, ref_S, ref_Q):
    bad = np.flatnonzero(~(tc.same_bits(got_S, ref_S) & tc.same_bits(got_Q, ref_Q)))
    print("%s: %d rays, %d differ" % (what, len(ref_S), len(bad)))
    assert len(bad) == 0, "%s: ray %d: got %r / %r, expected %r / %r" % (
        what, bad[0], got_S[bad[0]].tolist(), got_Q[bad[0]].tolist(), ref_S[bad[0]].tolist(), ref_Q[bad[0]].tolist())


# ---- 1. f64 against the checker
@pytest.mark.parametrize("name", tc.F64_CHECKED)
def test_f64_sums_equal_the_checker(rtsr, orc, chk, name):
    """sum and sumsq of every ray equal the checker's loop bit for bit.  Cornell smoke, Book-2 and moving_test run P_ANY, scene 8
    P_ALL, the zoo layouts P_INST; the media of the first two draw from the path's stream; Book-2's and moving_test's times lie
    in the shutter."""
    c, scene = _case(rtsr, orc, name)
    cc.check_mix(name, c.first_hits)
    got = _plain(rtsr, orc, name, tc.SPP)
    assert got.spp == tc.SPP and got.sum.shape == (tc.RAYS, 3) and got.sumsq.shape == (tc.RAYS, 3)
    S, Q = tc.host_trace(chk, c.flat, c.o, c.d, c.time)
    _assert_same(name, got.sum, got.sumsq, S, Q)
    assert np.isfinite(got.sum).all() and (got.sum.max(axis=1) > 0).any()
    assert np.array_equal(got.mean, got.sum / tc.SPP)


# ---- 2. light sampling
@pytest.mark.parametrize("name", ["cornell_smoke", "simple_light"])
def test_light_sampling_equals_the_checker(rtsr, orc, chk, name):
    c, scene = _case(rtsr, orc, name)
    cc.check_mix(name, c.first_hits)
    assert c.flat.lights()["n_lights"] >= 1
    got = _trace(scene, c, light_sampling=True)
    S, Q = tc.host_trace(chk, c.flat, c.o, c.d, c.time, light_sampling=True)
    _assert_same(name + " (light sampling)", got.sum, got.sumsq, S, Q)
    plain = _plain(rtsr, orc, name, tc.SPP)
    assert not tc.same_bits(got.sum, plain.sum).all()  # another estimator ran


def test_light_sampling_with_an_empty_light_table(rtsr, orc):
    c, scene = _case(rtsr, orc, "book1")
    assert c.flat.lights()["n_lights"] == 0
    got, plain = _trace(scene, c, light_sampling=True), _plain(rtsr, orc, "book1", tc.SPP)
    _assert_same("book1, light sampling without lights", got.sum, got.sumsq, plain.sum, plain.sumsq)


# ---- 3. estimator agreement
def test_estimators_agree_within_four_standard_errors(rtsr, orc):
    """Cornell smoke's 2000 rays x 64 spp: the two estimators' batch-mean radiance per channel differ by at most 4 combined
    standard errors computed from the returned sumsq.  A condition, not a measurement: test_trace_rays_abi.py shows that the
    checker meets it on these rays."""
    c, scene = _case(rtsr, orc, "cornell_smoke")
    (m0, e0), (m1, e1) = [tc.batch_mean_and_se(r.sum, r.sumsq, 64) for r in (_trace(scene, c, spp=64), _trace(scene, c, spp=64, light_sampling=True))]
    se = np.sqrt(e0 * e0 + e1 * e1)
    print("means %s / %s, combined SE %s, difference in SE %s" % (m0, m1, se, np.abs(m0 - m1) / se))
    assert np.all(m0 > 0) and np.all(se > 0)
    assert np.all(np.abs(m0 - m1) <= 4.0 * se)


# ---- 4. edges of the index space: every cut against one plain call
@pytest.mark.parametrize("spp", [1, 9])
def test_small_batches(rtsr, orc, spp):
    """n around the wave and the chunk: with spp 9 a chunk of 512 items straddles sample planes and the last one is clamped."""
    c, scene = _case(rtsr, orc, "cornell_smoke")
    whole = _plain(rtsr, orc, "cornell_smoke", spp)
    for n in (1, 63, 64, 65, 257):
        part = _trace(scene, c, n=n, spp=spp)
        _assert_same("n = %d, spp %d" % (n, spp), part.sum, part.sumsq, whole.sum[:n], whole.sumsq[:n])


@pytest.mark.parametrize("n,spp", [(73, 7), (64, 8), (57, 9), (511, 1), (512, 1), (513, 1)])
def test_items_around_one_chunk(rtsr, orc, n, spp):
    """n x spp = 511, 512 and 513 items: one chunk less one, exactly one, one more."""
    assert n * spp in (511, 512, 513)
    c, scene = _case(rtsr, orc, "cornell_smoke")
    whole = _plain(rtsr, orc, "cornell_smoke", spp)
    part = _trace(scene, c, n=n, spp=spp)
    _assert_same("%d x %d" % (n, spp), part.sum, part.sumsq, whole.sum[:n], whole.sumsq[:n])


def test_several_passes(rtsr, orc):
    """A sample plane of 2000 rays is 48000 bytes.  72000 bytes hold one plane and no second half: spp 3 goes out as three passes
    on one stream (the stats say so).  288000 bytes at spp 9 are two halves of three planes: three passes, two deep."""
    c, scene = _case(rtsr, orc, "cornell_smoke")
    three, nine = _plain(rtsr, orc, "cornell_smoke", 3), _plain(rtsr, orc, "cornell_smoke", 9)
    serial = _trace(scene, c, spp=3, sample_buffer_bytes=72000, want_stats=True)
    assert serial.stats.passes == 3 and serial.stats.trace_kernel == rtsr.RTX_KERNEL_RAYS
    _assert_same("three passes", serial.sum, serial.sumsq, three.sum, three.sumsq)
    deep = _trace(scene, c, spp=9, sample_buffer_bytes=288000)
    _assert_same("three passes, two deep", deep.sum, deep.sumsq, nine.sum, nine.sumsq)
    single = _trace(scene, c, spp=9, sample_buffer_bytes=48000)  # nine passes of one plane
    _assert_same("nine passes", single.sum, single.sumsq, nine.sum, nine.sumsq)


def test_a_batch_cut_by_first_ray_and_by_accumulate(rtsr, orc):
    c, scene = _case(rtsr, orc, "cornell_smoke")
    whole = _plain(rtsr, orc, "cornell_smoke", tc.SPP)
    cuts = [0, 517, 1300, c.n]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        cut = lambda a: np.ascontiguousarray(a[lo:hi])
        part = scene.trace_rays(cut(c.o), cut(c.d), cut(c.time), spp=tc.SPP, max_depth=tc.DEPTH, background=tc.BACKGROUND,
                                seed=tc.SEED, first_ray=lo, sumsq=True)
        _assert_same("rays [%d, %d)" % (lo, hi), part.sum, part.sumsq, whole.sum[lo:hi], whole.sumsq[lo:hi])
    # two calls over the samples [0, 3) and [3, 4) through the C struct's accumulate
    acc = _trace(scene, c, spp=3)
    again = _trace(scene, c, spp=1, first_sample=3, out=acc)
    assert again is acc and acc.spp == 4
    _assert_same("accumulate", acc.sum, acc.sumsq, whole.sum, whole.sumsq)


def test_host_batch_one_ray_longer_than_a_staging_slice(rtsr, orc):
    """262145 rays at spp 1 through the host entry (two slices, the second of one ray) against one launch from device memory."""
    import torch
    c, scene = _case(rtsr, orc, "book1")
    n = 262144 + 1
    o, d = cc.sphere_rays(n, 21, (-12.0, -1.0, -12.0), (12.0, 14.0, 12.0), 1.0)
    kw = dict(spp=1, max_depth=tc.DEPTH, seed=tc.SEED, sumsq=True)
    host = scene.trace_rays(o, d, **kw)
    dev = scene.trace_rays(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), **kw)
    torch.cuda.synchronize()
    _assert_same("host slices", host.sum, host.sumsq, dev.sum.cpu().numpy(), dev.sumsq.cpu().numpy())
    last = scene.trace_rays(np.ascontiguousarray(o[-1:]), np.ascontiguousarray(d[-1:]), first_ray=n - 1, **kw)
    _assert_same("the last ray alone", last.sum, last.sumsq, host.sum[-1:], host.sumsq[-1:])


# ---- 5. closed forms and the time limit
def test_empty_world_is_the_background(rtsr):
    b = rtsr.Builder(1)
    world, cam, _ = b.get_world_cam(rtsr.SCENE_EMPTY)
    scene = b.flatten(world).upload()
    o, d = cc.sphere_rays(300, 3, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), 2.0)
    bg = np.array([0.25, 0.5, 3.0])
    for nee in (False, True):
        got = scene.trace_rays(o, d, spp=5, background=bg, light_sampling=nee, sumsq=True)
        assert np.array_equal(got.sum, np.tile(5 * bg, (300, 1))) and np.array_equal(got.sumsq, np.tile(5 * bg * bg, (300, 1)))
    assert scene.trace_rays(np.zeros((0, 3)), np.zeros((0, 3))).sum.shape == (0, 3)  # n = 0: RTX_OK, nothing launched


def test_gravity_rays_at_and_past_the_time_limit(rtsr, orc, chk):
    """Scene 8: a ray exactly AT gravity_time_limit is traced and equals the checker; one ulp past it, its sums are NaN."""
    c, scene = _case(rtsr, orc, "gravity_t0.37")
    limit = tc.gravity_time_limit()
    pick = np.flatnonzero(c.first_hits[:, 0] == 1.0)[:4]
    o = np.ascontiguousarray(np.concatenate([c.o[pick], c.o[pick]]))
    d = np.ascontiguousarray(np.concatenate([c.d[pick], c.d[pick]]))
    time = np.concatenate([np.full(4, limit), np.full(4, np.nextafter(limit, np.inf))])
    got = scene.trace_rays(o, d, time, spp=2, max_depth=3, sumsq=True)  # (few bounces: get_center walks 10 000 steps per sphere test here)
    S, Q = tc.host_trace(chk, c.flat, o[:4], d[:4], time[:4], spp=2, max_depth=3)
    _assert_same("gravity at the limit", got.sum[:4], got.sumsq[:4], S, Q)
    assert np.isfinite(got.sum[:4]).all()
    assert np.isnan(got.sum[4:]).all() and np.isnan(got.sumsq[4:]).all()


# ---- 6. f32 scenes
@pytest.mark.parametrize("name", list(cc.F32_CASES))
def test_f32_sums_equal_the_float_checker(rtsr, orc, chk, name):
    """Tier-A scenes (no noise, image or medium: no platform function is reached) against the float judge, bit for bit."""
    c, scene = _case(rtsr, orc, name)
    assert scene.is_f32
    cc.check_mix(name, c.first_hits)
    got = _trace(scene, c)
    S, Q = tc.host_trace(chk, c.flat, c.o, c.d, c.time, f32=True)
    _assert_same(name, got.sum, got.sumsq, S, Q)


def test_f32_scene_has_no_light_sampling(rtsr, orc):
    c, scene = _case(rtsr, orc, "book1_f32")
    with pytest.raises(rtsr.RtxError) as e:
        _trace(scene, c, light_sampling=True)
    assert e.value.status == rtsr.RTX_EUNSUPPORTED


# ---- 7. plumbing
def test_torch_tensors_on_a_side_stream_and_stats(rtsr, orc):
    import torch
    c, scene = _case(rtsr, orc, "cornell_smoke")
    whole = _plain(rtsr, orc, "cornell_smoke", tc.SPP)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    kw = dict(max_depth=tc.DEPTH, background=tc.BACKGROUND, seed=tc.SEED, sumsq=True)
    with torch.cuda.stream(side):
        tens = [torch.from_numpy(a).to(dev) for a in (c.o, c.d, c.time)]
        keep = [t.clone() for t in tens]
        got = scene.trace_rays(*tens, spp=3, **kw)
        scene.trace_rays(*tens, spp=1, first_sample=3, out=got, **kw)  # out= continuation, enqueued behind the first call
        no_q = scene.trace_rays(tens[0], tens[1], tens[2], spp=tc.SPP, max_depth=tc.DEPTH, background=tc.BACKGROUND, seed=tc.SEED)
    side.synchronize()
    assert got.spp == 4 and got.sum.is_cuda and got.sum.dtype == torch.float64 and tuple(got.sumsq.shape) == (c.n, 3)
    _assert_same("torch, side stream", got.sum.cpu().numpy(), got.sumsq.cpu().numpy(), whole.sum, whole.sumsq)
    assert no_q.sumsq is None and tc.same_bits(no_q.sum.cpu().numpy(), whole.sum).all()
    assert all(torch.equal(a, b) for a, b in zip(tens, keep))  # the inputs are unchanged
    with torch.cuda.stream(side):
        st = scene.trace_rays(*tens, spp=tc.SPP, want_stats=True, **kw)  # stats synchronise
    assert st.stats.trace_kernel == rtsr.RTX_KERNEL_RAYS and rtsr.trace_kernel_name(st.stats.trace_kernel) == "k_trace_rays"
    assert st.stats.samples == c.n * tc.SPP and st.stats.passes == 1 and st.stats.trace_ms > 0
    _assert_same("torch, with stats", st.sum.cpu().numpy(), st.sumsq.cpu().numpy(), whole.sum, whole.sumsq)
    host = _trace(scene, c, want_stats=True)
    assert host.stats.trace_kernel == rtsr.RTX_KERNEL_RAYS and host.stats.samples == c.n * tc.SPP
    with pytest.raises(ValueError) as e:
        scene.trace_rays(tens[0], tens[1], tens[2].cpu())
    assert str(e.value).startswith("times:")
