"""Gather queries on the device (Scene.gather, rtx_scene_gather*): k_gather and k_reduce_samples_sh give the sums of the host
checker (tests/gather_host_check.cpp) bit for bit, however the batch is cut; and, without leaning on the code under test,
the sums trace_rays gives for rays that land on a white Lambertian floor, and the closed forms of tests/gather_cases.py.

Every exact comparison is by bit pattern with NaN equal to NaN (cast_rays_cases.same_bits).  Bit-for-bit cases: 500 points x
4 spp x depth 8, the points the first hits of tests/trace_rays_cases.py's rays."""
import numpy as np
import pytest

import cast_rays_cases as cc
import gather_cases as gc
import trace_rays_cases as tc

pytestmark = pytest.mark.gpu
_SCENES = {}
_PLAIN = {}
# (surface form?, light sampling, sh_order)
MODES_F64 = [(True, False, 0), (True, True, 0), (False, False, 0), (False, True, 0), (False, False, 1), (False, True, 2), (False, False, 2)]
MODES_F32 = [(True, False, 0), (False, False, 0), (False, False, 1), (False, False, 2)]


@pytest.fixture(scope="module")
def chk(orc, tmp_path_factory):
    return gc.checkers(tmp_path_factory)


def _case(rtsr, orc, name):
    c = tc.case(rtsr, orc, name)
    if name not in _SCENES:
        _SCENES[name] = (c.flat.upload(f32=c.f32), gc.points_of(c))
    return (c,) + _SCENES[name]


def _gather(scene, pts, n=None, surface=True, **kw):
    p, nrm, t = pts
    n = len(p) if n is None else n
    kw.setdefault("spp", gc.SPP)
    cut = lambda a: np.ascontiguousarray(a[:n])
    return scene.gather(cut(p), cut(nrm) if surface else None, cut(t), max_depth=gc.DEPTH, background=gc.BACKGROUND, seed=gc.SEED, **kw)


def _plain(rtsr, orc, spp, surface=True, sh_order=0):
    """One plain call over Cornell smoke's whole batch (default sample buffer, first_point 0): what every cut is held to."""
    key = (spp, surface, sh_order)
    if key not in _PLAIN:
        c, scene, pts = _case(rtsr, orc, "cornell_smoke")
        _PLAIN[key] = _gather(scene, pts, spp=spp, surface=surface, sh_order=sh_order)
    return _PLAIN[key]


def _assert_same(what, got_S, got_Q, ref_S, ref_Q):
    bad = np.flatnonzero(~(gc.same_bits(got_S, ref_S) & gc.same_bits(got_Q, ref_Q)))
    print("%s: %d points, %d differ" % (what, len(ref_S), len(bad)))
    assert len(bad) == 0, "%s: point %d: got %r / %r, expected %r / %r" % (
        what, bad[0], got_S[bad[0]].tolist(), got_Q[bad[0]].tolist(), ref_S[bad[0]].tolist(), ref_Q[bad[0]].tolist())


# ---- 1. the identity that does not rest on the code under test
@pytest.mark.parametrize("kind", ["rect_light", "sphere_light", "metal_glass"])
def test_gather_on_a_white_floor_is_trace_rays_one_bounce_later(rtsr, kind):
    """Rays are cast onto a white Lambertian floor; p and normal come from cast_rays' columns.  A trace_rays path of such a ray
    scatters at p with the first draws of its stream, gathers nothing there (the floor does not emit) and carries the
    product (1, 1, 1) on: gather(p, normal, max_depth = d) of the same (seed, index, sample range) is that path from its second
    vertex, so sum and sumsq are equal bit for bit -- both estimators in f64, the plain one in f32."""
    b, flat = gc.white_floor_scene(rtsr, kind)
    assert flat.lights()["n_lights"] == 1
    o, d = gc.floor_rays(700)
    # one more ray, straight down far from every object: its ids name the floor's material and slot
    o = np.ascontiguousarray(np.concatenate([o, [[40.0, 1.0, 40.0]]]))
    d = np.ascontiguousarray(np.concatenate([d, [[0.0, -1.0, 0.0]]]))
    bg = (0.05, 0.07, 0.1) if kind != "metal_glass" else (0.4, 0.5, 0.7)
    for f32 in (False, True):
        scene = flat.upload(f32=f32)
        hits = scene.cast_rays(o, d, want=("p", "normal", "ids"))
        assert hits.ids[-1, 0] == 1
        on_floor = np.flatnonzero((hits.ids[:, 0] == 1) & (hits.ids[:, 1] == hits.ids[-1, 1]) & (hits.ids[:, 2] == hits.ids[-1, 2]))
        print("%s f32 %d: %d of %d rays land on the floor" % (kind, f32, len(on_floor), len(o)))
        assert len(on_floor) >= 450
        assert np.array_equal(hits.normal[on_floor], np.tile([0.0, 1.0, 0.0], (len(on_floor), 1)))
        p, nrm = np.ascontiguousarray(hits.p), np.ascontiguousarray(hits.normal)
        lit = 0
        for nee in ((False,) if f32 else (False, True)):
            for depth in (1, 2, 8):
                kw = dict(spp=4, background=bg, seed=5, light_sampling=nee)
                ref = scene.trace_rays(o, d, max_depth=depth + 1, sumsq=True, **kw)
                got = scene.gather(p, nrm, max_depth=depth, **kw)
                _assert_same("%s f32 %d light sampling %d depth %d" % (kind, f32, nee, depth), got.sum[on_floor], got.sumsq[on_floor],
                             ref.sum[on_floor], ref.sumsq[on_floor])
                assert np.isfinite(got.sum).all()
                lit += int((got.sum[on_floor].max(axis=1) > 0).sum())
        assert lit > 0


# ---- 2. against the judge
@pytest.mark.parametrize("name", ["cornell_smoke", "book2", "zoo_middle", "gravity_t0.37"])
def test_f64_sums_equal_the_checker(rtsr, orc, chk, name):
    """Both forms, both estimators, sh_order 0, 1 and 2.  Cornell smoke and Book-2 run P_ANY and their media draw from the path's
    stream, the zoo runs P_INST, scene 8 P_ALL."""
    c, scene, pts = _case(rtsr, orc, name)
    p, nrm, t = pts
    n, kw = (gc.POINTS, {}) if name != "gravity_t0.37" else (64, dict(spp=2))  # (get_center walks thousands of steps per sphere test)
    depth = gc.DEPTH if name != "gravity_t0.37" else 3
    for surface, nee, order in MODES_F64:
        got = scene.gather(p[:n].copy(), nrm[:n].copy() if surface else None, t[:n].copy(), spp=kw.get("spp", gc.SPP), max_depth=depth,
                           background=gc.BACKGROUND, seed=gc.SEED, light_sampling=nee, sh_order=order)
        S, Q = gc.host_gather(chk, c.flat, p[:n], nrm[:n] if surface else None, t[:n], spp=kw.get("spp", gc.SPP), max_depth=depth,
                              light_sampling=nee, sh_order=order)
        assert got.sum.shape == gc.sum_shape(n, order) and got.sumsq.shape == gc.sum_shape(n, order)
        _assert_same("%s surface %d light sampling %d sh_order %d" % (name, surface, nee, order), got.sum, got.sumsq, S, Q)
        assert np.isfinite(got.sum).all() and (got.sum != 0).any()


def test_light_sampling_is_another_estimator(rtsr, orc):
    c, scene, pts = _case(rtsr, orc, "cornell_smoke")
    assert c.flat.lights()["n_lights"] >= 1
    for surface in (True, False):
        a, b = _gather(scene, pts, surface=surface), _gather(scene, pts, surface=surface, light_sampling=True)
        assert not gc.same_bits(a.sum, b.sum).all()
    assert not gc.same_bits(_gather(scene, pts, surface=True).sum, _gather(scene, pts, surface=False).sum).all()


def test_gravity_points_at_and_past_the_time_limit(rtsr, orc, chk):
    """Scene 8: a point exactly AT gravity_time_limit is traced and equals the checker; one ulp past it, its sums are NaN -- the
    SH sums too."""
    c, scene, pts = _case(rtsr, orc, "gravity_t0.37")
    limit = tc.gravity_time_limit()
    p = np.ascontiguousarray(np.concatenate([pts[0][:4], pts[0][:4]]))
    nrm = np.ascontiguousarray(np.concatenate([pts[1][:4], pts[1][:4]]))
    time = np.concatenate([np.full(4, limit), np.full(4, np.nextafter(limit, np.inf))])
    for surface, order in ((True, 0), (False, 0), (False, 2)):
        got = scene.gather(p, nrm if surface else None, time, spp=2, max_depth=3, sh_order=order)
        S, Q = gc.host_gather(chk, c.flat, p, nrm if surface else None, time, spp=2, max_depth=3, sh_order=order)
        _assert_same("gravity at and past the limit, surface %d sh_order %d" % (surface, order), got.sum, got.sumsq, S, Q)
        assert np.isfinite(got.sum[:4]).all()
        assert np.isnan(got.sum[4:]).all() and np.isnan(got.sumsq[4:]).all()


@pytest.mark.parametrize("name", list(cc.F32_CASES))
def test_f32_sums_equal_the_float_checker(rtsr, orc, chk, name):
    """Tier-A scenes (no noise, image or medium: no platform function is reached) against the float judge, bit for bit."""
    c, scene, pts = _case(rtsr, orc, name)
    assert scene.is_f32
    p, nrm, t = pts
    for surface, nee, order in MODES_F32:
        got = _gather(scene, pts, surface=surface, sh_order=order)
        S, Q = gc.host_gather(chk, c.flat, p, nrm if surface else None, t, sh_order=order, f32=True)
        _assert_same("%s surface %d sh_order %d" % (name, surface, order), got.sum, got.sumsq, S, Q)
        assert np.isfinite(got.sum).all() and (got.sum != 0).any()
    with pytest.raises(rtsr.RtxError) as e:
        _gather(scene, pts, light_sampling=True)
    assert e.value.status == rtsr.RTX_EUNSUPPORTED


# ---- 3. cuts against one plain call
@pytest.mark.parametrize("spp", [1, 9])
def test_small_batches(rtsr, orc, spp):
    """n around the wave and the chunk: with spp 9 a chunk of 512 items straddles sample planes and the last one is clamped."""
    c, scene, pts = _case(rtsr, orc, "cornell_smoke")
    for surface, order in ((True, 0), (False, 2)):
        whole = _plain(rtsr, orc, spp, surface, order)
        for n in (1, 63, 64, 65, 257):
            part = _gather(scene, pts, n=n, spp=spp, surface=surface, sh_order=order)
            _assert_same("n = %d, spp %d, surface %d" % (n, spp, surface), part.sum, part.sumsq, whole.sum[:n], whole.sumsq[:n])


@pytest.mark.parametrize("n,spp", [(73, 7), (64, 8), (57, 9)])
def test_items_around_one_chunk(rtsr, orc, n, spp):
    """n x spp = 511, 512 and 513 items: one chunk less one, exactly one, one more."""
    assert n * spp in (511, 512, 513)
    c, scene, pts = _case(rtsr, orc, "cornell_smoke")
    whole = _plain(rtsr, orc, spp)
    part = _gather(scene, pts, n=n, spp=spp)
    _assert_same("%d x %d" % (n, spp), part.sum, part.sumsq, whole.sum[:n], whole.sumsq[:n])


def test_several_passes(rtsr, orc):
    """A sample plane of 500 points is 12000 bytes.  18000 bytes hold one plane and no second half: spp 3 goes out as three passes
    on one stream (the stats say so).  72000 bytes at spp 9 are two halves of three planes: three passes, two deep.  The SH
    reduction runs once per pass and must continue the sums in pass order."""
    c, scene, pts = _case(rtsr, orc, "cornell_smoke")
    for surface, order in ((True, 0), (False, 2)):
        three, nine = _plain(rtsr, orc, 3, surface, order), _plain(rtsr, orc, 9, surface, order)
        serial = _gather(scene, pts, spp=3, surface=surface, sh_order=order, sample_buffer_bytes=18000, want_stats=True)
        assert serial.stats.passes == 3 and serial.stats.trace_kernel == rtsr.RTX_KERNEL_RAYS
        _assert_same("three passes", serial.sum, serial.sumsq, three.sum, three.sumsq)
        deep = _gather(scene, pts, spp=9, surface=surface, sh_order=order, sample_buffer_bytes=72000)
        _assert_same("three passes, two deep", deep.sum, deep.sumsq, nine.sum, nine.sumsq)
        single = _gather(scene, pts, spp=9, surface=surface, sh_order=order, sample_buffer_bytes=12000)  # nine passes of one plane
        _assert_same("nine passes", single.sum, single.sumsq, nine.sum, nine.sumsq)


@pytest.mark.parametrize("group", ["1", "3", "64", "499", "500"])
def test_every_item_order_gives_the_same_sums(rtsr, orc, monkeypatch, group):
    """The order of a pass's items (core/item_order.hpp; RTX_ITEM_GROUP, read at upload) cannot change a sum: groups of 1, 3, 64,
    499 (a last group of one point) and 500 points (one group) at 9 spp, in one pass and in passes of three sample planes."""
    c, scene, pts = _case(rtsr, orc, "cornell_smoke")
    monkeypatch.setenv("RTX_ITEM_GROUP", group)
    grouped = c.flat.upload()
    monkeypatch.delenv("RTX_ITEM_GROUP")
    for surface, nee, order in ((True, True, 0), (False, False, 2)):
        whole = _gather(scene, pts, spp=9, surface=surface, light_sampling=nee, sh_order=order)
        for budget in (0, 72000):
            got = _gather(grouped, pts, spp=9, surface=surface, light_sampling=nee, sh_order=order, sample_buffer_bytes=budget)
            _assert_same("groups of %s, budget %d, surface %d" % (group, budget, surface), got.sum, got.sumsq, whole.sum, whole.sumsq)


def test_a_batch_cut_by_first_point_and_by_accumulate(rtsr, orc):
    c, scene, pts = _case(rtsr, orc, "cornell_smoke")
    p, nrm, t = pts
    for surface, order in ((True, 0), (False, 1)):
        whole = _plain(rtsr, orc, gc.SPP, surface, order)
        cuts = [0, 129, 330, len(p)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            cut = lambda a: np.ascontiguousarray(a[lo:hi])
            part = scene.gather(cut(p), cut(nrm) if surface else None, cut(t), spp=gc.SPP, max_depth=gc.DEPTH, background=gc.BACKGROUND,
                                seed=gc.SEED, first_point=lo, sh_order=order)
            _assert_same("points [%d, %d)" % (lo, hi), part.sum, part.sumsq, whole.sum[lo:hi], whole.sumsq[lo:hi])
        # two calls over the samples [0, 3) and [3, 4) through the C struct's accumulate
        acc = _gather(scene, pts, spp=3, surface=surface, sh_order=order)
        again = _gather(scene, pts, spp=1, first_sample=3, out=acc, surface=surface, sh_order=order)
        assert again is acc and acc.spp == 4
        _assert_same("accumulate", acc.sum, acc.sumsq, whole.sum, whole.sumsq)


def test_host_batch_one_point_longer_than_a_staging_slice(rtsr, orc):
    """262145 points at spp 1, depth 1 through the host entry (two slices, the second of one point) against one launch from
    device memory."""
    import torch
    c, scene, pts = _case(rtsr, orc, "book1")
    n = 262144 + 1
    rng = np.random.default_rng(21)
    p = np.ascontiguousarray(rng.uniform((-12.0, 0.1, -12.0), (12.0, 4.0, 12.0), (n, 3)))
    nrm = np.ascontiguousarray(rng.normal(size=(n, 3)))
    kw = dict(spp=1, max_depth=1, seed=gc.SEED)
    host = scene.gather(p, nrm, **kw)
    dev = scene.gather(torch.from_numpy(p).cuda(), torch.from_numpy(nrm).cuda(), **kw)
    torch.cuda.synchronize()
    _assert_same("host slices", host.sum, host.sumsq, dev.sum.cpu().numpy(), dev.sumsq.cpu().numpy())
    last = scene.gather(np.ascontiguousarray(p[-1:]), np.ascontiguousarray(nrm[-1:]), first_point=n - 1, **kw)
    _assert_same("the last point alone", last.sum, last.sumsq, host.sum[-1:], host.sumsq[-1:])
    assert len(np.unique(host.sum, axis=0)) >= 2  # the sky, and 0 from inside a sphere


# ---- 4. SH sums against trace_rays
@pytest.mark.parametrize("f32", [False, True])
def test_sh_sums_equal_trace_rays_along_the_directions(rtsr, f32):
    """Media-free scene, max_depth 1: a sample depends on its direction alone (the first hit's emission, or the background).
    Directions from rtx_gather_directions, radiances from trace_rays along them (one ray per (point, sample), one sample each),
    summed in numpy in the stated order: bit for bit the SH sums."""
    b, flat = gc.white_floor_scene(rtsr, "metal_glass")
    scene = flat.upload(f32=f32)
    n, spp = 96, 6
    rng = np.random.default_rng(12)
    p = np.ascontiguousarray(rng.uniform((-3.0, 0.2, -3.0), (3.0, 3.0, 3.0), (n, 3)))
    bg = (0.4, 0.5, 0.7)
    for order in (1, 2):
        got = scene.gather(p, spp=spp, max_depth=1, background=bg, seed=8, sh_order=order, first_point=4, first_sample=2)
        d = rtsr.gather_directions(n, spp=spp, seed=8, first_point=4, first_sample=2, f32=f32)
        rays = scene.trace_rays(np.ascontiguousarray(np.repeat(p, spp, axis=0)), np.ascontiguousarray(d.reshape(-1, 3)), spp=1, max_depth=1,
                                background=bg)
        L = rays.sum.reshape(n, spp, 3)
        assert len(np.unique(L.reshape(-1, 3), axis=0)) >= 2  # the light and the background are both seen
        S, Q = gc.sh_sums_in_stated_order(d, L, order)
        _assert_same("SH order %d f32 %d" % (order, f32), got.sum, got.sumsq, S, Q)
        plain = scene.gather(p, spp=spp, max_depth=1, background=bg, seed=8, first_point=4, first_sample=2)
        assert gc.same_bits(plain.sum, _ordered_sum(L)).all()


def _ordered_sum(L):
    s = np.zeros((L.shape[0], 3))
    for k in range(L.shape[1]):
        s = s + L[:, k]
    return s


# ---- 5. closed forms
@pytest.mark.parametrize("name", list(gc.SURFACE_CASES))
def test_surface_gather_meets_the_form_factor(rtsr, name):
    """Background 0, depth 1: the mean equals Le * F within 4.5 standard errors of the device's own sumsq, both estimators; on the
    small light, light sampling's standard error is below the plain estimator's.  test_gather_abi.py shows that the checker
    meets the same conditions."""
    b, flat = gc.SURFACE_CASES[name].build(rtsr)
    lines, failed = gc.surface_check(name, gc.scene_gatherer(flat.upload()))
    print("\n".join(lines))
    assert not failed, failed


def test_probe_gather_meets_the_cap_coefficients(rtsr):
    b, flat = gc.probe_scene(rtsr)
    scene = flat.upload()
    lines, failed = gc.probe_check(gc.scene_gatherer(scene))
    print("\n".join(lines))
    assert not failed, failed
    got = scene.gather(np.ascontiguousarray(gc.PROBES), spp=64, max_depth=1, background=(0.0, 0.0, 0.0), sh_order=2)
    assert np.array_equal(got.sh, got.sum * (4.0 * np.pi / 64)) and got.irradiance is None and got.form == "probe"


# ---- 6. plumbing
def test_torch_tensors_on_a_side_stream_and_stats(rtsr, orc):
    import torch
    c, scene, pts = _case(rtsr, orc, "cornell_smoke")
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    kw = dict(max_depth=gc.DEPTH, background=gc.BACKGROUND, seed=gc.SEED)
    for surface, order in ((True, 0), (False, 2)):
        whole = _plain(rtsr, orc, gc.SPP, surface, order)
        with torch.cuda.stream(side):
            tens = [torch.from_numpy(a).to(dev) for a in pts]
            keep = [t.clone() for t in tens]
            args = (tens[0], tens[1] if surface else None, tens[2])
            got = scene.gather(*args, spp=3, sh_order=order, **kw)
            scene.gather(*args, spp=1, first_sample=3, out=got, sh_order=order, **kw)  # out= continuation, enqueued behind the first call
            no_q = scene.gather(*args, spp=gc.SPP, sumsq=False, sh_order=order, **kw)
        explicit = scene.gather(*args, spp=gc.SPP, sh_order=order, stream=side, **kw)  # the stream named, not current
        side.synchronize()
        assert got.spp == 4 and got.sum.is_cuda and got.sum.dtype == torch.float64 and tuple(got.sumsq.shape) == gc.sum_shape(len(pts[0]), order)
        _assert_same("torch, side stream", got.sum.cpu().numpy(), got.sumsq.cpu().numpy(), whole.sum, whole.sumsq)
        _assert_same("torch, stream=", explicit.sum.cpu().numpy(), explicit.sumsq.cpu().numpy(), whole.sum, whole.sumsq)
        assert no_q.sumsq is None and gc.same_bits(no_q.sum.cpu().numpy(), whole.sum).all()
        assert all(torch.equal(a, b) for a, b in zip(tens, keep))  # the inputs are unchanged
        with torch.cuda.stream(side):
            st = scene.gather(*args, spp=gc.SPP, sh_order=order, want_stats=True, **kw)  # stats synchronise
        assert st.stats.trace_kernel == rtsr.RTX_KERNEL_RAYS
        assert st.stats.samples == len(pts[0]) * gc.SPP and st.stats.passes == 1 and st.stats.trace_ms > 0
        _assert_same("torch, with stats", st.sum.cpu().numpy(), st.sumsq.cpu().numpy(), whole.sum, whole.sumsq)
    host = _gather(scene, pts, want_stats=True)
    assert host.stats.trace_kernel == rtsr.RTX_KERNEL_RAYS and host.stats.samples == len(pts[0]) * gc.SPP
    assert np.array_equal(host.irradiance, host.sum * (np.pi / gc.SPP)) and host.sh is None
    with pytest.raises(ValueError) as e:
        scene.gather(tens[0], tens[1].cpu())
    assert str(e.value).startswith("normals:")
    empty = scene.gather(np.zeros((0, 3)), np.zeros((0, 3)))  # n = 0: RTX_OK, nothing launched
    assert empty.sum.shape == (0, 3) and scene.gather(np.zeros((0, 3)), sh_order=2).sum.shape == (0, 9, 3)
