"""Occlusion queries on the device (Scene.occlusion, rtx_scene_occlusion*): k_occlusion answers what the CPU core answers.

Every comparison with the judge (tests/occlusion_host_check.cpp: a plain loop over world_occlusion<F_ALL>) is by bit pattern
with NaN equal to NaN.  Scenes and rays: tests/occlusion_cases.py (at most 2000 rays per scene); a case's scene is uploaded
once per precision and shared by the tests of this file."""
import numpy as np
import pytest

import cast_rays_cases as cc
import occlusion_cases as oc
import trace_rays_cases as tc

pytestmark = pytest.mark.gpu
_SCENES = {}


@pytest.fixture(scope="module")
def chk(orc, tmp_path_factory):
    return oc.checkers(tmp_path_factory)


def _scene(c, f32):
    key = (c.name, f32)
    if key not in _SCENES:
        _SCENES[key] = c.flat.upload(f32=f32)
    return _SCENES[key]


def _assert_same(name, got, ref):
    bad = np.flatnonzero(~oc.same_bits(got, ref))
    print("%s: %d rays, %d blocked, %d through fog, %d differ from the judge" %
          (name, len(ref), int(np.isinf(ref).sum()), int(((ref > 0) & np.isfinite(ref)).sum()), len(bad)))
    assert len(bad) == 0, "%s: ray %d: device %r, judge %r" % (name, bad[0], got[bad[0]], ref[bad[0]])


# ---- 1. bit for bit against the judge: P_INST (the zoos), P_ALL (scene 8), P_ANY (the rest), media included, both precisions
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(oc.MEDIA_FREE) + list(oc.MEDIA))
def test_tau_equals_the_judge(rtsr, orc, chk, name, f32):
    c = oc.case(rtsr, orc, name)
    scene = _scene(c, f32)
    assert scene.is_f32 == f32
    got = scene.occlusion(c.o, c.d, c.time, c.t_max, t_min=oc.T_MIN)
    ref = oc.host_tau(chk, c.flat, c.o, c.d, c.time, c.t_max, f32=f32)
    _assert_same(name, got.tau, ref)
    assert np.array_equal(got.blocked, np.isinf(ref)) and got.n == c.n
    if name == "book2":
        # the scene-wide mist lies on every ray that no surface blocks (Cornell smoke's rays end on a wall or miss the room:
        # its fog is test_media_segments_equal_the_judge's)
        assert ((ref > 0) & np.isfinite(ref)).sum() >= c.n // 10
    if name in oc.MEDIA_FREE:
        # consequence 1 on the device's own answers: blocked is the hit flag of the closest-hit cast
        ids = scene.cast_rays(c.o, c.d, c.time, c.t_max, t_min=oc.T_MIN, want=("ids",)).ids
        assert np.array_equal(np.isinf(got.tau), ids[:, 0] == 1)
        assert 4 * int(got.blocked.sum()) >= c.n and 10 * int((~got.blocked).sum()) >= c.n


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_media_segments_equal_the_judge(rtsr, orc, chk, f32):
    c = oc.case(rtsr, orc, "cornell_smoke")
    a, b = oc.segments()
    ref = oc.segment_tau(chk, c.flat, a, b, f32=f32)
    scene = _scene(c, f32)
    got = scene.occlusion_between(a, b)
    _assert_same("media segments", got.tau, ref)
    # occlusion_between is occlusion with direction b - a on [0.001, 1 - eps], as one bound for all rays or one per ray
    d = np.ascontiguousarray(b - a)
    assert oc.same_bits(scene.occlusion(a, d, t_max_all=1.0 - oc.SEG_EPS).tau, got.tau).all()
    assert oc.same_bits(scene.occlusion(a, d, None, np.full(len(a), 1.0 - oc.SEG_EPS)).tau, got.tau).all()
    t = got.transmittance
    assert np.all(t[got.blocked] == 0.0) and np.all(t[got.tau == 0.0] == 1.0) and np.all((t >= 0.0) & (t <= 1.0))


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_closed_form_scenes_equal_the_judge(rtsr, orc, chk, f32):
    for c in oc.closed_form_cases(rtsr):
        got = c.flat.upload(f32=f32).occlusion(c.o, c.d, None, c.t_max, t_min=c.t_min)
        _assert_same(c.name, got.tau, oc.host_tau(chk, c.flat, c.o, c.d, None, c.t_max, t_min=c.t_min, f32=f32))


# ---- 2. the GravitySpheres' time limit
def test_gravity_rays_at_and_past_the_time_limit(rtsr, orc, chk):
    """A ray exactly AT the limit is tested and equals the judge; one ulp past it is NaN: not tested must not read as clear."""
    c = oc.case(rtsr, orc, "gravity_t0.37")
    limit = tc.gravity_time_limit()
    o, d = np.ascontiguousarray(np.concatenate([c.o[:6], c.o[:6]])), np.ascontiguousarray(np.concatenate([c.d[:6], c.d[:6]]))
    time = np.concatenate([np.full(6, limit), np.full(6, np.nextafter(limit, np.inf))])
    got = _scene(c, False).occlusion(o, d, time)
    ref = oc.host_tau(chk, c.flat, o, d, time)
    assert not np.isnan(ref[:6]).any() and np.isnan(ref[6:]).all()
    _assert_same("gravity at the limit", got.tau, ref)
    assert not got.blocked[6:].any() and np.isnan(got.transmittance[6:]).all()


# ---- 3. batch shapes
def test_batch_sizes(rtsr, orc, chk):
    """1, 63, 64, 65, 257 rays, and one pass of the grid (8 blocks of 256 threads per CU) plus one ray, which also crosses a
    staging slice of the host entry (262144 rays)."""
    import torch
    c = oc.case(rtsr, orc, "slot_list")
    scene = _scene(c, False)
    n = 8 * 256 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    assert n > 262144
    o, d = cc.sphere_rays(n, 11, *c.box)
    big = scene.occlusion(o, d).tau
    assert set(np.unique(big).tolist()) == {0.0, np.inf}
    assert 4 * int(np.isinf(big).sum()) >= n and 10 * int((big == 0).sum()) >= n
    # the judge on the first and the last rays of the batch, the device's cast on all of them
    for lo, hi in ((0, 1500), (n - 1500, n)):
        _assert_same("big batch [%d, %d)" % (lo, hi), big[lo:hi], oc.host_tau(chk, c.flat, o[lo:hi], d[lo:hi]))
    assert np.array_equal(np.isinf(big), scene.cast_rays(o, d, want=("ids",)).ids[:, 0] == 1)
    for k in (1, 63, 64, 65, 257):
        part = scene.occlusion(np.ascontiguousarray(o[:k]), np.ascontiguousarray(d[:k])).tau
        assert part.shape == (k,) and part.tobytes() == big[:k].tobytes(), k
    empty = scene.occlusion(np.zeros((0, 3)), np.zeros((0, 3)))
    assert empty.n == 0 and empty.tau.shape == (0,)


def test_a_split_batch_equals_the_whole(rtsr, orc):
    c = oc.case(rtsr, orc, "cornell_smoke")
    scene = _scene(c, False)
    whole = scene.occlusion(c.o, c.d, c.time, c.t_max).tau
    cuts = [0, 517, 1300, c.n]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        cut = lambda x: np.ascontiguousarray(x[lo:hi])
        assert scene.occlusion(cut(c.o), cut(c.d), cut(c.time), cut(c.t_max)).tau.tobytes() == whole[lo:hi].tobytes(), (lo, hi)


# ---- 4. device pointers
def test_torch_tensors_on_a_side_stream(rtsr, orc):
    import torch
    c = oc.case(rtsr, orc, "cornell_smoke")
    scene = _scene(c, False)
    ref = scene.occlusion(c.o, c.d, c.time, c.t_max)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        tens = [torch.from_numpy(x).to(dev) for x in (c.o, c.d, c.time, c.t_max)]
        keep = [t.clone() for t in tens]
        got = scene.occlusion(*tens)                   # torch's current stream: the side stream
        named = scene.occlusion(*tens, stream=side)    # the same stream, named
    side.synchronize()
    assert got.tau.is_cuda and got.tau.dtype == torch.float64 and tuple(got.tau.shape) == (c.n,)
    assert got.tau.cpu().numpy().tobytes() == ref.tau.tobytes() and named.tau.cpu().numpy().tobytes() == ref.tau.tobytes()
    assert torch.equal(got.blocked.cpu(), torch.from_numpy(ref.blocked))
    assert np.array_equal(got.transmittance.cpu().numpy() == 0.0, ref.blocked)
    assert all(torch.equal(x, y) for x, y in zip(tens, keep))  # the inputs are unchanged
    with pytest.raises(ValueError) as e:
        scene.occlusion(tens[0], tens[1], t_max=tens[3].cpu())
    assert str(e.value).startswith("t_max:")


# ---- 5. the query reads what the updates wrote
def test_tau_follows_set_spheres_and_set_shading(rtsr, orc, chk):
    """A fog sphere and a solid ball on a resident scene: the ball moved out of the rays' way (set_spheres) and the fog thinned
    (set_shading) -- tau equals the judge on the flat scene given the same updates."""
    b = rtsr.Builder(1)
    grey = b.lambertian((0.5, 0.5, 0.5))
    ball = b.sphere((0.0, 0.0, 4.0), 1.0, grey)
    fog = b.constant_medium((0.8, 0.8, 0.8), 0.4, b.sphere((0.0, 0.0, 0.0), 2.0, grey))
    flat = b.flatten(b.hittable_list([fog, ball, b.sphere((50.0, 0.0, 0.0), 1.0, grey)]))
    rng = np.random.default_rng(5)
    o = np.ascontiguousarray(np.column_stack([rng.uniform(-1.5, 1.5, 300), rng.uniform(-1.5, 1.5, 300), np.full(300, -6.0)]))
    d = np.ascontiguousarray(np.tile([0.0, 0.0, 1.0], (300, 1)))
    scene = flat.upload()
    before = scene.occlusion(o, d).tau
    _assert_same("before the updates", before, oc.host_tau(chk, flat, o, d))
    ids = flat.sphere_ids(b, ball)
    moved = np.array([[20.0, 0.0, 4.0, 1.0]])
    scene.set_spheres(ids, moved)
    scene.set_shading([("medium_density", 0, 0.1)])
    flat.set_spheres(ids, moved)
    flat.set_shading([("medium_density", 0, 0.1)])
    after = scene.occlusion(o, d).tau
    ref = oc.host_tau(chk, flat, o, d)
    _assert_same("after the updates", after, ref)
    was_blocked = np.isinf(before)
    assert 10 * int(was_blocked.sum()) >= 300 and not np.isinf(after).any()     # the ball is out of the way
    thin = ~was_blocked & (before > 0)
    assert thin.any() and np.all(after[thin] < before[thin])                    # and the fog is thinner
