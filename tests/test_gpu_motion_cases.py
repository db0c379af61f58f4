"""The device on the scenes of tests/motion_cases.py (proven on the CPU in tests/test_motion_cases.py): every time interval of
a MovingSphere, of the BVH above it and of the shutter, through k_trace_lds -- whose three pieces of interval arithmetic (the
common ratio, the time-aware boxes in both forms) the frame cannot tell apart, so RtxRenderStats.trace_variant is held to the
table as well -- under every switch that picks another instantiation, through the other walkers, through ray queries at the
movers' centres, as plain lists through k_trace_world, and in the f32 fast mode.  Frames are 96 x 64 at 4 spp."""
import numpy as np
import pytest

import motion_cases as mc

pytestmark = pytest.mark.gpu

WALKERS = ({"RTX_WIDE": "0"}, {"RTX_WIDE": "1"}, {"RTX_TRACE_KERNEL": "simple"}, {"RTX_TRACE_KERNEL": "world"}, {"RTX_TRACE_KERNEL": "wavefront"})
SWITCHES = ({"RTX_MV_COMMON": "0"}, {"RTX_MOTION": "0"}, {"RTX_MOTION_AXIS": "0"}, {"RTX_RING": "0"})
WD_TIME_BOX = 64  # csrc/hip/trace_world.inc
_built = {}


class Built:
    """One (case, shutter): the scene, its flat form, the oracle's frame (where one is claimed) and the default render."""

    def __init__(self, rtsr, orc, case_id, shutter):
        self.b, self.world, self.cam, self.cfg, self.movers = mc.build(rtsr, case_id, shutter)
        self.h = rtsr.image_height(self.cfg)
        self.flat = self.b.flatten(self.world)
        self.ref = self.ref8 = None
        if case_id in mc.PARITY:
            self.ref, self.ref8 = orc.o2_render(self.flat.arrays_ptr(), self.cam, self.cfg, self.h, threads=16)
        self.scene = self.flat.upload()
        self.screen = self.scene.render(self.cam, self.cfg, want_stats=True)


def _get(rtsr, orc, case_id, shutter=0):
    if (case_id, shutter) not in _built:
        _built[(case_id, shutter)] = Built(rtsr, orc, case_id, shutter)
    return _built[(case_id, shutter)]


def _same(a, b):
    """Equal values, a NaN equal to a NaN (only `degenerate` has any)."""
    return np.array_equal(a, b, equal_nan=True)


def _diff(a, b):
    return "%d pixels differ" % int((~((a == b) | (np.isnan(a) & np.isnan(b)))).any(axis=2).sum())


def _kernel(rtsr, screen):
    return rtsr.trace_kernel_name(screen.stats.trace_kernel)


def _render_under(rtsr, monkeypatch, flat, cam, cfg, env):
    """A fresh upload under the switches of env (they are read per upload) and its frame."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    screen = flat.upload().render(cam, cfg, want_stats=True)
    for k in env:
        monkeypatch.delenv(k)
    return screen


@pytest.mark.parametrize("case_id,shutter", [p for p in mc.SHUTTERS if p[0] in mc.PARITY], ids=lambda v: str(v))
def test_k_trace_lds_renders_the_oracles_frame_and_says_which_form_ran(rtsr, orc, case_id, shutter):
    s = _get(rtsr, orc, case_id, shutter)
    print("\n[motion cases] %s shutter %d: kernel %s, variant %d (expected %d), %s" % (
        case_id, shutter, _kernel(rtsr, s.screen), s.screen.stats.trace_variant, mc.expected_variant(case_id, shutter), _diff(s.screen.accum, s.ref)))
    assert np.array_equal(s.screen.accum, s.ref), _diff(s.screen.accum, s.ref)
    assert np.array_equal(s.screen.rgb8, s.ref8)
    assert _kernel(rtsr, s.screen) == "k_trace_lds"
    assert s.screen.stats.trace_variant == mc.expected_variant(case_id, shutter)


@pytest.mark.parametrize("case_id", mc.PARITY)
def test_every_switch_and_leaf_size_renders_the_same_frame(rtsr, orc, monkeypatch, case_id):
    """RTX_MV_COMMON=0 (every record's own interval: the non-common leaf path), RTX_MOTION=0 (static boxes), RTX_MOTION_AXIS=0
    (all-axes slopes), RTX_RING=0 and leaves of 1 and of up to 4: the oracle's frame each time, the variant word the table's."""
    s = _get(rtsr, orc, case_id)
    for env in SWITCHES:
        got = _render_under(rtsr, monkeypatch, s.flat, s.cam, s.cfg, env)
        assert np.array_equal(got.accum, s.ref), (env, _diff(got.accum, s.ref))
        assert np.array_equal(got.rgb8, s.ref8), env
        assert _kernel(rtsr, got) == "k_trace_lds", env
        assert got.stats.trace_variant == mc.expected_variant(case_id, 0, env), (env, got.stats.trace_variant)
    for leaf in (1, 4):
        got = s.b.flatten(s.world, max_leaf=leaf).upload().render(s.cam, s.cfg, want_stats=True)
        assert np.array_equal(got.accum, s.ref), (leaf, _diff(got.accum, s.ref))
        assert np.array_equal(got.rgb8, s.ref8), leaf
        assert _kernel(rtsr, got) == "k_trace_lds", leaf
        assert got.stats.trace_variant == mc.expected_variant(case_id), (leaf, got.stats.trace_variant)


@pytest.mark.parametrize("case_id", ["offset", "bvh_narrower", "mixed", "reversed"])
def test_every_other_walker_renders_the_same_frame(rtsr, orc, monkeypatch, case_id):
    s = _get(rtsr, orc, case_id)
    for env in WALKERS:
        got = _render_under(rtsr, monkeypatch, s.flat, s.cam, s.cfg, env)
        assert np.array_equal(got.accum, s.ref), (env, _diff(got.accum, s.ref))
        assert np.array_equal(got.rgb8, s.ref8), env
        # RTX_WIDE concerns the other kernels' trees: k_trace_lds still renders, in the table's form; every other kernel says 0
        lds = "RTX_TRACE_KERNEL" not in env
        assert (_kernel(rtsr, got) == "k_trace_lds") == lds, (env, _kernel(rtsr, got))
        assert got.stats.trace_variant == (mc.expected_variant(case_id) if lds else 0), (env, got.stats.trace_variant)


@pytest.mark.parametrize("case_id", ["offset", "bvh_wider", "mixed", "reversed"])
def test_rays_from_the_movers_centres_equal_the_cpu_core(rtsr, orc, case_id):
    """The closed-form rays of tests/test_motion_cases.py (which holds the CPU core to t = r) through Scene.cast_rays with
    per-ray times: hit or miss, t, normal, front face and material equal core_world_hit_mat's bit for bit, blocked rays too."""
    s = _get(rtsr, orc, case_id)
    n_hit = 0
    for t, origins, dirs, radii, blocked in mc.centre_rays(case_id, s.movers):
        hits = s.scene.cast_rays(origins, dirs, np.full(len(origins), t))
        for r in range(len(origins)):
            rec = orc.core_world_hit_mat(s.flat.arrays_ptr(), origins[r], dirs[r], time=t)
            if rec is None:
                assert hits.ids[r, 0] == 0 and np.isinf(hits.t[r]), (t, r)
                continue
            n_hit += 1
            assert hits.ids[r, 0] == 1 and hits.t[r] == rec["t"], (t, r, hits.t[r], rec["t"])
            assert tuple(hits.normal[r]) == rec["normal"] and hits.ids[r, 3] == int(rec["front_face"]), (t, r)
            assert hits.ids[r, 1] == rec["mat"], (t, r, hits.ids[r], rec["mat"])
    assert n_hit >= 3 * len(s.movers) * 3


@pytest.mark.parametrize("case_id,shutter", mc.SHUTTERS, ids=lambda v: str(v))
def test_list_form_through_k_trace_world(rtsr, orc, case_id, shutter):
    """The first 40 objects as a plain HittableList: no tree, so the frame is the literal object graph's at ANY shutter, outside
    the spheres' intervals and with time0 == time1 (NaN roots, in list order) too.  k_trace_world's per-sphere f32 box
    (WD_TIME_BOX) exists only for time0 < time1."""
    b, world, cam, cfg, movers = mc.build(rtsr, case_id, shutter, as_list=True)
    h = rtsr.image_height(cfg)
    flat = b.flatten(world)
    a1, r1 = orc.o1_render(b.graph_ptr(), world, cam, cfg, h, threads=16)
    scene = flat.upload()
    got = scene.render(cam, cfg, want_stats=True)
    print("\n[motion cases] list form of %s shutter %d: kernel %s, %s" % (case_id, shutter, _kernel(rtsr, got), _diff(got.accum, a1)))
    assert _same(got.accum, a1), _diff(got.accum, a1)
    assert np.array_equal(got.rgb8, r1)
    assert _kernel(rtsr, got) == "k_trace_world" and got.stats.trace_variant == 0
    flags = scene.array("world_desc").view(np.int32).reshape(mc.N_LIST, -1)[:, 0]
    ordered = [t0 < t1 for (_, _, t0, t1, _) in movers]
    assert int(((flags & WD_TIME_BOX) != 0).sum()) == sum(ordered)
    if case_id in ("degenerate", "reversed"):
        assert not any(ordered) and not (flags & WD_TIME_BOX).any()
    else:
        assert all(ordered) and len(movers) == 29


@pytest.mark.parametrize("shutter", [0, 1])
def test_a_shutter_that_straddles_the_interval_falls_back_to_static_boxes(rtsr, orc, monkeypatch, shutter):
    """Ray times beyond the BVH's interval: a lerped box is no bound there, and no frame is claimed
    (tests/test_gpu_compat.py: test_time_aware_boxes_on_the_device); the launcher must take the static boxes."""
    s = _get(rtsr, orc, "straddle", shutter)
    assert _kernel(rtsr, s.screen) == "k_trace_lds"
    assert s.screen.stats.trace_variant == mc.expected_variant("straddle", shutter) == mc.COMMON_RATIO
    plain = _render_under(rtsr, monkeypatch, s.flat, s.cam, s.cfg, {"RTX_MOTION": "0"})
    assert plain.stats.trace_variant == mc.COMMON_RATIO
    assert np.array_equal(s.screen.accum, plain.accum), _diff(s.screen.accum, plain.accum)
    assert np.array_equal(s.screen.rgb8, plain.rgb8)
    assert np.isfinite(s.screen.accum).all() and s.screen.accum.std() > 0.1


def test_an_empty_sphere_interval_leaves_the_static_spheres_alone(rtsr, orc, monkeypatch):
    """time0 == time1 on every mover.  One ratio for every record would be x / 0, its product with a static sphere's c1 - c0 = 0
    a NaN, and every STATIC sphere of the scene would take a NaN centre (Sphere::hit never reads the time): the launcher must
    not share the ratio.  The movers themselves answer with t = NaN as in the reference (tests/test_motion_cases.py), so the
    frame depends on the order of the tests and is compared with the same kernel in the same walk order only.
    Before plan_lds asked for time0 != time1 the variant word read 5 (common ratio) where 1 is expected.  The frames could not
    tell: one such mover closes the sky for every ray, and a k_trace_lds world has no other light -- all 6144 pixels are black
    under either rule ("Ray time"), which also is what "not the sky's" comes to below."""
    s = _get(rtsr, orc, "degenerate")
    assert _kernel(rtsr, s.screen) == "k_trace_lds"
    assert s.screen.stats.trace_variant == mc.expected_variant("degenerate") == mc.TIME_BOXES
    own = _render_under(rtsr, monkeypatch, s.flat, s.cam, s.cfg, {"RTX_MV_COMMON": "0"})
    assert own.stats.trace_variant == mc.TIME_BOXES
    assert _same(s.screen.accum, own.accum), _diff(s.screen.accum, own.accum)
    assert np.array_equal(s.screen.rgb8, own.rgb8)
    # the static spheres are in the picture: over the pixels where the scene WITHOUT the movers shows anything but sky, the
    # frame is not the sky's
    b0, world0, cam, cfg, _ = mc.build(rtsr, "degenerate", with_movers=False)
    flat0 = b0.flatten(world0)  # (kept: arrays_ptr points into it)
    a0, _ = orc.o2_render(flat0.arrays_ptr(), cam, cfg, s.h, threads=16)
    sky = np.zeros(3)
    for _ in range(cfg.samples_per_pixel):
        sky = sky + np.array(mc.SKY)
    shown = (a0 != sky).any(axis=2)
    assert 0.3 < shown.mean() < 1.0
    mean = s.screen.accum[shown].mean(axis=0)
    print("\n[motion cases] degenerate: %d of %d pixels show the static scene, the frame's mean there %s against the sky's %s, %d black pixels" % (
        int(shown.sum()), shown.size, mean, sky, int((s.screen.accum == 0).all(axis=2).sum())))
    assert not np.array_equal(mean, sky)


@pytest.mark.parametrize("case_id", ["offset", "far_offset", "mixed"])
def test_f32_fast_mode_cannot_see_the_culling_or_the_shared_ratio(rtsr, orc, monkeypatch, case_id):
    """rtx_scene_upload_f32: the frame with default switches equals the f32 frames under RTX_MOTION=0 and RTX_MV_COMMON=0 bit
    for bit (far_offset: time - 1000 in float), and its mean is within tests/test_gpu_f32.py's bound of the f64 frame's."""
    s = _get(rtsr, orc, case_id)
    fast = s.flat.upload(f32=True).render(s.cam, s.cfg, want_stats=True)
    assert _kernel(rtsr, fast) == "k_trace_lds" and fast.stats.trace_variant == mc.expected_variant(case_id)
    for env in ({"RTX_MOTION": "0"}, {"RTX_MV_COMMON": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        other = s.flat.upload(f32=True).render(s.cam, s.cfg, want_stats=True)
        for k in env:
            monkeypatch.delenv(k)
        assert other.stats.trace_variant == mc.expected_variant(case_id, 0, env), env
        assert np.array_equal(fast.accum, other.accum), (env, _diff(fast.accum, other.accum))
        assert np.array_equal(fast.rgb8, other.rgb8), env
    a, f = s.ref / s.cfg.samples_per_pixel, fast.accum / s.cfg.samples_per_pixel
    assert np.isfinite(f).all()
    rel = abs(f.mean() - a.mean()) / a.mean()
    print("\n[motion cases] %s f32: frame mean %.6f against %.6f in f64, relative %.3g" % (case_id, f.mean(), a.mean(), rel))
    assert rel < 5e-3, (case_id, a.mean(), f.mean())
