"""The order of a pass's items (csrc/core/item_order.hpp, RTX_ITEM_GROUP) cannot change a frame: streams are keyed by (pixel,
sample), every sample owns its slot of the sample buffer and the reduction adds slots in sample order.  Every kernel family is
rendered with groups of 1, 3, 8 and 64 pixels and with its default, and compared bit for bit with the same render in the
row-strip order (RTX_ITEM_GROUP = 2^30: one group).  Frames of 37 x 24 = 888 = 13 x 64 + 56 pixels, 5 and 67 samples: no group
size divides the pixel count or the sample count, and the last group of every order is short."""
import numpy as np
import pytest

from test_gpu_progressive import _rel_err, _setup, _with

pytestmark = pytest.mark.gpu

STRIP = "1073741824"                    # one group: the row-strip order
GROUPS = ("1", "3", "8", "64", None)    # None: the kernel family's default
WIDTH, ASPECT = 37, 1.5
SPPS = (5, 67)
COUNTERS = ("samples", "rays", "box_tests", "sphere_tests", "moving_sphere_tests", "rect_tests", "triangle_tests", "scatters",
            "texels", "perlin_calls")

CASES = [  # (name, scene id, environment, f32 upload, trace kernel's name)
    ("lds_ring", 100, {}, False, "k_trace_lds"),
    ("lds_time_boxes_no_ring", 13, {}, False, "k_trace_lds"),
    ("vote", 100, {"RTX_SCENE_LDS": "0"}, False, "k_trace_vote"),
    ("world", 100, {"RTX_TRACE_KERNEL": "world"}, False, "k_trace_world"),
    ("wavefront", 100, {"RTX_TRACE_KERNEL": "wavefront"}, False, "k_wf_trace"),
    ("simple", 100, {"RTX_TRACE_KERNEL": "simple"}, False, "k_trace_simple"),
    ("lds_f32", 100, {}, True, "k_trace_lds"),
]


def _upload_under(monkeypatch, flat, env, group, f32=False):
    """The scene uploaded with the switches of env and RTX_ITEM_GROUP = group (None: unset); switches are read at upload."""
    env = dict(env)
    if group is not None:
        env["RTX_ITEM_GROUP"] = group
    monkeypatch.delenv("RTX_ITEM_GROUP", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene = flat.upload(f32=f32)
    for k in env:
        monkeypatch.delenv(k)
    return scene


def _flat(rtsr, sid):
    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(sid)
    cfg = rtsr.Config.new(ASPECT, WIDTH, SPPS[0], 50, 10, seed=3, background=bg)
    assert rtsr.image_height(cfg) * WIDTH == 888
    return b, b.flatten(world), cam, cfg


@pytest.mark.parametrize("name,sid,env,f32,kernel", CASES, ids=[c[0] for c in CASES])
def test_every_group_size_renders_the_row_strip_frame(rtsr, monkeypatch, name, sid, env, f32, kernel):
    b, flat, cam, cfg = _flat(rtsr, sid)
    ref_scene = _upload_under(monkeypatch, flat, env, STRIP, f32)
    st = ref_scene.render_device(cam, cfg, want_stats=True)
    assert kernel in rtsr.trace_kernel_name(st.trace_kernel), rtsr.trace_kernel_name(st.trace_kernel)
    refs = {spp: ref_scene.render(cam, _with(rtsr, cfg, samples_per_pixel=spp)) for spp in SPPS}
    for group in GROUPS:
        scene = _upload_under(monkeypatch, flat, env, group, f32)
        for spp in SPPS:
            got = scene.render(cam, _with(rtsr, cfg, samples_per_pixel=spp))
            assert got.accum.dtype == np.float64
            bad = int((got.accum != refs[spp].accum).any(axis=2).sum())
            assert bad == 0, "%s, groups of %s, %d spp: %d of 888 pixels differ" % (name, group, spp, bad)
            assert np.array_equal(got.rgb8, refs[spp].rgb8), (name, group, spp)
        del scene


@pytest.mark.parametrize("env", [{}, {"RTX_TRACE_KERNEL": "world"}], ids=["lds", "world"])
def test_passes_of_unequal_length_two_in_flight(rtsr, monkeypatch, env):
    """A sample buffer of six planes: 67 samples go in pipelined passes of 3, the last of them 1 sample long -- every pass has
    its own order (P S changes with S) in its own half of the buffer."""
    b, flat, cam, cfg = _flat(rtsr, 100)
    c = _with(rtsr, cfg, samples_per_pixel=67, sample_buffer_bytes=6 * 24 * 888)
    ref = _upload_under(monkeypatch, flat, env, STRIP).render(cam, c)
    one = _upload_under(monkeypatch, flat, env, STRIP).render(cam, _with(rtsr, cfg, samples_per_pixel=67))
    assert np.array_equal(ref.accum, one.accum)
    for group in GROUPS:
        got = _upload_under(monkeypatch, flat, env, group).render(cam, c)
        assert np.array_equal(got.accum, ref.accum) and np.array_equal(got.rgb8, ref.rgb8), group


def test_a_shard_renders_the_same_rows(rtsr, monkeypatch):
    b, flat, cam, cfg = _flat(rtsr, 100)
    shard = (1, 3, 2)

    def frame(group, spp):
        prog = _upload_under(monkeypatch, flat, {}, group).progressive(cam, _with(rtsr, cfg, samples_per_pixel=spp), shard=shard)
        prog.add(spp)
        S, Q = prog.moments()
        return S, Q, prog.screen(want_accum=False).rgb8

    for spp in SPPS:
        ref = frame(STRIP, spp)
        assert ref[0].shape[0] * ref[0].shape[1] % 64 != 0
        for group in GROUPS:
            got = frame(group, spp)
            for k in range(3):
                assert np.array_equal(got[k], ref[k]), (group, spp, k)


def test_the_counting_render_does_the_same_work(rtsr, monkeypatch):
    b, flat, cam, cfg = _flat(rtsr, 100)
    c = _with(rtsr, cfg, samples_per_pixel=67)
    ref = _upload_under(monkeypatch, flat, {}, STRIP).render_count(cam, c)
    assert ref.samples == 888 * 67 and ref.rays > ref.samples and ref.box_tests > ref.rays
    for group in GROUPS:
        got = _upload_under(monkeypatch, flat, {}, group).render_count(cam, c)
        for f in COUNTERS:
            assert getattr(got, f) == getattr(ref, f), (group, f)


@pytest.mark.parametrize("env", [{}, {"RTX_SCENE_LDS": "0"}], ids=["lds", "vote"])
def test_an_adaptive_pass_over_a_list_no_group_size_divides(rtsr, monkeypatch, env):
    """After 8 uniform samples all but 437 pixels retire (437 = 3 x 145 + 2 = 8 x 54 + 5 = 64 x 6 + 53); two adaptive rounds of
    5 samples then trace the list of those 437, whose last group is short for every group size."""
    b, flat, cam, cfg = _flat(rtsr, 100)
    c = _with(rtsr, cfg, samples_per_pixel=24)
    keep = 437
    assert all(keep % p for p in (3, 8, 64))

    def run(group, target=None):
        prog = _upload_under(monkeypatch, flat, env, group).progressive(cam, c)
        prog.add(8)
        if target is None:
            S, Q = prog.moments()
            r = np.sort(_rel_err(S, Q, 8).ravel())
            assert r[-keep - 1] < r[-keep]
            target = float(r[-keep - 1])  # the largest error that retires
        st = prog.add_adaptive(5, 6, target, want_stats=True)
        n_p = prog.pixel_spp()
        assert int((n_p == prog.spp_done).sum()) == keep and st.samples == 5 * keep
        prog.add_adaptive(5, 6, 0.0)  # (nothing retires at 0: the same list again)
        S, Q = prog.moments()
        return target, (prog.pixel_spp(), S, Q, prog.screen(want_accum=False).rgb8)

    target, ref = run(STRIP)
    assert int((ref[0] == 18).sum()) == keep and int((ref[0] == 8).sum()) == 888 - keep
    for group in GROUPS:
        _, got = run(group, target)
        for k in range(4):
            assert np.array_equal(got[k], ref[k]), (group, k)
