"""Instance trees on the GPU: every entry point and mode gives, bit for bit, the frame of the hoisted spelling (the members written
into the world list), which is the parent's code path, unchanged.  Scenes: tests/instance_scenes.py, N = 60 and N = 1024."""
import numpy as np
import pytest

from instance_scenes import box_field, field_cam_cfg, tie_cam_cfg, tie_scene

pytestmark = pytest.mark.gpu

RTX_KERNEL_SIMPLE, RTX_KERNEL_WORLD, RTX_KERNEL_NEE = 0, 6, 8
FRAMES = {60: dict(width=72, spp=16), 1024: dict(width=48, spp=16, depth=12)}


def _pair(rtsr, n, **kw):
    """(flat, scene) of the hoisted and of the instanced spelling, camera, config, height."""
    cam, cfg, h = field_cam_cfg(rtsr, n=n, **FRAMES[n])
    out = []
    for spelling in ("hoisted", "instanced"):
        b, w = box_field(rtsr, spelling, n=n, **kw)
        flat = b.flatten(w)
        out.append((b, flat, flat.upload()))
    assert out[0][1].instances()["n_trees"] == 0 and out[1][1].instances()["n_trees"] == 1
    return out[0], out[1], cam, cfg, h


@pytest.mark.parametrize("kernel", ["default", "simple"])
@pytest.mark.parametrize("n", [60, 1024])
def test_one_shot_render(rtsr, orc, monkeypatch, n, kernel):
    """rtx_render(instanced) == rtx_render(hoisted) == O2(instanced); k_trace_world by default, k_trace_simple when forced."""
    if kernel == "simple":
        monkeypatch.setenv("RTX_TRACE_KERNEL", "simple")
    (bh, fh, sh), (bi, fi, si), cam, cfg, h = _pair(rtsr, n)
    hoisted = sh.render(cam, cfg, want_stats=True)
    inst = si.render(cam, cfg, want_stats=True)
    want = RTX_KERNEL_WORLD if kernel == "default" else RTX_KERNEL_SIMPLE
    assert inst.stats.trace_kernel == want and hoisted.stats.trace_kernel == want
    o2, o2_rgb8 = orc.o2_render(fi.arrays_ptr(), cam, cfg, h, threads=16)
    bad = int((inst.accum != hoisted.accum).any(axis=2).sum())
    print("N %d %s: %d of %d pixels differ from the hoisted frame, %d from O2" % (n, kernel, bad, h * cfg.image_width,
                                                                                int((inst.accum != o2).any(axis=2).sum())))
    assert bad == 0 and np.array_equal(inst.rgb8, hoisted.rgb8)
    assert np.array_equal(inst.accum, o2) and np.array_equal(inst.rgb8, o2_rgb8)


@pytest.mark.parametrize("n", [60, 1024])
def test_shards_progressive_adaptive_multi(rtsr, n):
    """The instanced frame against the hoisted one-shot frame: three shards (each a progressive handle over its shard, the
    whole budget in one add) reassembled; a whole-image handle split 5 + 11; an adaptive until_adaptive run (frame, pixel_spp,
    samples) against the hoisted scene's; rtx_multi_render with two shards on one device."""
    (bh, fh, sh), (bi, fi, si), cam, cfg, h = _pair(rtsr, n)
    whole = sh.render(cam, cfg).accum
    # three shards reassembled
    got = np.zeros_like(whole)
    for s in range(3):
        prog = si.progressive(cam, cfg, shard=(s, 3, 1))
        prog.add(cfg.samples_per_pixel)
        got[[j for j in range(h) if j % 3 == s]] = prog.screen().accum
        del prog
    assert np.array_equal(got, whole)
    # a progressive handle split 5 + 11
    assert cfg.samples_per_pixel == 16
    prog = si.progressive(cam, cfg)
    prog.add(5)
    prog.add(11)
    assert np.array_equal(prog.screen().accum, whole)
    del prog
    # adaptive: frames, per-pixel sample counts and the sample total
    res = []
    for scene in (sh, si):
        prog = scene.progressive(cam, cfg)
        st = prog.until_adaptive(2, 2, 0.05)
        res.append((prog.screen().accum, prog.screen().rgb8, prog.pixel_spp(), st.samples))
        del prog
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert np.array_equal(res[0][2], res[1][2]) and res[0][3] == res[1][3] and res[0][3] > 0
    # rtx_multi_render: two shards on one device
    multi = rtsr.MultiScene(fi, 2, device_ids=[0, 0]).render(cam, cfg)
    assert np.array_equal(multi.accum, whole)


@pytest.mark.parametrize("n", [60, 1024])
def test_denoiser_features_and_frame(rtsr, n):
    (bh, fh, sh), (bi, fi, si), cam, cfg, h = _pair(rtsr, n)
    res = []
    for scene in (sh, si):
        prog = scene.progressive(cam, cfg)
        prog.add(cfg.samples_per_pixel)
        albedo, normal = prog.features(2)
        d = prog.denoise()
        res.append((albedo, normal, d.accum, d.rgb8))
        del prog
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
    assert res[0][0].std() > 0.0


@pytest.mark.parametrize("n", [60, 1024])
def test_light_sampling_with_the_lamp_as_a_member(rtsr, n):
    """The lamp, a plain sphere light, as the first MEMBER: an ordinary slot, so a sampled light exactly as when hoisted."""
    (bh, fh, sh), (bi, fi, si), cam, cfg, h = _pair(rtsr, n, lamp_member=True)
    assert fi.lights() == fh.lights() and fi.lights()["n_sphere_lights"] == 1
    hoisted = sh.render(cam, cfg, light_sampling=True, want_stats=True)
    inst = si.render(cam, cfg, light_sampling=True, want_stats=True)
    assert inst.stats.trace_kernel == RTX_KERNEL_NEE
    assert np.array_equal(inst.accum, hoisted.accum) and np.array_equal(inst.rgb8, hoisted.rgb8)
    assert not np.array_equal(inst.accum, si.render(cam, cfg).accum)  # the estimator did sample the lamp


def test_exact_ties_through_k_trace_world(rtsr, orc):
    cam, cfg, h = tie_cam_cfg(rtsr)
    frames = {}
    for order in ("AB", "BA"):
        b, w = tie_scene(rtsr, order, "list")
        o1, _ = orc.o1_render(b.graph_ptr(), w, cam, cfg, h, threads=8)
        b2, w2 = tie_scene(rtsr, order, "instanced")
        flat = b2.flatten(w2)
        got = flat.upload().render(cam, cfg, want_stats=True)
        assert got.stats.trace_kernel == RTX_KERNEL_WORLD
        assert np.array_equal(got.accum, o1), "order %s: %d pixels differ" % (order, int((got.accum != o1).any(axis=2).sum()))
        frames[order] = o1
    assert int((frames["AB"] != frames["BA"]).any(axis=2).sum()) > 20


@pytest.mark.parametrize("n", [60, 1024])
def test_counting_kernel(rtsr, n):
    """rtx_render_count: the same samples, rays and scatters as the hoisted spelling; at N = 1024 the rectangle tests per ray
    within the cap of the CPU test (one tenth of the hoisted scan's 6 N)."""
    (bh, fh, sh), (bi, fi, si), cam, cfg, h = _pair(rtsr, n)
    ch, ci = sh.render_count(cam, cfg), si.render_count(cam, cfg)
    for name in ("samples", "rays", "scatters"):
        assert getattr(ci, name) == getattr(ch, name) and getattr(ci, name) > 0, name
    per_ray_h, per_ray_i = ch.rect_tests / ch.rays, ci.rect_tests / ci.rays
    print("N %d: rect tests per ray hoisted %.1f, instanced %.2f (ratio %.5f)" % (n, per_ray_h, per_ray_i, per_ray_i / per_ray_h))
    assert per_ray_h >= 6 * n
    if n == 1024:
        assert per_ray_i <= 0.1 * per_ray_h
    else:
        assert per_ray_i < per_ray_h


@pytest.mark.parametrize("kernel", ["default", "simple"])
@pytest.mark.parametrize("n", [60, 1024])
def test_f32_mode_equals_the_float_oracle(rtsr, orc, monkeypatch, n, kernel):
    """The field reaches none of the platform functions (no noise, medium or image texture): tier A of
    tests/test_gpu_f32_parity.py, so the f32 kernels equal O2f bit for bit -- in both spellings."""
    if kernel == "simple":
        monkeypatch.setenv("RTX_TRACE_KERNEL", "simple")
    cam, cfg, h = field_cam_cfg(rtsr, n=n, **FRAMES[n])
    frames = []
    for spelling in ("hoisted", "instanced"):
        b, w = box_field(rtsr, spelling, n=n)
        flat = b.flatten(w)
        scene = flat.upload(f32=True)
        assert scene.is_f32
        got = scene.render(cam, cfg, want_stats=True)
        assert rtsr.trace_kernel_name(got.stats.trace_kernel) == ("k_trace_world" if kernel == "default" else "k_trace_simple")
        ref, ref8 = orc.o2f_render(flat.arrays_ptr(), cam, cfg, h, threads=16)
        bad = int((got.accum != ref).any(axis=2).sum())
        print("f32 N %d %s %s: %d of %d pixels differ from O2f" % (n, spelling, kernel, bad, h * cfg.image_width))
        assert bad == 0 and np.array_equal(got.rgb8, ref8)
        frames.append(got.accum)
    assert np.array_equal(frames[0], frames[1])


def test_the_tree_is_faster_than_the_scan_at_1024(rtsr):
    """N = 1024 at 256 x 256 x 16 spp: the instanced trace_ms is below the hoisted trace_ms of the same run (the hoisted path
    is the parent's code).  Both are warmed up once; the figures are printed."""
    cam, cfg, h = field_cam_cfg(rtsr, n=1024, width=256, spp=16, depth=30)
    cfg.aspect_ratio = 1.0
    h = rtsr.image_height(cfg)
    assert (cfg.image_width, h, cfg.samples_per_pixel) == (256, 256, 16)
    ms, frames = {}, {}
    for spelling in ("hoisted", "instanced"):
        b, w = box_field(rtsr, spelling, n=1024)
        scene = b.flatten(w).upload()
        scene.render(cam, cfg)
        runs = [scene.render(cam, cfg, want_stats=True) for _ in range(3)]
        assert runs[0].stats.trace_kernel == RTX_KERNEL_WORLD
        ms[spelling] = sorted(r.stats.trace_ms for r in runs)
        frames[spelling] = runs[0].accum
    print("trace_ms at N = 1024, 256 x 256 x 16 spp (three runs each): hoisted %s, instanced %s" % (ms["hoisted"], ms["instanced"]))
    assert np.array_equal(frames["hoisted"], frames["instanced"])
    assert ms["instanced"][-1] < ms["hoisted"][0]
