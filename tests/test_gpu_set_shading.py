"""Scene.set_shading on the device (rtx_scene_set_shading: k_set_shading, and k_refresh_lights after a texture edit).

Two judges, neither the code under test: the resident ARRAYS after an edit are byte-equal to those of the host-edited flat
scene uploaded afresh (rtx_flat_set_shading, which tests/test_set_shading_host.py holds to a fresh flatten and to the oracle),
and every ENTRY POINT on the edited scene answers bit for bit as on a FRESH upload of the same world built from scratch with
the new values.  f64 frames also equal the CPU oracle's frame of the edited flat arrays.  Frames are 48 x 27 at 4 spp.
Nothing here is statistical."""
import os

import numpy as np
import pytest

import cast_rays_cases as cc
import update_cases
from shading_cases import (CASES, DEVICE_KEPT, DEVICE_WRITTEN, KERNEL_OF, LIGHT, MATERIAL, MATERIAL32, REST, VARIANTS, book1, book1_edits, build, cam_cfg,
                           call_set_shading, edits_for, pairs, refusals, sequence)

pytestmark = pytest.mark.gpu
SWITCHES = ("RTX_TRACE_KERNEL", "RTX_WIDE", "RTX_MAT_LDS")


def _upload(flat, env=None, f32=False):
    """flat.upload() under the given RTX_* switches (read once per upload)."""
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env or {})
    try:
        return flat.upload(f32=f32)
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _device(scene, names=DEVICE_WRITTEN + DEVICE_KEPT):
    return {k: scene.array(k) for k in names}


def _assert_equal(now, want, what):
    for k in want:
        assert now[k].size == want[k].size and np.array_equal(now[k], want[k]), "%s: %s differs in %d bytes" % (
            what, k, int((now[k] != want[k]).sum()) if now[k].size == want[k].size else -1)


def _same_screen(a, b, what):
    bad = int((a.accum != b.accum).any(axis=2).sum())
    assert bad == 0 and np.array_equal(a.rgb8, b.rgb8), "%s: %d pixels differ" % (what, bad)


def _kernel(rtsr, screen):
    return rtsr.trace_kernel_name(screen.stats.trace_kernel)


def _rays(n, seed):
    return update_cases.seeded_rays(n, seed, (-0.5, 0.3, -0.5), (6.5, 3.5, 6.5), (0.3, 2.2))


# ---- 1. the arrays
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name,k", pairs())
def test_edited_arrays_equal_the_host_edited_scene_uploaded_fresh(rtsr, name, k, f32):
    """materials, textures, entries, world_desc and (f64) lights: those of the host-edited flat scene uploaded fresh -- and of
    the world built from scratch with the new values; every other array: its bytes from before the edit.  Then back to rest."""
    case = build(rtsr, name)
    flat = case.flatten()
    scene = _upload(flat, f32=f32)
    first = _device(scene)
    variant = VARIANTS[name][k]
    edits = edits_for(case, flat, variant)
    scene.set_shading(edits)
    flat.set_shading(edits)
    want = _device(_upload(flat, f32=f32))
    now = _device(scene)
    what = "%s %d %s" % (name, k, "f32" if f32 else "f64")
    _assert_equal(now, want, what)
    _assert_equal(now, _device(_upload(build(rtsr, name, k).flatten(), f32=f32)), what + " (built from scratch)")
    assert any(not np.array_equal(now[a], first[a]) for a in DEVICE_WRITTEN), what
    _assert_equal({a: now[a] for a in DEVICE_KEPT}, {a: first[a] for a in DEVICE_KEPT}, what + " (untouched)")
    if f32:  # the (float) cast of the f64 values
        assert len(now["lights"]) == 0
        m64, m32 = flat.array("materials").view(MATERIAL), now["materials"].view(MATERIAL32)
        assert np.array_equal(m32["albedo"], m64["albedo"].astype(np.float32)) and np.array_equal(m32["param"], m64["param"].astype(np.float32))
    back = edits_for(case, flat, {key: REST[name][key] for key in variant})
    scene.set_shading(back)
    _assert_equal(_device(scene), first, what + " back at rest")
    scene.set_shading([])  # n = 0: nothing launched


# ---- 2. frames under every kernel family
def _frames(rtsr, orc, name, k, env, expect, f32):
    case, fresh_case = build(rtsr, name), build(rtsr, name, k)
    flat, fresh_flat = case.flatten(), fresh_case.flatten()
    scene, fresh = _upload(flat, env, f32), _upload(fresh_flat, env, f32)
    cam, cfg, h = cam_cfg(rtsr, case)
    assert (cfg.image_width, h, cfg.samples_per_pixel) == (48, 27, 4)
    what = "%s %d %s %s" % (name, k, env, "f32" if f32 else "f64")
    rest = scene.render(cam, cfg)
    edits = edits_for(case, flat, VARIANTS[name][k])
    scene.set_shading(edits)
    got, want = scene.render(cam, cfg, want_stats=True), fresh.render(cam, cfg, want_stats=True)
    assert want.accum.std() > 0.01
    _same_screen(got, want, what)
    assert _kernel(rtsr, got) == _kernel(rtsr, want), what
    if expect is not None and not f32:
        assert _kernel(rtsr, got) == expect, what
    if not f32:
        flat.set_shading(edits)
        o2, o2_8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=4)
        assert np.array_equal(got.accum, o2) and np.array_equal(got.rgb8, o2_8), what
    return rest, got


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_frames_on_the_edited_scene_equal_the_fresh_upload(rtsr, orc, name, f32):
    """The default kernel on every variant, then every forced family on variant 0: `simple` and `world` take any world, `vote`
    and the wavefront integrator a world of one BVH beside plain primitives (Case.vote) and k_trace_world runs where they do
    not apply; by default a world of one sphere BVH runs k_trace_lds.  At least one variant must SHOW in the frame."""
    case = build(rtsr, name)
    default = "k_trace_lds" if case.lds else ("k_trace_vote" if case.vote else "k_trace_world")
    shown = False
    for k in range(len(VARIANTS[name])):
        rest, got = _frames(rtsr, orc, name, k, {}, default, f32)
        shown = shown or bool((rest.accum != got.accum).any())
    assert shown, name
    for kernel in ("simple", "world", "vote", "wavefront"):
        expect = KERNEL_OF[kernel] if kernel in ("simple", "world") or case.vote else "k_trace_world"
        _frames(rtsr, orc, name, 0, {"RTX_TRACE_KERNEL": kernel}, expect, f32)


@pytest.mark.parametrize("mat_lds", ["0", "1"])
@pytest.mark.parametrize("n", [16, 17, 64, 65])
def test_tables_in_lds_or_in_global_memory(rtsr, orc, n, mat_lds):
    """16 / 17 and 64 / 65 materials and textures: the counts at which the wide k_trace_vote (<= 16) and k_trace_world (<= 64)
    move both tables into LDS -- copied from global memory at every launch, so the LAST record's edit must show either way."""
    name = "tables_%d" % n
    for env, expect in (({"RTX_WIDE": "1"}, "k_trace_vote"), ({"RTX_TRACE_KERNEL": "world"}, "k_trace_world"),
                        ({"RTX_TRACE_KERNEL": "world", "RTX_WIDE": "1"}, "k_trace_world")):
        rest, got = _frames(rtsr, orc, name, 0, dict(env, RTX_MAT_LDS=mat_lds), expect, False)
        assert (rest.accum != got.accum).any(), (name, env)  # the ground wears the last material
    _frames(rtsr, orc, name, 0, {"RTX_TRACE_KERNEL": "world", "RTX_MAT_LDS": mat_lds}, "k_trace_world", True)


def test_book1_every_material_edited(rtsr, orc):
    """Catalogue scene 100 through k_trace_lds with every material edited by its kind: arrays and frame against the
    host-edited flat scene uploaded fresh, the frame against the CPU oracle on that flat scene, under every kernel family."""
    b, world, cam, bg = book1(rtsr)
    flat = b.flatten(world)
    edits = book1_edits(flat)
    cfg = rtsr.Config.new(1.5, 48, 4, 8, 4, seed=31, background=bg)
    h = rtsr.image_height(cfg)
    edited = b.flatten(world)
    edited.set_shading(edits)
    o2, o2_8 = orc.o2_render(edited.arrays_ptr(), cam, cfg, h, threads=4)
    for kernel in (None, "simple", "vote", "world", "wavefront"):
        env = {"RTX_TRACE_KERNEL": kernel} if kernel else {}
        scene, fresh = _upload(flat, env), _upload(edited, env)
        rest = scene.render(cam, cfg)
        scene.set_shading(edits)
        if kernel is None:
            _assert_equal(_device(scene), _device(fresh), "book1")
        got, want = scene.render(cam, cfg, want_stats=True), fresh.render(cam, cfg, want_stats=True)
        assert _kernel(rtsr, got) == _kernel(rtsr, want) == (KERNEL_OF[kernel] if kernel else "k_trace_lds")
        _same_screen(got, want, "book1 %s" % kernel)
        assert np.array_equal(got.accum, o2) and np.array_equal(got.rgb8, o2_8), kernel
        assert (rest.accum != got.accum).any(axis=2).mean() > 0.5


# ---- 3. exact meaning
def test_a_ray_at_a_light_returns_the_new_colour_by_bit_pattern(rtsr):
    """trace_rays at max_depth = 1: a ray that ends on a light returns its emitted colour, one that ends on the floor 0."""
    aim = {"cornell_light": [("light", (2.78, 3.0, 2.8), (0.0, 1.0, 0.0))],
           "two_lamps": [("rect", (1.9, 1.0, 2.7), (0.0, 1.0, 0.0)), ("ball", (4.3, 1.0, 2.7), (0.0, 1.0, 0.0))]}
    floor = {"cornell_light": ((0.6, 1.0, 0.6), (0.0, -1.0, 0.0)), "two_lamps": ((0.5, 1.0, 0.5), (0.0, -1.0, 0.0))}
    for name, lights in aim.items():
        case = build(rtsr, name)
        flat = case.flatten()
        for f32 in (False, True):
            scene = _upload(flat, f32=f32)
            for k, variant in enumerate(VARIANTS[name]):
                values = dict(REST[name])
                values.update(variant)
                scene.set_shading(edits_for(case, flat, variant))
                o = np.array([p for _, p, _ in lights] + [floor[name][0]], dtype=np.float64)
                d = np.array([q for _, _, q in lights] + [floor[name][1]], dtype=np.float64)
                got = scene.trace_rays(o, d, spp=1, max_depth=1, background=(0.0, 0.0, 0.0)).sum
                for r, (key, _, _) in enumerate(lights):
                    want = np.array(values[key], dtype=np.float64)
                    if f32:
                        want = want.astype(np.float32).astype(np.float64)
                    assert got[r].tobytes() == want.tobytes(), (name, k, key, f32, got[r], want)
                assert not got[-1].any(), (name, k, got[-1])
                scene.set_shading(edits_for(case, flat, {key: REST[name][key] for key in variant}))


# ---- 4. queries and estimators
_PAIRS = {}


def _pair(rtsr, name):
    """(edited scene, fresh scene, case, the flat scene at rest): f64, default switches, variant 0; built once per case."""
    if name not in _PAIRS:
        case = build(rtsr, name)
        flat = case.flatten()
        scene = _upload(flat)
        scene.set_shading(edits_for(case, flat, VARIANTS[name][0]))
        _PAIRS[name] = (scene, _upload(build(rtsr, name, 0).flatten()), case, flat)
    return _PAIRS[name]


@pytest.mark.parametrize("name", ["cornell_light", "shared_texture", "checker_children", "fog", "noise_lamp"])
def test_queries_on_the_edited_scene_equal_the_fresh_upload(rtsr, name):
    """cast_rays, all columns (the material ids do not change); trace_rays without and -- where the world has sampled lights --
    with light sampling; render(light_sampling=True); a progressive handle made AFTER the edit with its features."""
    scene, fresh, case, flat = _pair(rtsr, name)
    o, d = _rays(1500, 41)
    hm, hf = scene.cast_rays(o, d, seed=1, stream_step=1), fresh.cast_rays(o, d, seed=1, stream_step=1)
    assert hf.hit.sum() >= 200
    for col in ("t", "p", "normal", "uv"):
        a, b = getattr(hm, col), getattr(hf, col)
        assert cc.same_bits(a.reshape(len(o), -1), b.reshape(len(o), -1)).all(), col
    assert np.array_equal(hm.ids, hf.ids)
    bg = case.bg
    lit = flat.lights()["n_lights"] > 0
    for nee in ([False, True] if lit else [False]):
        rm = scene.trace_rays(o[:400], d[:400], spp=4, max_depth=8, background=bg, light_sampling=nee, sumsq=True)
        rf = fresh.trace_rays(o[:400], d[:400], spp=4, max_depth=8, background=bg, light_sampling=nee, sumsq=True)
        assert rf.sum.std() > 0.0 and rm.sum.tobytes() == rf.sum.tobytes() and rm.sumsq.tobytes() == rf.sumsq.tobytes(), (name, nee)
    cam, cfg, h = cam_cfg(rtsr, case)
    if lit:
        _same_screen(scene.render(cam, cfg, light_sampling=True), fresh.render(cam, cfg, light_sampling=True), name + ": light sampling")
    pm, pf = scene.progressive(cam, cfg), fresh.progressive(cam, cfg)
    for p in (pm, pf):
        p.add(2)
        p.add(2)
    _same_screen(pm.screen(), pf.screen(), name + ": progressive")
    _same_screen(pm.screen(), fresh.render(cam, cfg), name + ": progressive against the one-shot render")
    (am, nm), (af, nf) = pm.features(4), pf.features(4)
    assert af.std() > 0.01 and np.array_equal(am, af) and np.array_equal(nm, nf)


def test_the_albedo_feature_follows_a_colour_edit(rtsr):
    case = build(rtsr, "cornell_light")
    flat = case.flatten()
    scene = _upload(flat)
    cam, cfg, h = cam_cfg(rtsr, case)
    before = scene.progressive(cam, cfg).features(4)[0]
    scene.set_shading(edits_for(case, flat, {"wall": (0.1, 0.2, 0.7)}))
    after = scene.progressive(cam, cfg).features(4)[0]
    assert (before != after).any()


# ---- 5. the light table
def test_the_light_table_on_the_device_is_the_hosts(rtsr):
    """k_refresh_lights against build_light_table on two_lamps' three edits (the uniform fallback among them) and on the noise
    lamp; and a texture edit that touches no light leaves `lights` byte-equal to before: the refresh is a recomputation by the
    function that built the table."""
    for name in ("two_lamps", "noise_lamp"):
        case = build(rtsr, name)
        for k, variant in enumerate(VARIANTS[name]):
            flat = case.flatten()
            scene = _upload(flat)
            t0 = scene.array("lights")
            assert len(t0) == 2 * LIGHT.itemsize and np.array_equal(t0, flat.array("lights"))
            edits = edits_for(case, flat, variant)
            scene.set_shading(edits)
            flat.set_shading(edits)
            t1 = scene.array("lights")
            assert np.array_equal(t1, flat.array("lights")), (name, k)
            assert not np.array_equal(t1.view(LIGHT)["pmf"], t0.view(LIGHT)["pmf"]), (name, k)
            if name == "two_lamps" and k == 1:
                assert list(t1.view(LIGHT)["pmf"]) == [0.5, 0.5]
    for name, variant in (("cornell_light", {"wall": (0.1, 0.2, 0.7)}), ("noise_lamp", {"marble": 0.4}), ("shared_texture", {"fog": (0.9, 0.1, 0.1)})):
        case = build(rtsr, name)
        flat = case.flatten()
        scene = _upload(flat)
        t0, tex0 = scene.array("lights"), scene.array("textures")
        assert len(t0) > 0
        scene.set_shading(edits_for(case, flat, variant))
        assert np.array_equal(scene.array("lights"), t0) and not np.array_equal(scene.array("textures"), tex0), name


# ---- 6. ordering on a stream
def test_two_edits_and_their_readers_on_a_side_stream(rtsr):
    """Two edits, a cast and a render enqueued on one side stream without a host wait: after waiting on that stream the frame
    is the second edit's."""
    import torch
    case = build(rtsr, "cornell_light")
    flat = case.flatten()
    scene = _upload(flat)
    fresh = _upload(build(rtsr, "cornell_light", 1).flatten())
    cam, cfg, h = cam_cfg(rtsr, case)
    o, d = _rays(500, 43)
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    d_acc = torch.zeros((h, cfg.image_width, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        scene.set_shading(edits_for(case, flat, VARIANTS["cornell_light"][0]), stream=side)
        scene.set_shading(edits_for(case, flat, dict(VARIANTS["cornell_light"][1], wall=(0.65, 0.05, 0.05))), stream=side)
        got = scene.cast_rays(to, td)  # behind both edits on the same stream
        scene.render_device(cam, cfg, d_accum=d_acc.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    want = fresh.render(cam, cfg)
    assert np.array_equal(d_acc.cpu().numpy(), want.accum)
    ref = fresh.cast_rays(o, d)
    assert ref.hit.sum() > 100 and np.array_equal(got.ids.cpu().numpy(), ref.ids)
    _assert_equal(_device(scene), _device(fresh), "after two edits on a side stream")


# ---- 7. with the other updates
def test_one_scene_through_every_kind_of_update(rtsr):
    """set_spheres (the lamp moves), set_shading (its colour and the fog's density), set_transforms (the fog moves), set_shading
    again: after every step lights, world_desc and one frame equal the host sequence uploaded fresh."""
    case = sequence(rtsr)
    flat = case.flatten()
    scene = _upload(flat)
    cam, cfg, h = cam_cfg(rtsr, case)
    lamp_id = flat.sphere_ids(case.builder, case.lamp)
    steps = [
        ("set_spheres", (lamp_id, [[3.6, 2.9, 3.4, 0.3]])),
        ("set_shading", (edits_for(case, flat, {"ball": (0.5, 9.0, 2.0), "d": 0.2}),)),
        ("set_transforms", ({case.fog_slot: [("translate", (3.1, 0.4, 1.6)), ("rotate_y", -40.0)]},)),
        ("set_shading", (edits_for(case, flat, {"ball": (0.0, 0.0, 0.0), "c": (0.2, 0.9, 0.3), "rect": (7.0, 1.0, 1.0)}),)),
    ]
    last = scene.render(cam, cfg)
    for k, (method, args) in enumerate(steps):
        getattr(scene, method)(*args)
        getattr(flat, method)(*args)
        fresh = _upload(flat)
        what = "step %d (%s)" % (k, method)
        _assert_equal(_device(scene), _device(fresh), what)
        now = scene.render(cam, cfg)
        _same_screen(now, fresh.render(cam, cfg), what)
        assert (now.accum != last.accum).any(), what
        last = now


# ---- 8. refusals
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_scene_refusals_enqueue_nothing(rtsr, f32):
    case = build(rtsr, "shared_texture")
    flat = case.flatten()
    scene = _upload(flat, f32=f32)
    cam, cfg, h = cam_cfg(rtsr, case)
    first, frame = _device(scene), scene.render(cam, cfg)
    for edits, n, words in refusals(rtsr, case, flat):
        assert call_set_shading(rtsr, rtsr.lib.rtx_scene_set_shading, scene.ptr, edits, n, None) == rtsr.RTX_EINVAL, words
        msg = rtsr.last_error()
        assert msg.startswith("rtx_scene_set_shading: ") and all(w in msg for w in words), (words, msg)
    with pytest.raises(ValueError):
        scene.set_shading([("metal", 0, (1, 2, 3))])
    _assert_equal(_device(scene), first, "after the refusals")
    _same_screen(scene.render(cam, cfg), frame, "after the refusals")
    scene.set_shading(edits_for(case, flat, VARIANTS["shared_texture"][0]))  # a good edit still goes through
    assert not np.array_equal(scene.array("materials"), first["materials"])
