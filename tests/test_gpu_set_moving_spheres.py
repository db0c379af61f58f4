"""Scene.set_moving_spheres on the device (rtx_scene_set_moving_spheres / _device: k_set_prims<7>, k_refit_timed_bvh with its
three-box climb, k_refit_wide, k_slot_boxes' mover slots, the slope mask and the plan of k_trace_lds that hangs on it).

Two judges, neither the code under test: the resident ARRAYS after an update are byte-equal to those of the host-updated flat
scene uploaded afresh (rtx_flat_set_moving_spheres, which tests/test_set_moving_spheres_host.py holds to a fresh flatten, to the
flattener's top-down rule and to the oracle), and every ENTRY POINT on the updated scene answers bit for bit as on a FRESH
upload of the same world built from scratch with the new values.  Frames are 48 x 27 at 4 spp."""
import ctypes as C

import numpy as np
import pytest

import cast_rays_cases as cc
from mover_update_cases import (CASES, DESC, DEVICE_KEPT, DEVICE_WRITTEN, FORCED_KERNELS, INTERVALS, LDS_CASES, MOTION32, MOVER, NAN_CASES, NODE, NODE32,
                                NO_TIME_BOXES, ONE_AXIS, SLOPE_CASES, TIME_BOXES, WD_TIME_BOX, book1_head, book1_update, cam_cfg, refusals,
                                same_numbers, update_of, with_gravity)
from update_cases import KERNEL_OF, call_set_prims, device_arrays, same_screen as _same_screen, updated_pair
from update_cases import upload as _upload

pytestmark = pytest.mark.gpu
NUMBERS = {"nodes": NODE, "nodes32": NODE32, "motion32": MOTION32, "moving_spheres": MOVER}


def _device(scene):
    return device_arrays(scene, DEVICE_WRITTEN + DEVICE_KEPT)


def _assert_arrays(scene, want, what, nan=False):
    """Byte for byte; nan: a case whose movers have no finite centre -- its NaNs carry no specified sign or payload across
    machines, so the arrays that hold boxes are compared as numbers, a NaN equal to a NaN (mover_update_cases.NAN_CASES)."""
    now = _device(scene)
    for k in want:
        if nan and k in NUMBERS:
            assert same_numbers(now[k], want[k], NUMBERS[k]), "%s: %s differs from the host-updated scene uploaded fresh" % (what, k)
        else:
            assert now[k].size == want[k].size and np.array_equal(now[k], want[k]), "%s: %s differs from the host-updated scene uploaded fresh in %d bytes" % (
                what, k, int((now[k] != want[k]).sum()) if now[k].size == want[k].size else -1)


# ---- 1. the arrays, through both entries
@pytest.mark.parametrize("name", sorted(CASES))
def test_updated_arrays_equal_the_host_updated_scene_uploaded_fresh(rtsr, name):
    """Host values; then the way back as a torch tensor on the current stream; then the update again as a tensor on a side
    stream.  After each the written arrays are those of the host-updated flat scene uploaded fresh, and every other served array
    keeps its bytes."""
    import torch
    nan = name in NAN_CASES
    case = CASES[name](rtsr, False)
    flat = case.flatten()
    scene = _upload(flat)
    first = _device(scene)
    _assert_arrays(scene, _device(_upload(flat)), "upload", nan)
    ids, vals = update_of(case, flat)
    scene.set_moving_spheres(ids, vals)
    flat.set_moving_spheres(ids, vals)
    assert not np.array_equal(scene.array("moving_spheres"), first["moving_spheres"])
    moved = _device(_upload(flat))
    _assert_arrays(scene, moved, "host values", nan)
    for k in DEVICE_KEPT + ("top_box32", "lights"):  # what no mover's value reaches
        assert np.array_equal(moved[k], first[k]), k
    back_ids, back = update_of(case, flat, moved=False)
    scene.set_moving_spheres(back_ids, torch.from_numpy(back).cuda())
    _assert_arrays(scene, first, "a tensor on the current stream, back to rest", nan)
    t_vals = torch.from_numpy(vals).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        scene.set_moving_spheres(ids, t_vals, stream=side)
    side.synchronize()
    _assert_arrays(scene, moved, "a tensor on a side stream", nan)
    scene.set_moving_spheres([], np.zeros((0, 7)))  # n = 0: nothing launched
    scene.set_moving_spheres([], torch.zeros((0, 7), dtype=torch.float64, device="cuda"))


def test_partial_and_reversed_id_lists(rtsr):
    case = CASES["y_only"](rtsr, False)
    flat = case.flatten()
    scene = _upload(flat)
    first = _device(scene)
    for what, kw in (("one of 40", {"only": 5}), ("every 7th", {"every": 7}), ("reversed", {"reverse": True})):
        ids, vals = update_of(case, flat, **kw)
        scene.set_moving_spheres(ids, vals)
        flat.set_moving_spheres(ids, vals)
        _assert_arrays(scene, _device(_upload(flat)), what)
        back = update_of(case, flat, moved=False, **kw)
        scene.set_moving_spheres(*back)
        flat.set_moving_spheres(*back)
        _assert_arrays(scene, first, what + ", back")


def test_the_time_box_of_a_plain_mover_clears_and_comes_back(rtsr):
    """A plain mover in the world list: the slot record's box, WD_TIME_BOX and its two times.  A value that makes a plane
    overflow f32 clears the flag; the way back sets it again."""
    case = CASES["plain_overflow"](rtsr, False)
    flat = case.flatten()
    scene = _upload(flat)
    desc = lambda: scene.array("world_desc").view(DESC)
    d0 = desc().copy()
    assert len(d0) == 3 and d0["flags"][1] & WD_TIME_BOX and d0["flags"][2] & WD_TIME_BOX and d0["aux"][1] == 1.0
    ids, vals = update_of(case, flat)
    scene.set_moving_spheres(ids, vals)
    flat.set_moving_spheres(ids, vals)
    d1 = desc()
    assert not d1["flags"][1] & WD_TIME_BOX and d1["flags"][2] & WD_TIME_BOX and not np.isfinite(d1["box"][1]).all()
    assert not np.array_equal(d1["box"][2], d0["box"][2])
    _assert_arrays(scene, _device(_upload(flat)), "overflow")
    back = update_of(case, flat, moved=False)
    scene.set_moving_spheres(*back)
    assert np.array_equal(desc().view(np.uint8), d0.view(np.uint8))


@pytest.mark.parametrize("name", ["tri_mover", "mixed5_leaf4"])
def test_wide_records_follow_the_refit(rtsr, name):
    env = {"RTX_WIDE": "1"}
    case = CASES[name](rtsr, False)
    flat = case.flatten()
    scene = _upload(flat, env)
    first = _device(scene)
    ids, vals = update_of(case, flat)
    scene.set_moving_spheres(ids, vals)
    flat.set_moving_spheres(ids, vals)
    _assert_arrays(scene, _device(_upload(flat, env)), name + " wide")
    if name == "tri_mover":
        assert scene.wide_levels() > 0 and len(first["nodes4"]) > 0 and not np.array_equal(scene.array("nodes4"), first["nodes4"])
    assert np.array_equal(_device(scene)["plans"], first["plans"])


# ---- 2. frames on the updated scene against a fresh upload
_PAIRS = {}


def _pair(rtsr, name, env=()):
    return updated_pair(_PAIRS, rtsr, CASES, update_of, "set_moving_spheres", name, env)


@pytest.mark.parametrize("name", sorted(CASES))
def test_renders_on_the_updated_scene_equal_the_fresh_upload(rtsr, orc, name):
    """rtx_render under RTX_TRACE_KERNEL unset, simple, vote, world and wavefront; stats.trace_kernel is what was asked wherever
    choose_trace_kernel accepts the world (FORCED_KERNELS) and k_trace_world where it does not; a world of one sphere BVH runs
    k_trace_lds by default, in the variant the fresh upload reports.  Then a progressive handle made after the update, with its
    features, and the CPU oracle's frame of the host-updated flat scene."""
    honoured = set()
    for kernel in (None, "simple", "vote", "world", "wavefront"):
        env = (("RTX_TRACE_KERNEL", kernel),) if kernel else ()
        scene, fresh, flat, fresh_flat, case = _pair(rtsr, name, env)
        cam, cfg, h = cam_cfg(rtsr, case)
        assert (cfg.image_width, h, cfg.samples_per_pixel) == (48, 27, 4)
        what = "%s %s" % (name, kernel)
        want = fresh.render(cam, cfg, want_stats=True)
        got = scene.render(cam, cfg, want_stats=True)
        assert want.accum.std() > 0.01 or name in NAN_CASES
        assert np.array_equal(got.accum, want.accum, equal_nan=True) and np.array_equal(got.rgb8, want.rgb8), what
        ran = rtsr.trace_kernel_name(got.stats.trace_kernel)
        assert ran == rtsr.trace_kernel_name(want.stats.trace_kernel), what
        assert got.stats.trace_variant == want.stats.trace_variant, what
        if kernel is not None:
            assert ran == (KERNEL_OF[kernel] if kernel in FORCED_KERNELS[name] else "k_trace_world"), what
            if ran == KERNEL_OF[kernel]:
                honoured.add(kernel)
            continue
        if name in LDS_CASES:
            assert ran == "k_trace_lds", what
        if name in NAN_CASES:
            continue
        pm, pf = scene.progressive(cam, cfg), fresh.progressive(cam, cfg)
        for p in (pm, pf):
            p.add(2)
            p.add(2)
        _same_screen(pm.screen(), pf.screen(), what + ": progressive")
        _same_screen(pm.screen(), want, what + ": progressive against the one-shot render")
        (am, nm), (af, nf) = pm.features(4), pf.features(4)
        assert af.std() > 0.01 and np.array_equal(am, af) and np.array_equal(nm, nf)
        o2, o2_8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=4)
        assert np.array_equal(got.accum, o2) and np.array_equal(got.rgb8, o2_8)
    assert honoured == set(FORCED_KERNELS[name]), (name, sorted(honoured))


# ---- 3. the variant k_trace_lds is launched in follows the slopes
def _variant(scene, cam, cfg):
    s = scene.render(cam, cfg, want_stats=True)
    return s, s.stats.trace_variant & (TIME_BOXES | ONE_AXIS)


@pytest.mark.parametrize("wide", ["0", "1"])
@pytest.mark.parametrize("name", SLOPE_CASES)
def test_the_lds_variant_follows_the_slopes(rtsr, name, wide):
    """y_only keeps TIME_BOXES | ONE_AXIS; y_to_xy loses ONE_AXIS (the y-only instantiation would cull the drifting mover by
    boxes that no longer hold it); xy_to_y gets it back; still and z_only report what the fresh scene reports.  The variant is
    asked BEFORE the update too, so that the plan the update has to change is a plan that was used."""
    want_bits = {"y_only": (TIME_BOXES | ONE_AXIS, TIME_BOXES | ONE_AXIS), "y_to_xy": (TIME_BOXES | ONE_AXIS, TIME_BOXES),
                 "xy_to_y": (TIME_BOXES, TIME_BOXES | ONE_AXIS), "still": (TIME_BOXES | ONE_AXIS, TIME_BOXES), "z_only": (TIME_BOXES | ONE_AXIS, TIME_BOXES)}[name]
    env = {"RTX_WIDE": wide}
    case, moved = CASES[name](rtsr, False), CASES[name](rtsr, True)
    flat = case.flatten()
    scene, fresh = _upload(flat, env), _upload(moved.flatten(), env)
    cam, cfg, h = cam_cfg(rtsr, case)
    before, bits0 = _variant(scene, cam, cfg)
    assert rtsr.trace_kernel_name(before.stats.trace_kernel) == "k_trace_lds" and bits0 == want_bits[0]
    ids, vals = update_of(case, flat)
    scene.set_moving_spheres(ids, vals)
    got, bits = _variant(scene, cam, cfg)
    want, fresh_bits = _variant(fresh, cam, cfg)
    assert got.stats.trace_variant == want.stats.trace_variant and bits == fresh_bits == want_bits[1], (name, bits, fresh_bits)
    _same_screen(got, want, name)
    # a shutter outside the BVH's interval: no TIME_BOXES, before or after
    cam_out = rtsr.Camera.new(case.look[0], case.look[1], (0.0, 1.0, 0.0), 35.0, 16.0 / 9.0, 0.0, 10.0, 0.5, 1.5)
    out, out_bits = _variant(scene, cam_out, cfg)
    assert out_bits == 0 and out.stats.trace_variant == fresh.render(cam_out, cfg, want_stats=True).stats.trace_variant
    _same_screen(out, fresh.render(cam_out, cfg), name + ", shutter outside")
    # and back: the plan returns with the slopes
    scene.set_moving_spheres(*update_of(case, flat, moved=False))
    again, bits2 = _variant(scene, cam, cfg)
    assert bits2 == want_bits[0]
    _same_screen(again, before, name + ", back at rest")


@pytest.mark.parametrize("which", sorted(INTERVALS))
def test_the_lds_variant_on_every_interval(rtsr, which):
    name = "interval_" + which
    scene, fresh, flat, fresh_flat, case = _pair(rtsr, name)
    cam, cfg, h = cam_cfg(rtsr, case)
    got, want = scene.render(cam, cfg, want_stats=True), fresh.render(cam, cfg, want_stats=True)
    assert got.stats.trace_variant == want.stats.trace_variant
    assert bool(got.stats.trace_variant & TIME_BOXES) == (which not in NO_TIME_BOXES), which


# ---- 4. queries
@pytest.mark.parametrize("name", ["pair", "mixed5_leaf4", "y_to_xy", "interval_mixed", "plain", "radii"])
def test_rays_from_every_movers_centre_equal_the_cpu_core(rtsr, orc, name):
    """cast_rays from the centre of every mover at three ray times, along +y: what core_world_hit answers on the host-updated
    flat scene, bit for bit."""
    scene, fresh, flat, fresh_flat, case = _pair(rtsr, name)
    mov = flat.array("moving_spheres").view(MOVER)
    t_lo, t_hi = case.shutter
    o, d, times = [], [], []
    for t in (t_lo, t_lo + 0.3125 * (t_hi - t_lo), t_hi):
        for m in mov:
            if m["time0"] == m["time1"]:
                continue
            o.append(m["c0"] + (t - m["time0"]) / (m["time1"] - m["time0"]) * (m["c1"] - m["c0"]))
            d.append((0.0, 1.0, 0.0))
            times.append(t)
    o, d, times = np.ascontiguousarray(o), np.ascontiguousarray(d, dtype=np.float64), np.ascontiguousarray(times)
    hits = scene.cast_rays(o, d, times, seed=1, stream_step=1)
    want = fresh.cast_rays(o, d, times, seed=1, stream_step=1)
    n_hit = 0
    for r in range(len(o)):
        rec = orc.core_world_hit(flat.arrays_ptr(), tuple(o[r]), tuple(d[r]), float(times[r]), 0.001, float("inf"), rng_seed=1 + r)
        assert bool(hits.hit[r]) == (rec is not None), r
        if rec is None:
            continue
        n_hit += 1
        assert cc.same_bits(np.array([[hits.t[r], *hits.p[r], *hits.normal[r]]]), np.array([[rec["t"], *rec["p"], *rec["normal"]]])).all(), r
    assert n_hit >= len(o) // 2
    for col in ("t", "p", "normal", "uv", "ids"):
        assert cc.same_bits(getattr(hits, col).reshape(len(o), -1).astype(np.float64), getattr(want, col).reshape(len(o), -1).astype(np.float64)).all(), col


def test_trace_rays_light_sampling_and_a_progressive_handle(rtsr):
    """A rectangle light over plain movers: trace_rays at max_depth 1 and deeper, render(light_sampling=1) and a progressive
    handle with light sampling made after the update equal the fresh upload's."""
    def lit(rtsr, moved):
        case = CASES["plain"](rtsr, moved)
        b = case.builder
        case.world = b.hittable_list([case.world, b.xz_rect(1.5, 4.5, 1.5, 4.5, 3.4, b.diffuse_light((4.0, 4.0, 4.0)))])
        return case

    case, moved = lit(rtsr, False), lit(rtsr, True)
    flat = case.flatten()
    scene, fresh = _upload(flat), _upload(moved.flatten())
    ids, vals = update_of(case, flat)
    scene.set_moving_spheres(ids, vals)
    cam, cfg, h = cam_cfg(rtsr, case)
    want = fresh.render(cam, cfg, light_sampling=True)
    assert want.accum.std() > 0.01
    _same_screen(scene.render(cam, cfg, light_sampling=True), want, "light sampling")
    pm, pf = scene.progressive(cam, cfg, light_sampling=True), fresh.progressive(cam, cfg, light_sampling=True)
    for p in (pm, pf):
        p.add(4)
    _same_screen(pm.screen(), pf.screen(), "progressive with light sampling")
    rng = np.random.default_rng(5)
    o = np.array([3.0, 3.0, 9.0]) + rng.uniform(-0.5, 0.5, (500, 3))
    d = np.array([3.0, 1.0, 3.0]) + rng.uniform(-2.5, 2.5, (500, 3)) - o
    times = rng.uniform(0.0, 1.0, 500)
    for depth, ls in ((1, False), (8, False), (8, True)):
        rm = scene.trace_rays(o, d, times, spp=4, max_depth=depth, background=(0.05, 0.05, 0.08), sumsq=True, light_sampling=ls)
        rf = fresh.trace_rays(o, d, times, spp=4, max_depth=depth, background=(0.05, 0.05, 0.08), sumsq=True, light_sampling=ls)
        assert cc.same_bits(rm.sum, rf.sum).all() and cc.same_bits(rm.sumsq, rf.sumsq).all(), (depth, ls)
        assert depth == 1 or rf.sum.std() > 0.001


# ---- 5. one scene through several updates, nothing waited for in between
def test_a_sequence_of_updates_without_a_wait(rtsr):
    """ONE scene: set_moving_spheres, set_shading, set_moving_spheres, render -- the caller never synchronises.  The frame is
    that of the flat scene taken through the same steps on the host and uploaded fresh."""
    case = CASES["y_to_xy"](rtsr, False)
    flat = case.flatten()
    scene = _upload(flat)
    ids, vals = update_of(case, flat)
    half = 0.5 * (vals + update_of(case, flat, moved=False)[1])
    edits = [("metal", 1, (0.9, 0.5, 0.2), 0.05)]
    cam, cfg, h = cam_cfg(rtsr, case)
    scene.set_moving_spheres(ids, half)
    scene.set_shading(edits)
    scene.set_moving_spheres(ids, vals)
    got = scene.render(cam, cfg, want_stats=True)
    flat.set_moving_spheres(ids, half)
    flat.set_shading(edits)
    flat.set_moving_spheres(ids, vals)
    fresh = _upload(flat)
    want = fresh.render(cam, cfg, want_stats=True)
    assert got.stats.trace_variant == want.stats.trace_variant and not got.stats.trace_variant & ONE_AXIS
    _same_screen(got, want, "sequence")
    _assert_arrays(scene, _device(fresh), "sequence")


def test_the_device_entry_and_a_device_render_on_one_stream(rtsr):
    """rtx_scene_set_moving_spheres_device followed directly by rtx_render_device on the same stream: the frame of the fresh
    upload (the launcher's one wait for the slope mask is the only host wait in between)."""
    import torch
    case, moved = CASES["y_to_xy"](rtsr, False), CASES["y_to_xy"](rtsr, True)
    flat = case.flatten()
    scene, fresh = _upload(flat), _upload(moved.flatten())
    cam, cfg, h = cam_cfg(rtsr, case)
    scene.render(cam, cfg)  # the y-only plan has been used
    ids, vals = update_of(case, flat)
    t_vals = torch.from_numpy(vals).cuda()
    accum = torch.zeros((h, cfg.image_width, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        scene.set_moving_spheres(ids, t_vals, stream=side)
        scene.render_device(cam, cfg, d_accum=accum.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    want = fresh.render(cam, cfg)
    assert np.array_equal(accum.cpu().numpy(), want.accum)


def test_book1_at_head_refits_on_the_device(rtsr, orc):
    """Catalogue scene 13 through k_trace_lds: every mover hops, along y (the y-only variant stays) and then along x and y (it
    goes); arrays and frame against the host-updated flat scene uploaded fresh and against the CPU oracle; then back."""
    b, world, cam, bg = book1_head(rtsr)
    flat = b.flatten(world)
    scene = _upload(flat)
    first = _device(scene)
    cfg = rtsr.Config.new(16.0 / 9.0, 48, 4, 8, 4, seed=31, background=bg)
    h = rtsr.image_height(cfg)
    assert _variant(scene, cam, cfg)[1] == TIME_BOXES | ONE_AXIS
    ids, rest, _ = book1_update(flat, b, world)
    for axes, bits in (("y", TIME_BOXES | ONE_AXIS), ("xy", TIME_BOXES)):
        mv = book1_update(flat, b, world, axes=axes)[2]
        scene.set_moving_spheres(ids, mv)
        flat.set_moving_spheres(ids, mv)
        fresh = _upload(flat)
        _assert_arrays(scene, _device(fresh), "book1 " + axes)
        got, got_bits = _variant(scene, cam, cfg)
        want, want_bits = _variant(fresh, cam, cfg)
        assert rtsr.trace_kernel_name(got.stats.trace_kernel) == "k_trace_lds" and got_bits == want_bits == bits
        _same_screen(got, want, "book1 " + axes)
        o2, o2_8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=4)
        assert np.array_equal(got.accum, o2) and np.array_equal(got.rgb8, o2_8)
        scene.set_moving_spheres(ids, rest)
        flat.set_moving_spheres(ids, rest)
    _assert_arrays(scene, first, "book1 back at rest")
    assert _variant(scene, cam, cfg)[1] == TIME_BOXES | ONE_AXIS


# ---- 6. refusals
def test_scene_refusals_enqueue_nothing(rtsr):
    import torch
    case = with_gravity(rtsr, False)
    flat = case.flatten()
    scene = _upload(flat)
    cam, cfg, h = cam_cfg(rtsr, case)
    first, frame = _device(scene), scene.render(cam, cfg)
    n_ids = flat.info()["n_moving_spheres"]
    for name, ids, n, vals, word, host_only in refusals(n_ids):  # in ladder order
        st = call_set_prims(rtsr, rtsr.lib.rtx_scene_set_moving_spheres, scene.ptr, ids, n, vals, None)
        assert st == rtsr.RTX_EINVAL and "rtx_scene_set_moving_spheres" in rtsr.last_error() and word in rtsr.last_error(), (name, rtsr.last_error())
    good = torch.ones(14, dtype=torch.float64).cuda()
    two = (C.c_int32 * 2)(0, 1)
    dev = rtsr.lib.rtx_scene_set_moving_spheres_device
    assert dev(scene.ptr, two, 2, C.c_void_p(good.data_ptr() + 4), None) == rtsr.RTX_EINVAL and "d_movers is not 8-byte aligned" in rtsr.last_error()
    assert dev(scene.ptr, (C.c_int32 * 2)(0, n_ids), 2, C.c_void_p(good.data_ptr()), None) == rtsr.RTX_EINVAL and "out of range" in rtsr.last_error()
    assert dev(scene.ptr, (C.c_int32 * 2)(1, 1), 2, C.c_void_p(good.data_ptr()), None) == rtsr.RTX_EINVAL and "twice" in rtsr.last_error()
    assert dev(scene.ptr, two, 2, None, None) == rtsr.RTX_EINVAL and "NULL" in rtsr.last_error()
    assert dev(scene.ptr, two, 0, C.c_void_p(good.data_ptr()), None) == rtsr.RTX_OK
    # a mover inside a BVH that also holds a GravitySphere: alone and among good ids, through both entries
    bad = flat.moving_sphere_ids(case.builder, case.handles["bad"])
    ids, vals = update_of(case, flat)
    for i, v in ((bad, vals[-1:]), (ids, vals)):
        for values in (v, torch.from_numpy(np.ascontiguousarray(v)).cuda()):
            with pytest.raises(rtsr.RtxError) as e:
                scene.set_moving_spheres(i, values)
            assert e.value.status == rtsr.RTX_EUNSUPPORTED and "GravitySphere" in str(e.value) and "not linear in time" in str(e.value)
    back = _device(scene)
    assert all(np.array_equal(back[k], first[k]) for k in first)
    _same_screen(scene.render(cam, cfg), frame, "after the refusals")
    # the BVH of movers alone beside it still updates
    n_clean = case.handles["n_clean"]
    scene.set_moving_spheres(ids[:n_clean], vals[:n_clean])
    flat.set_moving_spheres(ids[:n_clean], vals[:n_clean])
    _assert_arrays(scene, _device(_upload(flat)), "the BVH beside the refused one")
    # an f32 scene: refused before the ids are looked at, the scene as it was
    plain = CASES["pair"](rtsr, False)
    pflat = plain.flatten()
    s32 = pflat.upload(f32=True)
    cam, cfg, h = cam_cfg(rtsr, plain)
    f32_first = s32.render(cam, cfg)
    with pytest.raises(rtsr.RtxError) as e:
        s32.set_moving_spheres(*update_of(plain, pflat))
    assert e.value.status == rtsr.RTX_EUNSUPPORTED and "rtx_flat_set_moving_spheres" in str(e.value) and "rtx_scene_upload_f32" in str(e.value)
    nan = update_of(plain, pflat)[1].copy()
    nan[0, 0] = float("nan")
    with pytest.raises(rtsr.RtxError) as e:  # a value that is not finite is RTX_EINVAL before the f32 scene is RTX_EUNSUPPORTED
        s32.set_moving_spheres(update_of(plain, pflat)[0], nan)
    assert e.value.status == rtsr.RTX_EINVAL and "not finite" in str(e.value)
    _same_screen(s32.render(cam, cfg), f32_first, "f32 after the refusal")
    # set_spheres keeps refusing a BVH that holds a mover, on the device too
    mixed = CASES["mixed5_leaf1"](rtsr, False)
    mscene = _upload(mixed.flatten())
    with pytest.raises(rtsr.RtxError) as e:
        mscene.set_spheres([1], [[1.3, 0.9, 2.1, 0.2]])
    assert e.value.status == rtsr.RTX_EUNSUPPORTED and "MovingSphere" in str(e.value)
