"""Scene.set_transforms on the device (rtx_scene_set_transforms: k_set_slot_ops, k_refit_instance_tree).

Two judges, neither the code under test: the resident ARRAYS after an update are byte-equal to the host refit of the same flat
scene (rtx_flat_set_transforms, which tests/test_set_transforms_host.py holds to a fresh flatten), and every ENTRY POINT on
the moved scene answers bit for bit as on a FRESH upload of the same world built with the new offsets and angles."""
import os

import numpy as np
import pytest

import cast_rays_cases as cc
from instance_scenes import box_field, member_zoo, zoo_cam_cfg
from set_transforms_cases import (build, calls_of_slots, chain_slots, prism_field, random_values, room, room_cam_cfg, two_trees, updates_for,
                                  values_of)

pytestmark = pytest.mark.gpu
DEVICE_ARRAYS = ("entries", "nodes", "nodes32", "motion32", "world_desc")


def _device(scene):
    return {k: scene.array(k) for k in DEVICE_ARRAYS}


def _assert_arrays_equal_host(scene, flat, what):
    for k in ("entries", "nodes", "nodes32", "motion32"):
        dev, host = scene.array(k), flat.array(k)
        assert dev.size == host.size and np.array_equal(dev, host), "%s: %s differs from the host refit in %d bytes" % (what, k, int((dev != host).sum()))


# ---- 1. the refitted arrays
@pytest.mark.parametrize("n,line", [(2, False), (3, False), (64, False), (65, False), (257, False), (1024, False), (40, True)])
def test_refitted_arrays_equal_the_host_refit(rtsr, n, line):
    """Root only, one internal child, a wave and a block boundary on either side, a deep tree, a skewed tree: after an update
    of every member the resident entries, nodes and nodes32 are the host refit's, byte for byte."""
    b, w, calls = build(rtsr, lambda r: prism_field(r, n, line))
    flat = b.flatten(w)
    tree = flat.instance_tree(0)
    assert tree["n_slots"] == n and tree["n_nodes"] == n - 1
    if line:
        assert tree["depth"] >= 9  # skewed: a balanced tree of 40 leaves has 6 levels
    scene = flat.upload()
    _assert_arrays_equal_host(scene, flat, "upload")
    first = _device(scene)
    upd = updates_for(flat, calls, random_values(calls, seed=n))
    scene.set_transforms(upd)
    flat.set_transforms(upd)
    assert not np.array_equal(flat.array("nodes"), first["nodes"])
    _assert_arrays_equal_host(scene, flat, "n = %d" % n)
    home = updates_for(flat, calls, values_of(calls))
    scene.set_transforms(home)
    back = _device(scene)
    assert all(np.array_equal(back[k], first[k]) for k in DEVICE_ARRAYS)


def test_update_patterns(rtsr):
    """One member; every 7th member; two updates in a row with nothing between them; the original pose again, which must give
    the arrays of the first upload."""
    b, w, calls = build(rtsr, lambda r: prism_field(r, 65))
    flat = b.flatten(w)
    scene = flat.upload()
    first = _device(scene)
    slots = chain_slots(flat)
    for only in ({slots[40]}, set(slots[::7])):
        values = random_values(calls, seed=len(only), only_calls=calls_of_slots(flat, calls, only))
        upd = updates_for(flat, calls, values, only=only)
        scene.set_transforms(upd)
        flat.set_transforms(upd)
        _assert_arrays_equal_host(scene, flat, "%d members" % len(only))
    v1, v2 = random_values(calls, seed=71), random_values(calls, seed=72)
    scene.set_transforms(updates_for(flat, calls, v1))
    scene.set_transforms(updates_for(flat, calls, v2, only=set(slots[1::2])))
    flat.set_transforms(updates_for(flat, calls, v1))
    flat.set_transforms(updates_for(flat, calls, v2, only=set(slots[1::2])))
    _assert_arrays_equal_host(scene, flat, "two updates in a row")
    scene.set_transforms({})
    scene.set_transforms(updates_for(flat, calls, values_of(calls)))
    back = _device(scene)
    for k in DEVICE_ARRAYS:
        assert np.array_equal(back[k], first[k]), k


# ---- 2. every entry point on the moved scene against a fresh upload
SCENES = {
    "zoo_middle": (lambda r: member_zoo(r, "instanced", "middle"), zoo_cam_cfg, (-8.0, -0.5, -6.5), (8.0, 6.0, 5.5)),
    "box_field": (lambda r: box_field(r, "instanced", n=60, lamp_member=True), zoo_cam_cfg, (-7.0, -0.5, -5.5), (7.0, 6.0, 5.5)),
    "room": (room, room_cam_cfg, (-50.0, -50.0, -50.0), (605.0, 605.0, 605.0)),
}
SIZES = ((48, 8), (120, 4))
_PAIRS = {}


def _pair(rtsr, name, f32=False, env=None):
    """(moved scene, fresh scene, fresh flat): the scene uploaded at its original pose and moved on the device, and the same
    world built with the new values, flattened and uploaded.  Built once per (scene, precision, environment)."""
    key = (name, f32, env)
    if key not in _PAIRS:
        old = os.environ.get("RTX_TRACE_KERNEL")
        if env:
            os.environ["RTX_TRACE_KERNEL"] = env  # read once per upload
        try:
            fn = SCENES[name][0]
            b, w, calls = build(rtsr, fn)
            flat = b.flatten(w)
            values = random_values(calls, seed=19, shift=30.0 if name == "room" else 0.4)
            bf, wf, _ = build(rtsr, fn, values)
            fresh_flat = bf.flatten(wf)
            moved = flat.upload(f32=f32)
            moved.set_transforms(updates_for(flat, calls, values))
            _PAIRS[key] = (moved, fresh_flat.upload(f32=f32), fresh_flat)
        finally:
            if env:
                if old is None:
                    del os.environ["RTX_TRACE_KERNEL"]
                else:
                    os.environ["RTX_TRACE_KERNEL"] = old
    return _PAIRS[key]


def _same_screen(a, b, what):
    bad = int((a.accum != b.accum).any(axis=2).sum())
    assert bad == 0 and np.array_equal(a.rgb8, b.rgb8), "%s: %d pixels differ from the fresh upload" % (what, bad)


@pytest.mark.parametrize("name", ["zoo_middle", "box_field", "room"])
def test_renders_on_the_moved_scene_equal_the_fresh_upload(rtsr, orc, name):
    """rtx_render with the default kernel and with RTX_TRACE_KERNEL=world, rtx_render_ex with light sampling, a progressive
    handle made after the update and its feature pass -- at 48 x 32 x 8 spp and 120 x 80 x 4 spp.  The zoo's frame is also
    O2's of the fresh flat scene."""
    moved, fresh, fresh_flat = _pair(rtsr, name)
    moved_w, fresh_w, _ = _pair(rtsr, name, env="world")
    for width, spp in SIZES:
        cam, cfg, h = SCENES[name][1](rtsr, width=width, spp=spp)
        assert (cfg.image_width, h, cfg.samples_per_pixel) == (width, width * 2 // 3, spp)
        want = fresh.render(cam, cfg)
        assert want.accum.std() > 0.01
        got = moved.render(cam, cfg)
        _same_screen(got, want, "%s %d: rtx_render" % (name, width))
        got_w = moved_w.render(cam, cfg, want_stats=True)
        assert rtsr.trace_kernel_name(got_w.stats.trace_kernel) == "k_trace_world"
        _same_screen(got_w, fresh_w.render(cam, cfg), "%s %d: k_trace_world" % (name, width))
        _same_screen(got_w, want, "%s %d: k_trace_world against the default kernel" % (name, width))
        _same_screen(moved.render(cam, cfg, light_sampling=True), fresh.render(cam, cfg, light_sampling=True), "%s %d: light sampling" % (name, width))
        pm, pf = moved.progressive(cam, cfg), fresh.progressive(cam, cfg)
        for p in (pm, pf):
            p.add(spp // 2)
            p.add(spp - spp // 2)
        _same_screen(pm.screen(), pf.screen(), "%s %d: progressive" % (name, width))
        _same_screen(pm.screen(), want, "%s %d: progressive against the one-shot render" % (name, width))
        (am, nm), (af, nf) = pm.features(4), pf.features(4)
        assert af.std() > 0.01 and np.array_equal(am, af) and np.array_equal(nm, nf)
        if name == "zoo_middle" and width == 48:
            o2, o2_8 = orc.o2_render(fresh_flat.arrays_ptr(), cam, cfg, h, threads=4)
            assert np.array_equal(got.accum, o2) and np.array_equal(got.rgb8, o2_8)


@pytest.mark.parametrize("name", ["zoo_middle", "box_field", "room"])
def test_ray_queries_on_the_moved_scene_equal_the_fresh_upload(rtsr, orc, name):
    """cast_rays with 2000 rays and every column, trace_rays at spp = 4.  The mix of hits and misses is counted on the CPU
    core's answers for the fresh flat scene alone."""
    moved, fresh, fresh_flat = _pair(rtsr, name)
    lo, hi = SCENES[name][2], SCENES[name][3]
    o, d = cc.sphere_rays(2000, 7, lo, hi, 0.45 if name == "room" else 1.0)
    ref = np.zeros((len(o), 11))
    for r in range(len(o)):
        rec = orc.core_world_hit(fresh_flat.arrays_ptr(), tuple(o[r]), tuple(d[r]), 0.0, cc.T_MIN, float("inf"), rng_seed=1 + r)
        if rec is not None:
            ref[r] = [1.0, rec["t"], *rec["p"], *rec["normal"], rec["u"], rec["v"], float(rec["front_face"])]
    if name != "room":  # a closed room is hit by every ray from inside it: the mix rule is for the open scenes
        cc.check_mix(name, ref)
    hm, hf = moved.cast_rays(o, d, seed=1, stream_step=1), fresh.cast_rays(o, d, seed=1, stream_step=1)
    for col in ("t", "p", "normal", "uv", "ids"):
        assert cc.same_bits(getattr(hm, col).reshape(len(o), -1).astype(np.float64), getattr(hf, col).reshape(len(o), -1).astype(np.float64)).all(), col
    assert cc.same_bits(cc.hits_as_records(hm), ref).all()
    rm = moved.trace_rays(o, d, spp=4, max_depth=12, background=(0.35, 0.4, 0.55), sumsq=True)
    rf = fresh.trace_rays(o, d, spp=4, max_depth=12, background=(0.35, 0.4, 0.55), sumsq=True)
    assert rf.sum.std() > 0.01 and cc.same_bits(rm.sum, rf.sum).all() and cc.same_bits(rm.sumsq, rf.sumsq).all()


@pytest.mark.parametrize("name", ["zoo_middle", "box_field"])
def test_f32_scene_moved_equals_fresh_f32_upload(rtsr, name):
    """The f32 compilation runs the same kernels on both sides, so this is exact: resident arrays, a render, a cast."""
    moved, fresh, _ = _pair(rtsr, name, f32=True)
    assert moved.is_f32 and fresh.is_f32
    for k in DEVICE_ARRAYS:
        a, b = moved.array(k), fresh.array(k)
        if k in ("nodes", "nodes32", "motion32"):
            continue  # the fresh tree has its own topology; its boxes are judged through the frames below
        assert np.array_equal(a, b), k
    cam, cfg, h = SCENES[name][1](rtsr, width=48, spp=8)
    _same_screen(moved.render(cam, cfg), fresh.render(cam, cfg), "%s f32" % name)
    o, d = cc.sphere_rays(2000, 7, SCENES[name][2], SCENES[name][3], 1.0)
    hm, hf = moved.cast_rays(o, d), fresh.cast_rays(o, d)
    assert hf.hit.sum() >= 500 and (~hf.hit).sum() >= 200
    for col in ("t", "p", "normal", "uv", "ids"):
        assert cc.same_bits(getattr(hm, col).reshape(len(o), -1).astype(np.float64), getattr(hf, col).reshape(len(o), -1).astype(np.float64)).all(), col


def test_f32_refit_arrays_are_the_narrowed_host_refit(rtsr, orc):
    """An f32 scene's nodes are the f64 refit narrowed down / up and its entries the (float) cast: the resident arrays after an
    update equal the product's converter run on the host refit (oracle f32_convert)."""
    b, w, calls = build(rtsr, lambda r: prism_field(r, 65))
    flat = b.flatten(w)
    scene = flat.upload(f32=True)
    upd = updates_for(flat, calls, random_values(calls, seed=5))
    scene.set_transforms(upd)
    flat.set_transforms(upd)
    descs = dict(orc.f32_descs())
    for name, elem64 in (("entries", 160), ("nodes", 112)):
        want, e32 = orc.f32_convert(descs[name], flat.array(name), elem64)
        assert want is not None and np.array_equal(scene.array(name), want), name
    assert np.array_equal(scene.array("nodes32"), flat.array("nodes32"))


# ---- 3. two trees beside a BvhNode of moving spheres
def test_two_trees_with_time_aware_boxes(rtsr):
    """motion32 is present: the trees' nodes carry their static boxes there, slopes 0.  One tree is updated, then both."""
    b, w, calls = build(rtsr, two_trees)
    flat = b.flatten(w)
    assert flat.instances()["n_trees"] == 2 and flat.array("motion32").size == flat.info()["n_nodes"] * 96
    scene = flat.upload()
    t0, t1 = flat.instance_tree(0), flat.instance_tree(1)
    in_tree = lambda t: {s for s in chain_slots(flat) if t["first_slot"] <= s < t["first_slot"] + t["n_slots"]}
    values = values_of(calls)
    for only, seed in ((in_tree(t1), 1), (in_tree(t0) | in_tree(t1), 2)):
        values = [new if k in calls_of_slots(flat, calls, only) else old for k, (old, new) in enumerate(zip(values, random_values(calls, seed=seed)))]
        upd = updates_for(flat, calls, values, only=only)
        scene.set_transforms(upd)
        flat.set_transforms(upd)
        _assert_arrays_equal_host(scene, flat, "%d slots" % len(only))
        bf, wf, _ = build(rtsr, two_trees, values)
        fresh = bf.flatten(wf).upload()
        cam = rtsr.Camera.new((0.5, 3.0, 9.0), (0.0, 0.6, 0.0), (0.0, 1.0, 0.0), 42.0, 1.5, 0.0, 9.0, 0.0, 1.0)
        cfg = rtsr.Config.new(1.5, 48, 8, 12, 4, seed=3, background=(0.6, 0.7, 0.9))
        _same_screen(scene.render(cam, cfg), fresh.render(cam, cfg), "two trees, %d slots moved" % len(only))


# ---- 4. streams
def test_update_and_cast_on_one_side_stream_without_a_host_wait(rtsr):
    import torch
    b, w, calls = build(rtsr, lambda r: prism_field(r, 257))
    flat = b.flatten(w)
    values = random_values(calls, seed=8)
    bf, wf, _ = build(rtsr, lambda r: prism_field(r, 257), values)
    fresh = bf.flatten(wf).upload()
    scene = flat.upload()
    o, d = cc.sphere_rays(2000, 3, (-9.0, -0.5, -9.0), (9.0, 6.0, 9.0), 1.0)  # fitted on the CPU core: 1680 hits, 320 misses on the fresh scene
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        scene.set_transforms(updates_for(flat, calls, values), stream=side)
        got = scene.cast_rays(to, td)  # enqueued behind the update on the same stream: no host synchronisation between them
    side.synchronize()
    want = fresh.cast_rays(o, d)
    assert want.hit.sum() >= 500 and (~want.hit).sum() >= 200
    assert cc.same_bits(got.t.cpu().numpy().reshape(-1, 1), want.t.reshape(-1, 1)).all()
    assert np.array_equal(got.ids.cpu().numpy(), want.ids) and cc.same_bits(got.p.cpu().numpy(), want.p).all()


# ---- 5. the probe
def test_a_probe_ray_loses_the_member_that_moved_away(rtsr):
    b, w, calls = build(rtsr, lambda r: prism_field(r, 9))
    flat = b.flatten(w)
    scene = flat.upload()
    slot = chain_slots(flat)[4]  # the middle box of the 3 x 3 field
    k_t = [k for k in calls_of_slots(flat, calls, {slot}) if calls[k][0] == "translate"][0]
    x, _, z = calls[k_t][1]
    o, d = np.array([[x, 5.0, z]]), np.array([[0.0, -1.0, 0.0]])
    before = scene.cast_rays(o, d)
    assert before.ids[0, 0] == 1 and before.ids[0, 2] == slot and 4.0 < before.t[0] < 5.0
    values = values_of(calls)
    values[k_t] = (x + 40.0, 0.0, z - 25.0)
    scene.set_transforms(updates_for(flat, calls, values, only={slot}))
    bf, wf, _ = build(rtsr, lambda r: prism_field(r, 9), values)
    fresh = bf.flatten(wf).upload()
    after, want = scene.cast_rays(o, d), fresh.cast_rays(o, d)
    # the ground now: a sphere of radius 500 whose top is y = 0, so a little below that away from the axis
    assert after.ids[0, 2] == want.ids[0, 2] == 0 and after.t[0] == want.t[0] and 5.0 <= after.t[0] < 5.01
    there = np.array([[x + 40.0, 5.0, z - 25.0]])
    a2, w2 = scene.cast_rays(there, d), fresh.cast_rays(there, d)
    assert a2.ids[0, 2] == w2.ids[0, 2] == slot and a2.t[0] == w2.t[0] == before.t[0]


def test_scene_refusals_enqueue_nothing(rtsr):
    b, w, calls = build(rtsr, lambda r: prism_field(r, 9))
    flat = b.flatten(w)
    scene = flat.upload()
    first = _device(scene)
    u = (rtsr.RtxSlotOps * 1)()
    for slot, n_ops, kinds, v, word in ((99, 2, (0, 1), 0.0, ".slot"), (0, 2, (0, 1), 0.0, "chain"), (3, 1, (0, 1), 0.0, ".n_ops"),
                                        (3, 2, (1, 0), 0.0, ".op"), (3, 2, (0, 1), 1.7976931348623157e308, "bounding box")):
        u[0].slot, u[0].n_ops = slot, n_ops
        for k in range(2):
            u[0].ops[k].op = kinds[k]
            u[0].ops[k].v[0] = v if kinds[k] == 0 else 10.0
        assert rtsr.lib.rtx_scene_set_transforms(scene.ptr, u, 1, None) == rtsr.RTX_EINVAL
        assert word in rtsr.last_error(), rtsr.last_error()
    back = _device(scene)
    assert all(np.array_equal(back[k], first[k]) for k in DEVICE_ARRAYS)
