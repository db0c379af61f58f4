"""Scene.set_rects on the device (rtx_scene_set_rects / _device: k_set_prims<5, FlatRect>, k_refit_bvh, k_refit_wide,
k_member_local_boxes, k_refit_instance_tree, k_slot_boxes, k_refresh_lights, and the host's copy of k_trace_vote's top-level
rectangles).

Two judges, neither the code under test: the resident ARRAYS after an update are byte-equal to those of the host-updated flat
scene uploaded afresh (rtx_flat_set_rects, which tests/test_set_rects_host.py holds to a fresh flatten and to the oracle), and
every ENTRY POINT on the updated scene answers bit for bit as on a FRESH upload of the same world built from scratch with the
moved rectangles.  A third, for the light: the radiance under a moved and resized area light against Lambert's closed form.
Frames are those of update_cases.cam_cfg, unchanged: 48 wide at aspect 1.5 (48 x 32), 4 spp, as in the other update tests."""
import ctypes as C

import numpy as np
import pytest

import cast_rays_cases as cc
import light_cases as lc
from rect_update_cases import CASES, DEVICE_ARRAYS, FORCED_KERNELS, LIGHT, LIGHT_MOVED, VOTE_CASES, beside_movers, cam_cfg, edge_values, probe_rays, refusals, update_of
from update_cases import KERNEL_OF, assert_arrays_equal as _assert_arrays_equal, call_set_prims, device_arrays, same_screen as _same_screen
from update_cases import upload as _upload

pytestmark = pytest.mark.gpu


def _device(scene):
    return device_arrays(scene, DEVICE_ARRAYS + ("plans",))


def _set(scene, ids, vals, entry):
    """Through the host entry (numpy) or the device entry (a torch tensor on the GPU, torch's current stream)."""
    if entry == "host":
        scene.set_rects(ids, vals)
        return
    import torch
    t = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float64)).cuda()
    scene.set_rects(ids, t)
    torch.cuda.synchronize()


# ---- 1. the arrays, every case, both entries
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_updated_arrays_equal_the_host_updated_scene_uploaded_fresh(rtsr, name, entry):
    """All ids; ids = 1 mod 3 of the parts; back to rest after each; two updates in a row; n = 0."""
    case = CASES[name](rtsr, False)
    flat = case.flatten()
    scene = _upload(flat)
    first = _device(scene)
    for what, sel in (("all", None), ("1 mod 3", lambda k: k % 3 == 1)):
        ids, vals = update_of(case, flat, select=sel)
        if not len(ids):
            continue
        _set(scene, ids, vals, entry)
        flat.set_rects(ids, vals)
        assert not np.array_equal(scene.array("rects"), first["rects"]), what
        _assert_arrays_equal(scene, _device(_upload(flat)), what)
        back = update_of(case, flat, moved=False, select=sel)
        _set(scene, *back, entry)
        flat.set_rects(*back)
        now = _device(scene)
        for k in first:  # back to rest: the arrays of the first upload, byte for byte (the cases keep every plane away from 0)
            assert np.array_equal(now[k], first[k]), (what, k)
    ids, vals = update_of(case, flat)
    half = len(ids) // 2
    _set(scene, ids[:half], vals[:half], entry)
    _set(scene, ids[half:], vals[half:], entry)
    flat.set_rects(ids, vals)
    _assert_arrays_equal(scene, _device(_upload(flat)), "two updates in a row")
    assert np.array_equal(_device(scene)["plans"], first["plans"])
    scene.set_rects([], np.zeros((0, 5)))  # n = 0: nothing launched


def test_wide_records_follow_the_refit(rtsr):
    case = CASES["rect_bvh65"](rtsr, False)
    flat = case.flatten()
    env = {"RTX_WIDE": "1"}
    scene = _upload(flat, env)
    assert scene.wide_levels() > 0 and len(scene.array("nodes4")) > 0
    first = scene.array("nodes4")
    ids, vals = update_of(case, flat)
    scene.set_rects(ids, vals)
    flat.set_rects(ids, vals)
    assert not np.array_equal(scene.array("nodes4"), first)
    # which nodes the collapse opened is KEPT by an update, while a fresh upload collapses by the new boxes: every array but
    # nodes4 is the fresh upload's, and the frame through the wide walk is
    fresh = _upload(flat, env)
    _assert_arrays_equal(scene, device_arrays(fresh, tuple(k for k in DEVICE_ARRAYS if k != "nodes4")), "wide")
    cam, cfg, h = cam_cfg(rtsr, case)
    want = fresh.render(cam, cfg)
    assert want.accum.std() > 0.01
    _same_screen(scene.render(cam, cfg), want, "wide")


EDGES = ("inverted", "zero extent", "negative zero k", "k = 1e13", "extents of 1e300", "itself")
WD_BOXED_PRIM = 8
DESC = np.dtype([("flags", np.int32), ("n_ops", np.int32), ("g", np.int32, (3,)), ("medium_mat", np.int32), ("box", np.float32, (6,)), ("rest", np.uint8, (144,))])


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("name", ["walls", "rect_bvh3"])
def test_edge_values_on_the_device(rtsr, name, edge, entry):
    """Inverted and zero extents, k = -0.0, k = 1e13 (k +- 0.0001 rounds back to k), extents of 1e300 (the slot box is not
    finite: WD_BOXED_PRIM clears) and a rectangle set to the values it has: arrays and a frame against an upload of the
    host-updated flat scene; `itself` leaves every array byte-identical."""
    case = CASES[name](rtsr, False)
    flat = case.flatten()
    scene = _upload(flat)
    first = _device(scene)
    h, rest, _ = case.parts[1]
    rid = flat.rect_ids(case.builder, h)
    vals = edge_values(rest[0])[edge]
    _set(scene, rid, [vals], entry)
    flat.set_rects(rid, [vals])
    fresh = _upload(flat)
    _assert_arrays_equal(scene, _device(fresh), edge)
    now = _device(scene)
    if edge == "itself":
        for k in first:
            assert np.array_equal(now[k], first[k]), k
    else:
        assert not np.array_equal(now["rects"], first["rects"])
    if name == "walls":
        slot = 0  # part 1 is the first slot of the world list (the light, made first, stands third)
        flags = now["world_desc"].view(DESC)["flags"]
        assert bool(flags[slot] & WD_BOXED_PRIM) == (edge != "extents of 1e300"), edge
    cam, cfg, hgt = cam_cfg(rtsr, case)
    _same_screen(scene.render(cam, cfg), fresh.render(cam, cfg), "%s %s" % (name, edge))
    _set(scene, rid, rest, entry)  # and back: the arrays of the first upload
    back = _device(scene)
    for k in first:
        assert np.array_equal(back[k], first[k]), (edge, k)


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("name", ["prism_field3", "prism_field65"])
def test_one_face_of_one_prism_on_the_device(rtsr, name, entry):
    """A partial GROUP: the top face of one member's prism rises, the other five stay.  member_local_box (through the tree above
    it), the nodes and a frame against an upload of the host-updated flat scene."""
    case = CASES[name](rtsr, False)
    flat = case.flatten()
    scene = _upload(flat)
    first = _device(scene)
    ids = flat.rect_ids(case.builder, case.parts[0][0])
    assert len(ids) == 6
    top = case.parts[0][1][2].copy()  # emission order: front, back, TOP, bottom, right, left
    top[4] += 0.45
    _set(scene, ids[2:3], [top], entry)
    flat.set_rects(ids[2:3], [top])
    fresh = _upload(flat)
    _assert_arrays_equal(scene, _device(fresh), "one face")
    now = _device(scene)
    assert not np.array_equal(now["nodes"], first["nodes"]) and not np.array_equal(now["rects"], first["rects"])
    cam, cfg, h = cam_cfg(rtsr, case)
    want = fresh.render(cam, cfg)
    assert want.accum.std() > 0.01
    _same_screen(scene.render(cam, cfg), want, "one face")
    # the next set_transforms reads the members' local boxes back: the lifted face must be in them
    slot = flat.instance_tree(0)["first_slot"]
    ops = {slot: [("translate", (0.9, 0.4, 1.3)), ("rotate_y", 33.0)]}
    scene.set_transforms(ops)
    flat.set_transforms(ops)
    _assert_arrays_equal(scene, _device(_upload(flat)), "one face, then set_transforms")


# ---- 2. every entry point on the updated scene against a fresh upload
def _pair(rtsr, name, entry, env=()):
    case, moved = CASES[name](rtsr, False), CASES[name](rtsr, True)
    flat = case.flatten()
    scene = _upload(flat, dict(env))
    _set(scene, *update_of(case, flat), entry)
    return scene, _upload(moved.flatten(), dict(env)), case


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("name", ["walls", "rect_bvh3", "rect_bvh65", "rect_bvh257_leaf1", "prism_field3", "prism_field65", "shared_prism"] + list(VOTE_CASES))
def test_renders_casts_and_queries_equal_the_fresh_upload(rtsr, name, entry):
    """rtx_render under RTX_TRACE_KERNEL unset, simple, vote, world and wavefront -- the vote cases through the device entry
    are the ones a stale copy of the top-level rectangles would fail -- then a cast_rays and a trace_rays batch."""
    honoured = set()
    for kernel in (None, "simple", "vote", "world", "wavefront"):
        env = (("RTX_TRACE_KERNEL", kernel),) if kernel else ()
        scene, fresh, case = _pair(rtsr, name, entry, env)
        cam, cfg, h = cam_cfg(rtsr, case)
        what = "%s %s %s" % (name, entry, kernel)
        want, got = fresh.render(cam, cfg, want_stats=True), scene.render(cam, cfg, want_stats=True)
        assert want.accum.std() > 0.01
        _same_screen(got, want, what)
        ran = rtsr.trace_kernel_name(got.stats.trace_kernel)
        assert ran == rtsr.trace_kernel_name(want.stats.trace_kernel), what
        if kernel is not None:
            assert ran == (KERNEL_OF[kernel] if kernel in FORCED_KERNELS[name] else "k_trace_world"), what
            if ran == KERNEL_OF[kernel]:
                honoured.add(kernel)
            continue
        o, d = probe_rays(case, 2000, 41)
        hm, hf = scene.cast_rays(o, d, seed=1, stream_step=1), fresh.cast_rays(o, d, seed=1, stream_step=1)
        assert hf.hit.sum() >= 200
        for col in ("t", "p", "normal", "uv", "ids"):
            assert cc.same_bits(getattr(hm, col).reshape(len(o), -1).astype(np.float64), getattr(hf, col).reshape(len(o), -1).astype(np.float64)).all(), col
        rm = scene.trace_rays(o[:500], d[:500], spp=4, max_depth=8, background=(0.05, 0.05, 0.08), sumsq=True)
        rf = fresh.trace_rays(o[:500], d[:500], spp=4, max_depth=8, background=(0.05, 0.05, 0.08), sumsq=True)
        assert rf.sum.std() > 0.001 and cc.same_bits(rm.sum, rf.sum).all() and cc.same_bits(rm.sumsq, rf.sumsq).all()
    assert honoured == FORCED_KERNELS[name], (name, sorted(honoured))


@pytest.mark.parametrize("entry", ["host", "device"])
def test_light_sampling_follows_the_light(rtsr, entry):
    """`walls` with light_sampling = 1: k_trace_nee reads the table k_refresh_lights wrote; set_shading of the light's colour
    after the resize leaves the table of the fresh upload with that colour."""
    scene, fresh, case = _pair(rtsr, "walls", entry)
    assert np.array_equal(scene.array("lights"), fresh.array("lights"))
    t = scene.array("lights").view(LIGHT)
    a0, a1, b0, b1, _ = LIGHT_MOVED
    assert len(t) == 1 and t["area"][0] == abs(a1 - a0) * abs(b1 - b0)
    cam, cfg, h = cam_cfg(rtsr, case)
    want = fresh.render(cam, cfg, light_sampling=True)
    assert want.accum.std() > 0.01
    _same_screen(scene.render(cam, cfg, light_sampling=True), want, "light sampling")
    mat = scene._flat.material(int(scene._flat.array("rects").view(np.dtype([("v", "f8", (5,)), ("axis", "i4"), ("mat", "i4")]))["mat"][0]))
    edit = [("solid_color", mat["tex"], (3.0, 9.0, 2.0))]
    scene.set_shading(edit)
    fresh.set_shading(edit)
    assert np.array_equal(scene.array("lights"), fresh.array("lights"))
    _same_screen(scene.render(cam, cfg, light_sampling=True), fresh.render(cam, cfg, light_sampling=True), "recoloured after the resize")


# ---- 3. the closed form: the update moved the LIGHT, not only the bytes
FLOOR_POINTS = ((2.6, 2.3), (3.1, 2.6), (2.2, 1.9))   # (x, z) under the moved light
CF_REST, CF_MOVED, CF_LE = (0.4, 1.6, 0.5, 1.7, 2.4), (2.3, 3.3, 2.0, 2.8, 1.1), np.array([9.0, 7.0, 5.0])


def _closed_form(vals, p):
    return lc.RHO / np.pi * CF_LE * lc.polygon_form(lc.rect_vertices("xz", *vals), np.array([p[0], 0.0, p[1]]))


@pytest.mark.parametrize("entry", ["host", "device"])
def test_radiance_under_the_moved_light_is_lambert_s_closed_form(rtsr, entry):
    """A Lambertian floor under an XZ light that the update slides, shrinks and lowers; rays straight down onto three floor
    points, depth 2, a black background, with light sampling.  Each point and channel within 4.5 standard errors
    (light_cases.Z_CAP) of the closed form for the NEW rectangle, which differs from the OLD one's by more than ten."""
    b = rtsr.Builder(5)
    light = b.xz_rect(*CF_REST, b.diffuse_light(tuple(CF_LE)))
    floor = b.xz_rect(-50.0, 50.0, -50.0, 50.0, 0.0, b.lambertian(tuple(lc.RHO)))
    flat = b.flatten(b.hittable_list([floor, light]))
    scene = _upload(flat)
    _set(scene, flat.rect_ids(b, light), [CF_MOVED], entry)
    o = np.array([[x, 0.5, z] for x, z in FLOOR_POINTS])
    od, dd = lc.replicated(o, np.tile([0.0, -1.0, 0.0], (3, 1)), 16)
    spp = 2048
    r = scene.trace_rays(od, dd, spp=spp, max_depth=2, background=(0.0, 0.0, 0.0), sumsq=True, light_sampling=True)
    mean, se = lc.mean_and_se(r.sum, r.sumsq, spp, n_points=3)
    new = np.array([_closed_form(CF_MOVED, p) for p in FLOOR_POINTS])
    old = np.array([_closed_form(CF_REST, p) for p in FLOOR_POINTS])
    z = lc.z_scores(mean, se, new)
    print("closed form: mean %s expected %s se %s z %s old %s" % (mean.tolist(), new.tolist(), se.tolist(), z.tolist(), old.tolist()))
    assert (np.abs(new - old) > 10.0 * se).all(), "the old and the new pose do not differ by ten standard errors"
    assert (se > 0).all() and z.max() <= lc.Z_CAP, "z %.2f" % z.max()


# ---- 4. patterns
def test_rects_transforms_rects_and_a_rebuild_on_one_scene(rtsr):
    case = CASES["prism_field65"](rtsr, False)
    flat = case.flatten()
    slot = flat.instance_tree(0)["first_slot"]
    ops = {slot: [("translate", (0.9, 0.4, 1.3)), ("rotate_y", 33.0)], slot + 3: [("translate", (2.9, 0.3, 0.7)), ("rotate_y", -12.0)]}
    steps = [("set_rects", lambda s: s.set_rects(*update_of(case, flat))),
             ("set_transforms", lambda s: s.set_transforms(ops)),
             ("set_rects again", lambda s: s.set_rects(*update_of(case, flat, moved=False, select=lambda k: k % 2 == 0))),
             ("rebuild_instance_trees", lambda s: s.rebuild_instance_trees()),
             ("set_rects after the rebuild", lambda s: s.set_rects(*update_of(case, flat, select=lambda k: k % 2 == 0)))]
    scene = _upload(flat)
    for what, apply in steps:
        apply(scene)
        apply(flat)
        _assert_arrays_equal(scene, _device(_upload(flat)), what)
    cam, cfg, h = cam_cfg(rtsr, case)
    want = _upload(flat).render(cam, cfg)
    assert want.accum.std() > 0.01
    _same_screen(scene.render(cam, cfg), want, "after the sequence")


def test_device_values_and_a_cast_on_a_side_stream(rtsr):
    import torch
    case = CASES["rect_bvh65"](rtsr, False)
    flat = case.flatten()
    scene = _upload(flat)
    ids, vals = update_of(case, flat)
    half = 0.5 * (vals + update_of(case, flat, moved=False)[1])
    fresh = _upload(CASES["rect_bvh65"](rtsr, True).flatten())
    o, d = probe_rays(case, 2000, 47)
    t_half, t_full = torch.from_numpy(half).cuda(), torch.from_numpy(vals).cuda()
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        scene.set_rects(ids, t_half)  # torch's current stream
        scene.set_rects(ids, t_full, stream=side)
        got = scene.cast_rays(to, td)  # behind both updates on the same stream, no host wait between
    side.synchronize()
    flat.set_rects(ids, vals)
    _assert_arrays_equal(scene, _device(_upload(flat)), "device entry on a side stream")
    ref = fresh.cast_rays(o, d)
    assert ref.hit.sum() >= 200
    assert cc.same_bits(got.t.cpu().numpy().reshape(-1, 1), ref.t.reshape(-1, 1)).all() and cc.same_bits(got.p.cpu().numpy(), ref.p).all()
    with pytest.raises(ValueError) as e:
        scene.set_rects(ids, t_full[:-1])
    assert "a0 a1 b0 b1 k" in str(e.value)
    with pytest.raises(ValueError):
        scene.set_rects(ids, t_full.float())


# ---- 5. refusals
def test_scene_refusals_enqueue_nothing(rtsr):
    case = CASES["vote_room7"](rtsr, False)
    flat = case.flatten()
    scene = _upload(flat)
    cam, cfg, h = cam_cfg(rtsr, case)
    first, frame = _device(scene), scene.render(cam, cfg)
    n_ids = flat.info()["n_rects"]
    for name, ids, n, vals, word, host_only in refusals(n_ids):
        st = call_set_prims(rtsr, rtsr.lib.rtx_scene_set_rects, scene.ptr, ids, n, vals, None)
        assert st == rtsr.RTX_EINVAL and "rtx_scene_set_rects" in rtsr.last_error() and word in rtsr.last_error(), (name, rtsr.last_error())
    import torch
    good = torch.ones(12, dtype=torch.float64).cuda()
    two = (C.c_int32 * 2)(0, 1)
    dev = rtsr.lib.rtx_scene_set_rects_device
    assert dev(scene.ptr, two, 2, C.c_void_p(good.data_ptr() + 4), None) == rtsr.RTX_EINVAL and "d_rects is not 8-byte aligned" in rtsr.last_error()
    assert dev(scene.ptr, (C.c_int32 * 2)(0, n_ids), 2, C.c_void_p(good.data_ptr()), None) == rtsr.RTX_EINVAL and "out of range" in rtsr.last_error()
    assert dev(scene.ptr, (C.c_int32 * 2)(1, 1), 2, C.c_void_p(good.data_ptr()), None) == rtsr.RTX_EINVAL and "twice" in rtsr.last_error()
    assert dev(scene.ptr, two, 2, None, None) == rtsr.RTX_EINVAL and "NULL" in rtsr.last_error()
    assert dev(scene.ptr, two, 0, C.c_void_p(good.data_ptr()), None) == rtsr.RTX_OK
    back = _device(scene)
    assert all(np.array_equal(back[k], first[k]) for k in first)
    _same_screen(scene.render(cam, cfg), frame, "after the refusals")
    # an f32 scene: refused; which = 19 names 28 bytes a record there
    ids, vals = update_of(case, flat)
    s32 = flat.upload(f32=True)
    f32_first = s32.render(cam, cfg)
    assert len(s32.array("rects")) == 28 * n_ids and len(scene.array("rects")) == 48 * n_ids
    with pytest.raises(rtsr.RtxError) as e:
        s32.set_rects(ids, vals)
    assert e.value.status == rtsr.RTX_EUNSUPPORTED and "rtx_flat_set_rects" in str(e.value) and "rtx_scene_upload_f32" in str(e.value)
    _same_screen(s32.render(cam, cfg), f32_first, "f32 after the refusal")
    # a BVH that holds a MovingSphere: its rectangle is refused, alone and among good ids; the plain slot beside it moves
    bm = beside_movers(rtsr, False)
    mflat = bm.flatten()
    mscene = _upload(mflat)
    mfirst = _device(mscene)
    bad = mflat.rect_ids(bm.builder, bm.handles["timed_rect"])
    ids, vals = update_of(bm, mflat)
    for i, v in ((bad, [[0.9, 1.7, 2.0, 2.8, 1.5]]), (np.concatenate([ids, bad]), np.concatenate([vals, [[0.9, 1.7, 2.0, 2.8, 1.5]]]))):
        with pytest.raises(rtsr.RtxError) as e:
            mscene.set_rects(i, v)
        assert e.value.status == rtsr.RTX_EUNSUPPORTED and "MovingSphere" in str(e.value)
    mback = _device(mscene)
    assert all(np.array_equal(mback[k], mfirst[k]) for k in mfirst)
    mscene.set_rects(ids, vals)
    mflat.set_rects(ids, vals)
    _assert_arrays_equal(mscene, _device(_upload(mflat)), "beside the movers")
