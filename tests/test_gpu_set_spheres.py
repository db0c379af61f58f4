"""Scene.set_spheres on the device (rtx_scene_set_spheres / _device: k_set_spheres, k_refit_bvh, k_refit_wide,
k_member_local_boxes, k_refit_instance_tree, k_sphere_slot_boxes, k_refresh_lights).

Two judges, neither the code under test: the resident ARRAYS after an update are byte-equal to those of the host-updated flat
scene uploaded afresh (rtx_flat_set_spheres, which tests/test_set_spheres_host.py holds to a fresh flatten and to the oracle),
and every ENTRY POINT on the updated scene answers bit for bit as on a FRESH upload of the same world built from scratch with
the moved spheres.  Frames are 48 x 32 at 4 spp."""
import ctypes as C

import numpy as np
import pytest

import cast_rays_cases as cc
from sphere_update_cases import (CASES, DESC, DEVICE_ARRAYS, FORCED_KERNELS, LDS_CASES, LIGHT, WD_BOXED_PRIM, WD_PAIR, assert_update_can_show, beside_movers, book1, book1_update,
                                 cam_cfg, instanced, refusals, rest_and_moved, seeded_rays, update_of)
from update_cases import KERNEL_OF, assert_arrays_equal as _assert_arrays_equal, call_set_prims, device_arrays, same_screen as _same_screen, updated_pair
from update_cases import upload as _upload

pytestmark = pytest.mark.gpu
def _device(scene):
    return device_arrays(scene, DEVICE_ARRAYS + ("plans",))


def _check_patterns(rtsr, case_fn, env=None):
    """Every update pattern of the issue on one case: all ids, one id, every 7th id, back to rest after each, and two updates
    enqueued back to back."""
    case = case_fn(rtsr, False)
    assert_update_can_show(*rest_and_moved(case))
    flat = case.flatten()
    scene = _upload(flat, env)
    first = _device(scene)
    _assert_arrays_equal(scene, _device(_upload(flat, env)), "upload")
    n_all = len(update_of(case, flat)[0])
    patterns = [("all", {}), ("one", {"only": 0})] + ([("every 7th", {"every": 7})] if n_all > 7 else [])
    for what, kw in patterns:
        ids, vals = update_of(case, flat, **kw)
        scene.set_spheres(ids, vals)
        flat.set_spheres(ids, vals)
        assert not np.array_equal(scene.array("spheres"), first["spheres"]), what
        _assert_arrays_equal(scene, _device(_upload(flat, env)), what)
        back = update_of(case, flat, moved=False, **kw)
        scene.set_spheres(*back)
        flat.set_spheres(*back)
        now = _device(scene)
        for k in first:  # back to rest: the arrays of the first upload, byte for byte (the cases keep every plane away from 0)
            assert np.array_equal(now[k], first[k]), (what, k)
    ids, vals = update_of(case, flat)
    half = len(ids) // 2
    scene.set_spheres(ids[:half], vals[:half])
    scene.set_spheres(ids[half:], vals[half:])
    flat.set_spheres(ids, vals)
    _assert_arrays_equal(scene, _device(_upload(flat, env)), "two updates in a row")
    assert np.array_equal(_device(scene)["plans"], first["plans"])
    scene.set_spheres([], np.zeros((0, 4)))  # n = 0: nothing launched


# ---- 1. the arrays
@pytest.mark.parametrize("name", sorted(CASES))
def test_updated_arrays_equal_the_host_updated_scene_uploaded_fresh(rtsr, name):
    _check_patterns(rtsr, CASES[name])


@pytest.mark.parametrize("name", ["mixed"])
def test_wide_records_follow_the_refit(rtsr, name):
    """The same under RTX_WIDE=1: the 4-wide records (which = 7) and their stack levels (which = 8).  (A world of spheres alone
    gets no 4-wide tree from the launcher, whatever the switch says: `mixed` is the case that has one.)"""
    case = CASES[name](rtsr, False)
    scene = _upload(case.flatten(), {"RTX_WIDE": "1"})
    assert scene.wide_levels() > 0 and len(scene.array("nodes4")) > 0
    _check_patterns(rtsr, CASES[name], {"RTX_WIDE": "1"})


def test_the_light_table_on_the_device_is_the_hosts(rtsr):
    """k_refresh_lights against build_light_table on the lamp's four updates, the uniform fallback among them; the slot records
    of the light carry its new box."""
    for name in ("lamp", "lamp_radius", "lamp_far", "lamp_dark"):
        case = CASES[name](rtsr, False)
        flat = case.flatten()
        scene = _upload(flat)
        t0 = scene.array("lights").view(LIGHT).copy()
        assert len(t0) == 2 and np.array_equal(t0.view(np.uint8), flat.array("lights"))
        ids, vals = update_of(case, flat, only=0)  # the light alone
        scene.set_spheres(ids, vals)
        flat.set_spheres(ids, vals)
        t1 = scene.array("lights").view(LIGHT)
        assert np.array_equal(t1.view(np.uint8), flat.array("lights")), name
        assert not np.array_equal(t1["pmf"], t0["pmf"]), name
        if name == "lamp_dark":
            assert list(t1["pmf"]) == [0.5, 0.5]
        _assert_arrays_equal(scene, _device(_upload(flat)), name)


def test_a_glass_ball_and_the_fog_inside_it_are_one_sphere_while_their_bytes_agree(rtsr):
    """The slot record of a plain sphere says whether the medium in the next slot is bounded by the very same sphere
    (build_world_desc compares the bytes).  The ball moved alone loses the flag; the boundary moved after it brings it back."""
    case = CASES["fog"](rtsr, False)
    flat = case.flatten()
    scene = _upload(flat)
    flags = lambda: scene.array("world_desc").view(DESC)["flags"]
    assert len(flags()) == 5 and flags()[1] & WD_PAIR and flags()[1] & WD_BOXED_PRIM and flags()[2] & WD_BOXED_PRIM
    for only, paired in ((0, False), (1, True)):
        ids, vals = update_of(case, flat, only=only)
        scene.set_spheres(ids, vals)
        flat.set_spheres(ids, vals)
        assert bool(flags()[1] & WD_PAIR) == paired and flags()[1] & WD_BOXED_PRIM and flags()[2] & WD_BOXED_PRIM
        _assert_arrays_equal(scene, _device(_upload(flat)), "fog %d" % only)


def test_book1_final_refits_on_the_device(rtsr, orc):
    """Catalogue scene 100 through k_trace_lds: arrays and frame against the host-updated flat scene uploaded fresh, and the
    frame against the CPU oracle on that flat scene."""
    b, world, cam, bg = book1(rtsr)
    flat = b.flatten(world)
    scene = _upload(flat)
    first = _device(scene)
    ids, rest, mv = book1_update(flat, b, world)
    assert_update_can_show(rest, mv)
    scene.set_spheres(ids, mv)
    flat.set_spheres(ids, mv)
    fresh = _upload(flat)
    _assert_arrays_equal(scene, _device(fresh), "book1")
    assert not np.array_equal(scene.array("nodes32"), first["nodes32"])
    cfg = rtsr.Config.new(1.5, 48, 4, 8, 4, seed=31, background=bg)
    h = rtsr.image_height(cfg)
    got, want = scene.render(cam, cfg, want_stats=True), fresh.render(cam, cfg, want_stats=True)
    assert rtsr.trace_kernel_name(got.stats.trace_kernel) == "k_trace_lds" == rtsr.trace_kernel_name(want.stats.trace_kernel)
    assert got.stats.trace_variant == want.stats.trace_variant == 0
    _same_screen(got, want, "book1")
    o2, o2_8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=4)
    assert np.array_equal(got.accum, o2) and np.array_equal(got.rgb8, o2_8)
    flat.set_spheres(ids, rest)
    for kernel in ("simple", "vote", "world", "wavefront"):  # a world of one BVH: the launcher accepts every forced kernel
        env = {"RTX_TRACE_KERNEL": kernel}
        forced = _upload(flat, env)
        forced.set_spheres(ids, mv)
        flat.set_spheres(ids, mv)
        f_got, f_want = forced.render(cam, cfg, want_stats=True), _upload(flat, env).render(cam, cfg, want_stats=True)
        assert rtsr.trace_kernel_name(f_got.stats.trace_kernel) == KERNEL_OF[kernel] == rtsr.trace_kernel_name(f_want.stats.trace_kernel)
        _same_screen(f_got, f_want, "book1 " + kernel)
        _same_screen(f_got, want, "book1 %s against k_trace_lds" % kernel)
        flat.set_spheres(ids, rest)
    scene.set_spheres(ids, rest)
    now = _device(scene)
    for k in first:
        assert np.array_equal(now[k], first[k]), k


# ---- 2. every entry point on the updated scene against a fresh upload
_PAIRS = {}


def _pair(rtsr, name, env=()):
    return updated_pair(_PAIRS, rtsr, CASES, update_of, "set_spheres", name, env)


@pytest.mark.parametrize("name", sorted(CASES))
def test_renders_on_the_updated_scene_equal_the_fresh_upload(rtsr, orc, name):
    """rtx_render under RTX_TRACE_KERNEL unset, simple, vote, world and wavefront; stats.trace_kernel is what was asked
    wherever choose_trace_kernel accepts the world (FORCED_KERNELS) and k_trace_world where it does not; by default a world
    of one sphere BVH runs k_trace_lds, variant 0.  Then a progressive handle made after the update, with its features, and
    the CPU oracle's frame of the host-updated flat scene."""
    honoured = set()
    for kernel in (None, "simple", "vote", "world", "wavefront"):
        env = (("RTX_TRACE_KERNEL", kernel),) if kernel else ()
        scene, fresh, flat, fresh_flat, case = _pair(rtsr, name, env)
        cam, cfg, h = cam_cfg(rtsr, case)
        assert (cfg.image_width, h, cfg.samples_per_pixel) == (48, 32, 4)
        what = "%s %s" % (name, kernel)
        want = fresh.render(cam, cfg, want_stats=True)
        got = scene.render(cam, cfg, want_stats=True)
        assert want.accum.std() > 0.01
        _same_screen(got, want, what)
        ran = rtsr.trace_kernel_name(got.stats.trace_kernel)
        assert ran == rtsr.trace_kernel_name(want.stats.trace_kernel), what
        if kernel is not None:
            assert ran == (KERNEL_OF[kernel] if kernel in FORCED_KERNELS[name] else "k_trace_world"), what
            if ran == KERNEL_OF[kernel]:
                honoured.add(kernel)
            continue
        if name in LDS_CASES:
            assert ran == "k_trace_lds" and got.stats.trace_variant == 0 and want.stats.trace_variant == 0, what
        pm, pf = scene.progressive(cam, cfg), fresh.progressive(cam, cfg)
        for p in (pm, pf):
            p.add(2)
            p.add(2)
        _same_screen(pm.screen(), pf.screen(), what + ": progressive")
        _same_screen(pm.screen(), want, what + ": progressive against the one-shot render")
        (am, nm), (af, nf) = pm.features(4), pf.features(4)
        assert af.std() > 0.01 and np.array_equal(am, af) and np.array_equal(nm, nf)
        o2, o2_8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=4)  # same topology as the host-updated flat scene
        assert np.array_equal(got.accum, o2) and np.array_equal(got.rgb8, o2_8)
    assert honoured == FORCED_KERNELS[name], (name, sorted(honoured))


@pytest.mark.parametrize("name", sorted(CASES))
def test_cast_rays_on_the_updated_scene_equal_the_fresh_upload(rtsr, name):
    scene, fresh, flat, fresh_flat, case = _pair(rtsr, name)
    o, d = seeded_rays(2000, 41)
    hm, hf = scene.cast_rays(o, d, seed=1, stream_step=1), fresh.cast_rays(o, d, seed=1, stream_step=1)
    assert hf.hit.sum() >= 200
    for col in ("t", "p", "normal", "uv", "ids"):
        assert cc.same_bits(getattr(hm, col).reshape(len(o), -1).astype(np.float64), getattr(hf, col).reshape(len(o), -1).astype(np.float64)).all(), col


@pytest.mark.parametrize("name", ["lamp", "lamp_radius", "lamp_far", "lamp_dark"])
def test_light_sampling_and_trace_rays_follow_the_light(rtsr, name):
    """light_sampling = 1 reads the table k_refresh_lights wrote: the frame and a radiance query equal the fresh upload's."""
    scene, fresh, flat, fresh_flat, case = _pair(rtsr, name)
    cam, cfg, h = cam_cfg(rtsr, case)
    want = fresh.render(cam, cfg, light_sampling=True)
    assert want.accum.std() > 0.01
    _same_screen(scene.render(cam, cfg, light_sampling=True), want, name + ": light sampling")
    pm, pf = scene.progressive(cam, cfg, light_sampling=True), fresh.progressive(cam, cfg, light_sampling=True)
    for p in (pm, pf):
        p.add(4)
    _same_screen(pm.screen(), pf.screen(), name + ": progressive with light sampling")
    o, d = seeded_rays(500, 43)
    for ls in (False, True):
        rm = scene.trace_rays(o, d, spp=4, max_depth=8, background=(0.05, 0.05, 0.08), sumsq=True, light_sampling=ls)
        rf = fresh.trace_rays(o, d, spp=4, max_depth=8, background=(0.05, 0.05, 0.08), sumsq=True, light_sampling=ls)
        assert rf.sum.std() > 0.001 and cc.same_bits(rm.sum, rf.sum).all() and cc.same_bits(rm.sumsq, rf.sumsq).all(), ls


# ---- 3. the device entry
def test_device_values_on_a_side_stream(rtsr):
    """A torch float64 tensor on a non-default stream: two updates and a cast enqueued on it without a host wait give the
    answers of the second update; then the frame of the second update."""
    import torch
    case = CASES["field65"](rtsr, False)
    flat = case.flatten()
    scene, twin = _upload(flat), _upload(flat)
    ids, vals = update_of(case, flat)
    half = 0.5 * (vals + update_of(case, flat, moved=False)[1])  # halfway there
    twin.set_spheres(ids, vals)
    want = _device(twin)
    fresh = _upload(CASES["field65"](rtsr, True).flatten())
    cam, cfg, h = cam_cfg(rtsr, case)
    o, d = seeded_rays(2000, 47)
    t_half, t_full = torch.from_numpy(half).cuda(), torch.from_numpy(vals).cuda()
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        scene.set_spheres(ids, t_half, stream=side)
        scene.set_spheres(ids, t_full, stream=side)
        got = scene.cast_rays(to, td)  # behind both updates on the same stream
    side.synchronize()
    _assert_arrays_equal(scene, want, "device entry")
    ref = fresh.cast_rays(o, d)
    assert ref.hit.sum() >= 200
    assert cc.same_bits(got.t.cpu().numpy().reshape(-1, 1), ref.t.reshape(-1, 1)).all() and cc.same_bits(got.p.cpu().numpy(), ref.p).all()
    _same_screen(scene.render(cam, cfg), fresh.render(cam, cfg), "after two updates on a side stream")
    scene.set_spheres([], torch.zeros((0, 4), dtype=torch.float64, device="cuda"))  # n = 0 through the tensor path
    _assert_arrays_equal(scene, want, "after an empty device update")
    with pytest.raises(ValueError):
        scene.set_spheres(ids, t_full[:-1])
    with pytest.raises(ValueError):
        scene.set_spheres(ids, t_full.float())


# ---- 4. one scene through every update
SEQUENCE_POSES = ((((1.0, 0.5, 0.2), 50.0), ((2.5, 0.1, 3.0), -10.0), ((0.3, 0.6, 3.2), None)),)


def test_one_scene_through_spheres_triangles_transforms_a_rebuild_and_spheres_again(rtsr):
    """set_spheres, set_triangles, set_transforms (the first after an update of members: it reads their local boxes back),
    rebuild_instance_trees, set_spheres -- on ONE resident scene.  After every step the resident arrays and max_stack are those
    of the flat scene taken through the same step on the host and uploaded fresh; then one frame on both."""
    case = instanced(rtsr, False)
    flat = case.flatten()
    assert flat.instances()["n_trees"] == 1 and flat.instance_tree(0)["n_slots"] == 4
    first_slot = flat.instance_tree(0)["first_slot"]
    pose = SEQUENCE_POSES[0]
    ops = {first_slot + k: [("translate", off)] + ([("rotate_y", ang)] if ang is not None else []) for k, (off, ang) in enumerate(pose)}
    tri_ids = flat.triangle_ids(case.builder, case.mesh)
    steps = [("set_spheres", lambda s: s.set_spheres(*update_of(case, flat))),
             ("set_triangles", lambda s: s.set_triangles(tri_ids, case.mesh_moved.reshape(-1, 9))),
             ("set_transforms", lambda s: s.set_transforms(ops)),
             ("rebuild_instance_trees", lambda s: s.rebuild_instance_trees()),
             ("set_spheres again", lambda s: s.set_spheres(*update_of(case, flat, moved=False, every=2)))]
    scene = _upload(flat)
    before = _device(scene)
    for what, apply in steps:
        apply(scene)
        apply(flat)
        _assert_arrays_equal(scene, _device(_upload(flat)), what)
        now = _device(scene)
        assert what == "rebuild_instance_trees" or not np.array_equal(now["nodes"], before["nodes"]), what
        before = now
    cam, cfg, h = cam_cfg(rtsr, case)
    want = _upload(flat).render(cam, cfg)
    assert want.accum.std() > 0.01
    _same_screen(scene.render(cam, cfg), want, "after the sequence")


# ---- 5. the slot boxes of both kinds
SLOT_ARRAYS = ("top_box32", "world_desc", "triangles", "spheres")


@pytest.mark.parametrize("n_tris", [256, 257])
def test_triangle_and_sphere_slots_get_their_boxes_from_one_kernel(rtsr, n_tris):
    """k_slot_boxes on a world of plain slots alone, no BVH over them: a triangle, a glass ball, the fog inside it (bounded by a
    sphere of the very same bytes: WD_PAIR), then n_tris - 1 more triangles.  256 triangle slots fill one block of the grid, 257
    cross into the second.  Every triangle updated, the ball moved alone (the pair flag clears), the ball set back (it returns);
    then the first and the last triangle alone, which must leave every slot not listed as it was.  After every step the four
    arrays are those of the host-updated flat scene uploaded afresh, and the step has changed what it should."""
    from deform_cases import displace
    b = rtsr.Builder(3)
    red, glass = b.lambertian((0.8, 0.3, 0.3)), b.dielectric(1.5)
    rest = np.array([[(0.3 + 0.02 * k, 1.0 + 0.001 * k, 0.4), (0.5 + 0.02 * k, 1.1, 0.5 + 0.003 * k), (0.4 + 0.02 * k, 1.6, 0.9)] for k in range(n_tris)])
    moved = displace(rest, 0.4)
    tris = [b.triangle(tuple(t[0]), tuple(t[1]), tuple(t[2]), red) for t in rest]
    ball_rest, ball_moved = np.array([[1.71, 1.32, 2.93, 1.1]]), np.array([[4.13, 1.74, 2.21, 0.85]])
    ball, inside = b.sphere(tuple(ball_rest[0, :3]), ball_rest[0, 3], glass), b.sphere(tuple(ball_rest[0, :3]), ball_rest[0, 3], glass)
    world = b.hittable_list([tris[0], ball, b.constant_medium((0.2, 0.4, 0.9), 0.8, inside)] + tris[1:])
    flat = b.flatten(world)
    assert flat.info()["n_top_level"] == n_tris + 2 and flat.info()["n_bvh"] == 0 and flat.instances()["n_trees"] == 0
    tri_ids, ball_id = flat.triangle_ids(b, world), flat.sphere_ids(b, ball)
    assert len(tri_ids) == n_tris and len(set(tri_ids.tolist())) == n_tris and len(ball_id) == 1
    slot_of = lambda k: 0 if k == 0 else k + 2  # triangle number k -> its slot
    scene = _upload(flat)
    desc = lambda a: a["world_desc"].view(DESC)
    now = lambda: device_arrays(scene, SLOT_ARRAYS)
    first = now()
    assert len(desc(first)) == n_tris + 2 and desc(first)["flags"][1] & WD_PAIR and all(desc(first)["flags"] & WD_BOXED_PRIM)

    def step(what, setter, ids, values, changed, paired):
        before = now()
        getattr(scene, setter)(ids, values)
        getattr(flat, setter)(ids, values)
        after = now()
        _assert_arrays_equal(scene, device_arrays(_upload(flat), SLOT_ARRAYS), what)
        for k in SLOT_ARRAYS:  # the step shows where it should, and nowhere else
            assert np.array_equal(after[k], before[k]) == (k not in changed), (what, k)
        assert bool(desc(after)["flags"][1] & WD_PAIR) == paired and all(desc(after)["flags"] & WD_BOXED_PRIM), what
        return before, after

    step("every triangle", "set_triangles", tri_ids, moved.reshape(-1, 9), ("top_box32", "world_desc", "triangles"), True)
    step("the ball alone", "set_spheres", ball_id, ball_moved, ("top_box32", "world_desc", "spheres"), False)
    step("the ball back", "set_spheres", ball_id, ball_rest, ("top_box32", "world_desc", "spheres"), True)
    for k in (0, n_tris - 1):  # one triangle back to rest: its slot alone
        before, after = step("triangle %d alone" % k, "set_triangles", tri_ids[k:k + 1], rest[k].reshape(1, 9), ("top_box32", "world_desc", "triangles"), True)
        others = np.arange(n_tris + 2) != slot_of(k)
        assert np.array_equal(after["top_box32"].view(np.float32).reshape(-1, 6)[others], before["top_box32"].view(np.float32).reshape(-1, 6)[others])
        assert np.array_equal(desc(after)[others], desc(before)[others])
        assert not np.array_equal(desc(after)["box"][~others], desc(before)["box"][~others])


# ---- 6. refusals
def test_scene_refusals_enqueue_nothing(rtsr):
    case = CASES["mixed"](rtsr, False)
    flat = case.flatten()
    scene = _upload(flat)
    cam, cfg, h = cam_cfg(rtsr, case)
    first, frame = _device(scene), scene.render(cam, cfg)
    n_ids = flat.info()["n_spheres"]
    for name, ids, n, vals, word, host_only in refusals(n_ids):  # duplicate ids and values that are not finite among them
        st = call_set_prims(rtsr, rtsr.lib.rtx_scene_set_spheres, scene.ptr, ids, n, vals, None)
        assert st == rtsr.RTX_EINVAL and "rtx_scene_set_spheres" in rtsr.last_error() and word in rtsr.last_error(), (name, rtsr.last_error())
    import torch
    good = torch.ones(8, dtype=torch.float64).cuda()
    two = (C.c_int32 * 2)(0, 1)
    dev = rtsr.lib.rtx_scene_set_spheres_device
    assert dev(scene.ptr, two, 2, C.c_void_p(good.data_ptr() + 4), None) == rtsr.RTX_EINVAL and "8-byte aligned" in rtsr.last_error()
    assert dev(scene.ptr, (C.c_int32 * 2)(0, n_ids), 2, C.c_void_p(good.data_ptr()), None) == rtsr.RTX_EINVAL and "out of range" in rtsr.last_error()
    assert dev(scene.ptr, (C.c_int32 * 2)(1, 1), 2, C.c_void_p(good.data_ptr()), None) == rtsr.RTX_EINVAL and "twice" in rtsr.last_error()
    assert dev(scene.ptr, two, 2, None, None) == rtsr.RTX_EINVAL and "NULL" in rtsr.last_error()
    assert dev(scene.ptr, two, 0, C.c_void_p(good.data_ptr()), None) == rtsr.RTX_OK
    back = _device(scene)
    assert all(np.array_equal(back[k], first[k]) for k in first)
    _same_screen(scene.render(cam, cfg), frame, "after the refusals")
    # an f32 scene
    ids, vals = update_of(case, flat)
    s32 = flat.upload(f32=True)
    f32_first = s32.render(cam, cfg)
    with pytest.raises(rtsr.RtxError) as e:
        s32.set_spheres(ids, vals)
    assert e.value.status == rtsr.RTX_EUNSUPPORTED and "rtx_flat_set_spheres" in str(e.value) and "rtx_scene_upload_f32" in str(e.value)
    _same_screen(s32.render(cam, cfg), f32_first, "f32 after the refusal")
    # the BVH that holds a MovingSphere: its static sphere is refused, alone and among good ids; the field beside it moves
    bm = beside_movers(rtsr, False)
    mflat = bm.flatten()
    mscene = _upload(mflat)
    mfirst, mframe = _device(mscene), mscene.render(cam, cfg)
    bad = mflat.sphere_ids(bm.builder, bm.handles["timed_static"])
    ids, vals = update_of(bm, mflat)
    for i, v in ((bad, [[0.9, 2.7, 5.1, 0.2]]), (np.concatenate([ids, bad]), np.concatenate([vals, [[0.9, 2.7, 5.1, 0.2]]]))):
        with pytest.raises(rtsr.RtxError) as e:
            mscene.set_spheres(i, v)
        assert e.value.status == rtsr.RTX_EUNSUPPORTED and "MovingSphere" in str(e.value)
    mback = _device(mscene)
    assert all(np.array_equal(mback[k], mfirst[k]) for k in mfirst)
    _same_screen(mscene.render(cam, cfg), mframe, "movers after the refusal")
    mscene.set_spheres(ids, vals)
    mflat.set_spheres(ids, vals)
    _assert_arrays_equal(mscene, _device(_upload(mflat)), "the field beside the movers")
