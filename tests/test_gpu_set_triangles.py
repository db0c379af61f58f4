"""Scene.set_triangles on the device (rtx_scene_set_triangles / _device: k_set_triangles, k_refit_bvh, k_refit_wide,
k_member_local_boxes, k_top_triangle_boxes).

Two judges, neither the code under test: the resident ARRAYS after an update are byte-equal to those of the host-updated flat
scene uploaded afresh (rtx_flat_set_triangles, which tests/test_set_triangles_host.py holds to a fresh flatten and to the
oracle), and every ENTRY POINT on the updated scene answers bit for bit as on a FRESH upload of the same world built from
scratch with the displaced vertices."""
import numpy as np
import pytest

import cast_rays_cases as cc
from deform_cases import (CASES, refusals, DEVICE_ARRAYS, NODE, NODE4, SHEET_LEAVES, cam_cfg, count_leaves, movers, narrow, sheet, sheet_tris_for_leaves, update_of, update_sequence)
from update_cases import KERNEL_OF, assert_arrays_equal as _assert_arrays_equal, call_set_prims, device_arrays, same_screen as _same_screen, updated_pair
from update_cases import upload as _upload

pytestmark = pytest.mark.gpu
def _device(scene):
    return device_arrays(scene, DEVICE_ARRAYS)


def _check_patterns(rtsr, orc, case_fn, audit):
    """Every update pattern of the issue on one case: all ids, one id, every 7th id, two updates in a row, back to rest."""
    case = case_fn(rtsr, False)
    flat = case.flatten()
    scene = _upload(flat)
    first = _device(scene)
    _assert_arrays_equal(scene, _device(_upload(flat)), "upload")
    n_all = len(update_of(case, flat)[0])
    patterns = [("all", {})] + ([("one", {"only": min(3, n_all - 1)}), ("every 7th", {"every": 7})] if n_all > 1 else [])
    for what, kw in patterns:
        ids, verts = update_of(case, flat, **kw)
        scene.set_triangles(ids, verts)
        flat.set_triangles(ids, verts)
        assert not np.array_equal(flat.array("nodes"), first["nodes"]) or len(first["nodes"]) == 0
        _assert_arrays_equal(scene, _device(_upload(flat)), what)
        rc, _ = orc.audit_flat_exact(flat.arrays_ptr(), nodes=scene.array("nodes").view(orc.FLAT_NODE), **audit)
        assert rc == 0, what
        back = update_of(case, flat, moved=False, **kw)
        scene.set_triangles(*back)
        flat.set_triangles(*back)
        now = _device(scene)
        assert all(np.array_equal(now[k], first[k]) for k in DEVICE_ARRAYS), what
    if n_all > 1:  # two updates enqueued back to back, nothing between them
        ids, verts = update_of(case, flat)
        half = len(ids) // 2
        scene.set_triangles(ids[:half], verts[:half])
        scene.set_triangles(ids[half:], verts[half:])
        flat.set_triangles(ids, verts)
        _assert_arrays_equal(scene, _device(_upload(flat)), "two updates in a row")
    scene.set_triangles([], np.zeros((0, 9)))  # n = 0: nothing launched


# ---- 1. the arrays
@pytest.mark.parametrize("name", sorted(CASES))
def test_updated_arrays_equal_the_host_updated_scene_uploaded_fresh(rtsr, orc, name):
    _check_patterns(rtsr, orc, CASES[name], {"ask_first": True})


@pytest.mark.parametrize("max_leaf", [1, 0])
@pytest.mark.parametrize("leaves", SHEET_LEAVES)
def test_sheets_by_their_number_of_leaves(rtsr, orc, leaves, max_leaf):
    """Root only, one inner child, a wave and a block boundary on either side, 1024 leaves."""
    n = sheet_tris_for_leaves(rtsr, leaves, max_leaf)
    assert count_leaves(sheet(rtsr, False, n, max_leaf).flatten()) == leaves
    _check_patterns(rtsr, orc, lambda r, mv: sheet(r, mv, n, max_leaf), {"ask_first": True})


def test_two_triangles_at_max_leaf_two(rtsr, orc):
    """The smallest BVH the flattener makes: ONE node holding two one-triangle leaves (build_bvh forces a node, so a leaf code
    for a root does not come out of a flatten; tests/set_triangles_host_check.cpp makes one by hand for the host path)."""
    flat = sheet(rtsr, False, 2, 2).flatten()
    assert flat.info()["n_nodes"] == 1 and count_leaves(flat) == 2
    _check_patterns(rtsr, orc, lambda r, mv: sheet(r, mv, 2, 2), {"ask_first": True})


def test_a_tree_from_the_gpu_builder_keeps_its_leaf_order(rtsr, orc):
    """2 048 triangles with gpu_builder: a Karras tree of full two-triangle clusters in leaf order, still one after the update."""
    case = sheet(rtsr, False, 2048, gpu_builder=True)
    flat = case.flatten()
    audit = {"leaf_order": True, "full_leaves": 2}
    assert orc.audit_flat_exact(flat.arrays_ptr(), **audit)[0] == 0
    scene = _upload(flat)
    first = _device(scene)
    ids, verts = update_of(case, flat)
    scene.set_triangles(ids, verts)
    flat.set_triangles(ids, verts)
    assert not np.array_equal(flat.array("nodes"), first["nodes"])
    assert orc.audit_flat_exact(flat.arrays_ptr(), **audit)[0] == 0
    assert orc.audit_flat_exact(flat.arrays_ptr(), nodes=scene.array("nodes").view(orc.FLAT_NODE), **audit)[0] == 0
    _assert_arrays_equal(scene, _device(_upload(flat)), "karras")


def test_three_host_updates_in_a_row_allocate_reuse_and_regrow_the_staging_buffer(rtsr):
    """One resident sheet of 65 leaves through the host-vertex entry with 1 id, 7 ids, then every id: the pinned block and its
    device twin are made by the first call and outgrown by the next two; a fourth call (back to rest) fits what is there.  The
    arrays are compared after every call."""
    case = sheet(rtsr, False, 65, 1)
    flat = case.flatten()
    assert count_leaves(flat) == 65
    scene = _upload(flat)
    first = _device(scene)
    for what, kw, n in (("1 id", {"only": 3}, 1), ("7 ids", {"every": 10}, 7), ("every id", {}, 65)):
        ids, verts = update_of(case, flat, **kw)
        assert len(ids) == n
        scene.set_triangles(ids, verts)
        flat.set_triangles(ids, verts)
        _assert_arrays_equal(scene, _device(_upload(flat)), what)
    assert not np.array_equal(scene.array("nodes"), first["nodes"])
    scene.set_triangles(*update_of(case, flat, moved=False))
    back = _device(scene)
    assert all(np.array_equal(back[k], first[k]) for k in DEVICE_ARRAYS)


def test_one_scene_through_set_triangles_set_transforms_and_a_rebuild(rtsr):
    """deform_cases.update_sequence on ONE resident scene: set_triangles, set_transforms (the first after a mesh update: it reads
    the members' local boxes back), rebuild_instance_trees, set_triangles, set_transforms.  After every step the resident
    arrays and max_stack are those of the flat scene taken through the same step on the host (the Morton rebuild) and uploaded
    fresh; then one 48 x 27 frame at 4 spp on both.  The host sequence itself is held to the end state built from scratch by
    tests/test_set_triangles_host.py."""
    case = CASES["instanced"](rtsr, False)
    flat = case.flatten()
    assert flat.instances()["n_trees"] == 1 and flat.instance_tree(0)["n_slots"] == 3
    scene = _upload(flat)
    before = _device(scene)
    for what, apply in update_sequence(case, flat):
        apply(scene)
        apply(flat)
        _assert_arrays_equal(scene, _device(_upload(flat)), what)
        assert scene.max_stack() == flat.info()["max_stack"], what
        now = _device(scene)
        assert what == "rebuild_instance_trees" or not np.array_equal(now["nodes"], before["nodes"]), what
        before = now
    cam = rtsr.Camera.new(case.look[0], case.look[1], (0.0, 1.0, 0.0), 35.0, 16.0 / 9.0, 0.0, 10.0, 0.0, 1.0)
    cfg = rtsr.Config.new(16.0 / 9.0, 48, 4, 8, 4, seed=31)
    assert (cfg.image_width, rtsr.image_height(cfg), cfg.samples_per_pixel) == (48, 27, 4)
    want = _upload(flat).render(cam, cfg)
    assert want.accum.std() > 0.01
    _same_screen(scene.render(cam, cfg), want, "after the sequence")


# ---- 2. the 4-wide tree
def _wide_cases(rtsr):
    out = [("sheet %d leaves" % l, (lambda r, mv, n=sheet_tris_for_leaves(rtsr, l, 1): sheet(r, mv, n, 1))) for l in (2, 3, 4, 5, 64, 257)]
    return out + [("mixed", CASES["mixed"])]


def test_wide_records_follow_the_refitted_binary_tree(rtsr):
    checked = 0
    for what, fn in _wide_cases(rtsr):
        case = fn(rtsr, False)
        flat = case.flatten()
        scene = _upload(flat, {"RTX_WIDE": "1"})
        wide0 = scene.array("nodes4").view(NODE4).copy()
        levels0 = scene.wide_levels()
        assert len(wide0) == flat.info()["n_nodes"] and levels0 > 0, "%s: the scene has no wide tree" % what
        nodes0 = scene.array("nodes")
        scene.set_triangles(*update_of(case, flat))
        wide, nodes = scene.array("nodes4").view(NODE4), scene.array("nodes").view(NODE)
        assert not np.array_equal(nodes.view(np.uint8), nodes0)
        assert np.array_equal(wide["child"], wide0["child"]) and np.array_equal(wide["pad"], wide0["pad"]) and scene.wide_levels() == levels0
        # every child code of the binary tree -> its f64 box there
        box = {}
        for n in range(len(nodes)):
            for c in range(2):
                box.setdefault(int(nodes["child"][n][c]), (nodes["bmin"][n][c], nodes["bmax"][n][c]))
        for i in range(len(wide)):
            if not wide["child"][i].any():
                assert wide[i].tobytes() == wide0[i].tobytes()  # a record no walk reaches
                continue
            for k in range(4):
                code = int(wide["child"][i][k])
                if code == 0x7fffffff:
                    assert np.all(wide["lo"][i][:, k] == np.inf) and np.all(wide["hi"][i][:, k] == -np.inf)
                    continue
                lo, hi = box[code]
                assert np.array_equal(wide["lo"][i][:, k], narrow(lo, up=False)) and np.array_equal(wide["hi"][i][:, k], narrow(hi, up=True)), (what, i, k)
                checked += 1
        # and the whole record array is the one a fresh upload of the host-updated scene collapses, where that opens the same nodes
        flat.set_triangles(*update_of(case, flat))
        fresh_wide = _upload(flat, {"RTX_WIDE": "1"}).array("nodes4").view(NODE4)
        if np.array_equal(fresh_wide["child"], wide["child"]):
            assert np.array_equal(fresh_wide.view(np.uint8), wide.view(np.uint8)), what
    assert checked > 300


# ---- 3. every entry point on the updated scene against a fresh upload
ENTRY_CASES = ["sheet257_leaf1", "mixed", "shared", "instanced", "fog"]
SIZES = ((48, 4), (120, 2))
# The forced kernels the launcher accepts each world under (choose_trace_kernel): `simple` and `world` take any world; `vote` and
# the wavefront integrator a world of ONE BVH beside plain primitives, which a chain over a member or a medium is not.
FORCED_KERNELS = {"sheet257_leaf1": {"simple", "vote", "world", "wavefront"}, "mixed": {"simple", "vote", "world", "wavefront"},
                  "shared": {"simple", "vote", "world", "wavefront"}, "instanced": {"simple", "world"}, "fog": {"simple", "world"}}
_PAIRS = {}


def _pair(rtsr, name, env=()):
    return updated_pair(_PAIRS, rtsr, CASES, update_of, "set_triangles", name, env)


@pytest.mark.parametrize("name", ENTRY_CASES)
def test_renders_on_the_updated_scene_equal_the_fresh_upload(rtsr, orc, name):
    """rtx_render under RTX_TRACE_KERNEL unset, simple, vote, world and wavefront, each with RTX_WIDE unset, 0 and 1;
    stats.trace_kernel is what was asked wherever the launcher accepts the world (FORCED_KERNELS) and k_trace_world where it
    does not; rtx_render_ex with light sampling; a progressive
    handle made after the update, with its features.  The updated scene's frame is also O2's of the host-updated flat scene."""
    honoured = set()
    for kernel in (None, "simple", "vote", "world", "wavefront"):
        for wide in (None, "0", "1"):
            env = tuple(sorted({k: v for k, v in (("RTX_TRACE_KERNEL", kernel), ("RTX_WIDE", wide)) if v is not None}.items()))
            scene, fresh, flat, fresh_flat, case = _pair(rtsr, name, env)  # (no switch makes an upload or an update fail)
            for width, spp in SIZES if (kernel, wide) == (None, None) else SIZES[:1]:
                cam, cfg, h = cam_cfg(rtsr, case, width=width, spp=spp)
                assert (cfg.image_width, h, cfg.samples_per_pixel) == (width, width * 2 // 3, spp)
                what = "%s %s wide=%s %d" % (name, kernel, wide, width)
                want = fresh.render(cam, cfg, want_stats=True)
                got = scene.render(cam, cfg, want_stats=True)
                assert want.accum.std() > 0.01
                _same_screen(got, want, what)
                ran = rtsr.trace_kernel_name(got.stats.trace_kernel)
                assert ran == rtsr.trace_kernel_name(want.stats.trace_kernel), what
                if kernel is not None:
                    # the launcher accepts a forced kernel or quietly walks the world with k_trace_world: what was asked ran
                    # exactly where FORCED_KERNELS says the launcher accepts this world
                    assert ran == (KERNEL_OF[kernel] if kernel in FORCED_KERNELS[name] else "k_trace_world"), what
                    if ran == KERNEL_OF[kernel]:
                        honoured.add(kernel)
                if (kernel, wide) == (None, None):
                    _same_screen(scene.render(cam, cfg, light_sampling=True), fresh.render(cam, cfg, light_sampling=True), what + ": light sampling")
                    pm, pf = scene.progressive(cam, cfg), fresh.progressive(cam, cfg)
                    for p in (pm, pf):
                        p.add(spp // 2)
                        p.add(spp - spp // 2)
                    _same_screen(pm.screen(), pf.screen(), what + ": progressive")
                    _same_screen(pm.screen(), want, what + ": progressive against the one-shot render")
                    (am, nm), (af, nf) = pm.features(4), pf.features(4)
                    assert af.std() > 0.01 and np.array_equal(am, af) and np.array_equal(nm, nf)
                    if width == 48:  # same topology as the host-updated flat scene, so ties included
                        o2, o2_8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=4)
                        assert np.array_equal(got.accum, o2) and np.array_equal(got.rgb8, o2_8)
    assert honoured == FORCED_KERNELS[name], (name, sorted(honoured))


@pytest.mark.parametrize("name", ENTRY_CASES)
def test_ray_queries_on_the_updated_scene_equal_the_fresh_upload(rtsr, name):
    """cast_rays at every triangle's centroid from two sides, all columns; trace_rays at 4 spp."""
    scene, fresh, flat, fresh_flat, case = _pair(rtsr, name)
    tris = np.concatenate([mv for _, _, mv in case.parts])
    centroid = tris.mean(axis=1)
    normal = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    normal /= np.linalg.norm(normal, axis=1)[:, None]
    if name == "instanced":  # the members' triangles are given in local space: aim at the scene from above and below instead
        centroid = centroid + np.array([1.0, 0.3, 1.5])
        normal = np.tile(np.array([0.05, 1.0, 0.08]), (len(centroid), 1))
    o = np.concatenate([centroid + 3.0 * normal, centroid - 3.0 * normal])
    d = np.concatenate([-normal, normal])
    hm, hf = scene.cast_rays(o, d, seed=1, stream_step=1), fresh.cast_rays(o, d, seed=1, stream_step=1)
    assert hf.hit.sum() >= len(o) // 2
    for col in ("t", "p", "normal", "uv", "ids"):
        assert cc.same_bits(getattr(hm, col).reshape(len(o), -1).astype(np.float64), getattr(hf, col).reshape(len(o), -1).astype(np.float64)).all(), col
    rm = scene.trace_rays(o, d, spp=4, max_depth=8, background=(0.35, 0.4, 0.55), sumsq=True)
    rf = fresh.trace_rays(o, d, spp=4, max_depth=8, background=(0.35, 0.4, 0.55), sumsq=True)
    assert rf.sum.std() > 0.01 and cc.same_bits(rm.sum, rf.sum).all() and cc.same_bits(rm.sumsq, rf.sumsq).all()


# ---- 4. the device entry
def test_device_vertices_on_a_side_stream(rtsr):
    """A torch float64 tensor on a non-default stream gives the arrays of the host entry; two updates enqueued back to back and
    a cast on the same stream, no host wait between them, give the answers of the second.  (The work behind the updates on
    the side stream is a CAST, not a render: Scene.render takes no stream, Scene.cast_rays with device tensors runs on the
    current one.  The frame of the second update is rendered after the stream has been waited for.)"""
    import torch
    case = CASES["mixed"](rtsr, False)
    flat = case.flatten()
    scene, twin = _upload(flat), _upload(flat)
    ids, verts = update_of(case, flat)
    half = 0.5 * (verts + update_of(case, flat, moved=False)[1])  # halfway there
    twin.set_triangles(ids, verts)
    want = _device(twin)
    fresh = _upload(CASES["mixed"](rtsr, True).flatten())
    cam, cfg, h = cam_cfg(rtsr, case)
    tris = verts.reshape(-1, 3, 3)
    o = tris.mean(axis=1) + np.array([0.0, 4.0, 0.0])
    d = np.tile(np.array([0.0, -1.0, 0.0]), (len(o), 1))
    t_half, t_full = torch.from_numpy(half).cuda(), torch.from_numpy(verts).cuda()
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        scene.set_triangles(ids, t_half, stream=side)
        scene.set_triangles(ids, t_full, stream=side)
        got = scene.cast_rays(to, td)  # behind both updates on the same stream
    side.synchronize()
    _assert_arrays_equal(scene, want, "device entry")
    ref = fresh.cast_rays(o, d)
    assert ref.hit.sum() >= len(o) // 2
    assert cc.same_bits(got.t.cpu().numpy().reshape(-1, 1), ref.t.reshape(-1, 1)).all() and cc.same_bits(got.p.cpu().numpy(), ref.p).all()
    _same_screen(scene.render(cam, cfg), fresh.render(cam, cfg), "after two updates on a side stream")
    # n = 0 through the tensor path: nothing to do, not "vertices is NULL" for the empty tensor's null pointer
    scene.set_triangles([], torch.zeros((0, 9), dtype=torch.float64, device="cuda"))
    _assert_arrays_equal(scene, want, "after an empty device update")
    # a transform update after a device-side triangle update still checks against the boxes as they are now
    inst = CASES["instanced"](rtsr, False)
    iflat = inst.flatten()
    iscene = _upload(iflat)
    iids, iverts = update_of(inst, iflat)
    iscene.set_triangles(iids, torch.from_numpy(iverts).cuda())
    iflat.set_triangles(iids, iverts)
    slot = iflat.instance_tree(0)["first_slot"]
    upd = {slot: [("translate", (0.6, 0.2, 0.1)), ("rotate_y", 33.0)]}
    iscene.set_transforms(upd)
    iflat.set_transforms(upd)
    _assert_arrays_equal(iscene, _device(_upload(iflat)), "set_transforms after set_triangles_device")


# ---- 5. refusals
def test_scene_refusals_enqueue_nothing(rtsr):
    import ctypes as C
    case = CASES["mixed"](rtsr, False)
    flat = case.flatten()
    scene = _upload(flat)
    cam, cfg, h = cam_cfg(rtsr, case)
    first, frame = _device(scene), scene.render(cam, cfg)
    n_ids = int(flat.array("triangle_id").view(np.int32).max()) + 1
    for name, ids, n, verts, word, host_only in refusals(n_ids):
        st = call_set_prims(rtsr, rtsr.lib.rtx_scene_set_triangles, scene.ptr, ids, n, verts, None)
        assert st == rtsr.RTX_EINVAL and "rtx_scene_set_triangles" in rtsr.last_error() and word in rtsr.last_error(), (name, rtsr.last_error())
    import torch
    good = torch.ones(18, dtype=torch.float64).cuda()
    two = (C.c_int32 * 2)(0, 1)
    dev = rtsr.lib.rtx_scene_set_triangles_device
    assert dev(scene.ptr, two, 2, C.c_void_p(good.data_ptr() + 4), None) == rtsr.RTX_EINVAL and "8-byte aligned" in rtsr.last_error()
    assert dev(scene.ptr, (C.c_int32 * 2)(0, n_ids), 2, C.c_void_p(good.data_ptr()), None) == rtsr.RTX_EINVAL and "out of range" in rtsr.last_error()
    assert dev(scene.ptr, (C.c_int32 * 2)(1, 1), 2, C.c_void_p(good.data_ptr()), None) == rtsr.RTX_EINVAL and "twice" in rtsr.last_error()
    assert dev(scene.ptr, two, 2, None, None) == rtsr.RTX_EINVAL and "NULL" in rtsr.last_error()
    assert dev(scene.ptr, two, 0, C.c_void_p(good.data_ptr()), None) == rtsr.RTX_OK
    back = _device(scene)
    assert all(np.array_equal(back[k], first[k]) for k in DEVICE_ARRAYS)
    _same_screen(scene.render(cam, cfg), frame, "after the refusals")
    # an f32 scene; a BVH that holds a MovingSphere
    ids, verts = update_of(case, flat)
    s32 = flat.upload(f32=True)
    f32_first = s32.render(cam, cfg)
    with pytest.raises(rtsr.RtxError) as e:
        s32.set_triangles(ids, verts)
    assert e.value.status == rtsr.RTX_EUNSUPPORTED and "rtx_flat_set_triangles" in str(e.value) and "rtx_scene_upload_f32" in str(e.value)
    _same_screen(s32.render(cam, cfg), f32_first, "f32 after the refusal")
    mv = movers(rtsr)
    mflat = mv.flatten()
    mscene = _upload(mflat)
    mfirst, mframe = _device(mscene), mscene.render(cam, cfg)
    with pytest.raises(rtsr.RtxError) as e:
        mscene.set_triangles(*update_of(mv, mflat))
    assert e.value.status == rtsr.RTX_EUNSUPPORTED and "MovingSphere" in str(e.value)
    mback = _device(mscene)
    assert all(np.array_equal(mback[k], mfirst[k]) for k in DEVICE_ARRAYS)
    _same_screen(mscene.render(cam, cfg), mframe, "movers after the refusal")
