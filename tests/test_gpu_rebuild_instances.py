"""Scene.rebuild_instance_trees and Scene.instance_tree_cost on the device (rtx_scene_rebuild_instance_trees: k_member_boxes,
k_member_morton, the radix sort, k_rebuild_radix, k_rebuild_emit; rtx_scene_instance_tree_cost: k_tree_cost_terms).

Two judges, neither the code under test: the resident ARRAYS after a rebuild are byte-equal to the host's RTX_REBUILD_MORTON of
the same flat scene (which tests/test_rebuild_instances_host.py audits in numpy and holds to a fresh flatten ray for ray), and
every ENTRY POINT on the rebuilt scene answers bit for bit as on a FRESH upload of the same world built at that pose.  The
stack budget and the cost are asserted BEFORE any walk is launched on a rebuilt tree: with a wrong budget a case fails there."""
import ctypes as C
import os

import numpy as np
import pytest

import cast_rays_cases as cc
import rebuild_cases as rc
from set_transforms_cases import build, random_values, updates_for

pytestmark = pytest.mark.gpu
DEVICE_ARRAYS = ("entries", "nodes", "nodes32", "motion32", "world_desc")
NAMES = sorted(rc.CASES)


def _device(scene):
    return {k: scene.array(k) for k in DEVICE_ARRAYS}


def _assert_arrays_equal_host(rtsr, orc, scene, flat, what):
    """f64: the resident arrays are the flat's.  f32: they are the product's converter run on the flat's (oracle f32_convert),
    and nodes32 is the flat's own."""
    if scene.is_f32:
        descs = dict(orc.f32_descs())
        for name, elem64 in (("entries", 160), ("nodes", 112)):
            want, _ = orc.f32_convert(descs[name], flat.array(name), elem64)
            dev = scene.array(name)
            assert want is not None and np.array_equal(dev, want), "%s: f32 %s differs from the converted host rebuild" % (what, name)
        names = ("nodes32", "motion32")
    else:
        names = ("entries", "nodes", "nodes32", "motion32")
    for k in names:
        dev, host = scene.array(k), flat.array(k)
        assert dev.size == host.size and np.array_equal(dev, host), "%s: %s differs from the host rebuild in %d bytes" % (what, k, int((dev != host).sum()))


def _with_kernel(env, fn):
    old = os.environ.get("RTX_TRACE_KERNEL")
    if env:
        os.environ["RTX_TRACE_KERNEL"] = env  # read once per upload
    try:
        return fn()
    finally:
        if env:
            if old is None:
                del os.environ["RTX_TRACE_KERNEL"]
            else:
                os.environ["RTX_TRACE_KERNEL"] = old


def _rebuilt_pair(rtsr, orc, name, f32=False, env=None):
    """(scene moved and rebuilt on the device, host flat moved and rebuilt with RTX_REBUILD_MORTON, fresh flat).  Arrays, stack
    budget and cost are asserted here, before anything walks the rebuilt tree."""
    fn, pose, trees = rc.CASES[name]
    b, w, calls = build(rtsr, fn)
    flat = b.flatten(w)
    values = pose(calls)
    bf, wf, _ = build(rtsr, fn, values)
    fresh = bf.flatten(wf)
    flat._keep = fresh._keep = (b, bf)
    scene = _with_kernel(env, lambda: flat.upload(f32=f32))
    assert scene.max_stack() == flat.info()["max_stack"]
    upd = updates_for(flat, calls, values)
    scene.set_transforms(upd)
    flat.set_transforms(upd)
    refitted_cost = scene.instance_tree_cost(0 if trees is None else trees[0])
    stats = scene.rebuild_instance_trees(trees)
    before = flat.info()["max_stack"]
    flat.rebuild_instance_trees(trees, builder="morton")
    n_trees = flat.instances()["n_trees"]
    rebuilt = list(range(n_trees)) if trees is None else trees
    assert stats == {"trees_rebuilt": len(rebuilt), "max_depth": max(flat.instance_tree(k)["depth"] for k in rebuilt),
                     "max_stack_before": before, "max_stack_after": flat.info()["max_stack"]}, stats
    assert scene.max_stack() == flat.info()["max_stack"]
    _assert_arrays_equal_host(rtsr, orc, scene, flat, "%s%s" % (name, " f32" if f32 else ""))
    if not f32:
        assert np.array_equal(scene.array("world_desc"), _with_kernel(env, lambda: flat.upload()).array("world_desc"))
        for k in range(n_trees):
            assert scene.instance_tree_cost(k) == flat.instance_tree_cost(k), k
    else:
        nodes_f32 = scene.array("nodes").view(rc.NODE_F32)  # the f32 scene's own planes, widened: the same sum in numpy
        for k in range(n_trees):
            assert scene.instance_tree_cost(k) == rc.tree_cost_of(nodes_f32, rc.instance_records(flat)[k][0]), k
    if name == "scramble":
        assert refitted_cost > scene.instance_tree_cost(0)
    return scene, flat, fresh


def _same_screen(a, b, what):
    bad = int((a.accum != b.accum).any(axis=2).sum())
    assert bad == 0 and np.array_equal(a.rgb8, b.rgb8), "%s: %d pixels differ from the fresh upload" % (what, bad)


def _same_hits(hm, hf, n):
    for col in ("t", "p", "normal", "uv", "ids"):
        assert cc.same_bits(getattr(hm, col).reshape(n, -1).astype(np.float64), getattr(hf, col).reshape(n, -1).astype(np.float64)).all(), col


@pytest.mark.parametrize("name", NAMES)
def test_rebuilt_f64_scene_equals_the_host_rebuild_and_the_fresh_upload(rtsr, orc, name):
    """Arrays, max_stack and cost first (in _rebuilt_pair); then the default kernel, light sampling, a progressive handle and its
    feature pass at 48 x 32 x 8 spp, 2000 cast rays and a trace_rays batch, all against a fresh upload of the pose."""
    scene, flat, fresh_flat = _rebuilt_pair(rtsr, orc, name)
    fresh = fresh_flat.upload()
    cam, cfg, h, lo, hi = rc.camera(rtsr, name)
    assert (cfg.image_width, h, cfg.samples_per_pixel) == (48, 32, 8)
    want = fresh.render(cam, cfg)
    assert want.accum.std() > 0.01
    _same_screen(scene.render(cam, cfg), want, "%s: rtx_render" % name)
    _same_screen(scene.render(cam, cfg, light_sampling=True), fresh.render(cam, cfg, light_sampling=True), "%s: light sampling" % name)
    pm, pf = scene.progressive(cam, cfg), fresh.progressive(cam, cfg)
    for p in (pm, pf):
        p.add(4)
        p.add(4)
    _same_screen(pm.screen(), pf.screen(), "%s: progressive" % name)
    _same_screen(pm.screen(), want, "%s: progressive against the one-shot render" % name)
    (am, nm), (af, nf) = pm.features(4), pf.features(4)
    assert af.std() > 0.01 and np.array_equal(am, af) and np.array_equal(nm, nf)
    o, d = cc.sphere_rays(2000, 7, lo, hi, 1.0)
    hm, hf = scene.cast_rays(o, d, seed=1, stream_step=1), fresh.cast_rays(o, d, seed=1, stream_step=1)
    assert hf.hit.sum() >= 300 and (~hf.hit).sum() >= 100
    _same_hits(hm, hf, len(o))
    rm = scene.trace_rays(o, d, spp=4, max_depth=12, background=(0.35, 0.4, 0.55), sumsq=True)
    rf = fresh.trace_rays(o, d, spp=4, max_depth=12, background=(0.35, 0.4, 0.55), sumsq=True)
    assert rf.sum.std() > 0.01 and cc.same_bits(rm.sum, rf.sum).all() and cc.same_bits(rm.sumsq, rf.sumsq).all()


@pytest.mark.parametrize("name", NAMES)
def test_rebuilt_scene_under_k_trace_simple(rtsr, orc, name):
    scene, _, fresh_flat = _rebuilt_pair(rtsr, orc, name, env="simple")
    fresh = _with_kernel("simple", lambda: fresh_flat.upload())
    cam, cfg, h, _, _ = rc.camera(rtsr, name)
    got = scene.render(cam, cfg, want_stats=True)
    assert rtsr.trace_kernel_name(got.stats.trace_kernel) == "k_trace_simple"
    _same_screen(got, fresh.render(cam, cfg), "%s: k_trace_simple" % name)


@pytest.mark.parametrize("name", NAMES)
def test_rebuilt_f32_scene_equals_the_host_rebuild_and_the_fresh_upload(rtsr, orc, name):
    """The f32 compilation: the same tree as the f64 scene's (topology comes from the f64 boxes), its planes narrowed; a render
    and a cast against a fresh f32 upload (the same kernels on both sides, so exact)."""
    scene, flat, fresh_flat = _rebuilt_pair(rtsr, orc, name, f32=True)
    fresh = fresh_flat.upload(f32=True)
    assert scene.is_f32 and fresh.is_f32
    cam, cfg, h, lo, hi = rc.camera(rtsr, name)
    _same_screen(scene.render(cam, cfg), fresh.render(cam, cfg), "%s f32" % name)
    o, d = cc.sphere_rays(2000, 7, lo, hi, 1.0)
    _same_hits(scene.cast_rays(o, d), fresh.cast_rays(o, d), len(o))


@pytest.mark.parametrize("f32", [False, True])
def test_rebuild_then_set_transforms_then_rebuild_twice(rtsr, orc, f32):
    """A third pose on the rebuilt tree: the arrays are the host's rebuild followed by the host's refit and the frame is the
    fresh upload's.  Then two rebuilds in a row: the second changes no byte."""
    name = "size_257"
    scene, flat, _ = _rebuilt_pair(rtsr, orc, name, f32=f32)
    fn = rc.CASES[name][0]
    _, _, calls = build(rtsr, fn)
    third = random_values(calls, seed=91, shift=3.0)
    upd = updates_for(flat, calls, third)
    scene.set_transforms(upd)
    flat.set_transforms(upd)
    _assert_arrays_equal_host(rtsr, orc, scene, flat, "refit after rebuild")
    bf, wf, _ = build(rtsr, fn, third)
    fresh = bf.flatten(wf).upload(f32=f32)
    cam, cfg, h, lo, hi = rc.camera(rtsr, name)
    _same_screen(scene.render(cam, cfg), fresh.render(cam, cfg), "refit after rebuild")
    scene.rebuild_instance_trees()
    once = _device(scene)
    flat.rebuild_instance_trees()
    _assert_arrays_equal_host(rtsr, orc, scene, flat, "second rebuild")
    stats = scene.rebuild_instance_trees([0])
    assert stats["max_stack_before"] == stats["max_stack_after"] == scene.max_stack()
    twice = _device(scene)
    assert all(np.array_equal(once[k], twice[k]) for k in DEVICE_ARRAYS)
    _same_screen(scene.render(cam, cfg), fresh.render(cam, cfg), "rebuilt twice")


def test_rebuild_and_cast_on_one_side_stream_without_a_host_wait(rtsr):
    import torch
    name = "size_257"
    fn, pose, _ = rc.CASES[name]
    b, w, calls = build(rtsr, fn)
    flat = b.flatten(w)
    values = pose(calls)
    bf, wf, _ = build(rtsr, fn, values)
    fresh = bf.flatten(wf).upload()
    scene = flat.upload()
    _, _, _, lo, hi = rc.camera(rtsr, name)
    o, d = cc.sphere_rays(2000, 3, lo, hi, 1.0)
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        scene.set_transforms(updates_for(flat, calls, values), stream=side)
        scene.rebuild_instance_trees(stream=side)  # waits on `side` itself, once; the test adds no wait
        got = scene.cast_rays(to, td)
    side.synchronize()
    want = fresh.cast_rays(o, d)
    assert want.hit.sum() >= 300 and (~want.hit).sum() >= 100
    assert cc.same_bits(got.t.cpu().numpy().reshape(-1, 1), want.t.reshape(-1, 1)).all()
    assert np.array_equal(got.ids.cpu().numpy(), want.ids) and cc.same_bits(got.p.cpu().numpy(), want.p).all()


def test_scene_refusals_leave_every_array_unchanged(rtsr):
    b, w = rc.CASES["two_trees"][0](rtsr)[:2]
    flat = b.flatten(w)
    scene = flat.upload()
    first, stack = _device(scene), scene.max_stack()
    fn = rtsr.lib.rtx_scene_rebuild_instance_trees
    I = lambda *v: (C.c_int32 * len(v))(*v)
    dirty = rtsr.RtxRebuildStats()
    dirty.reserved[0] = 5
    for what, args, word in (("negative n", (scene.ptr, I(0), -1, None, None), "n < 0"), ("index past the trees", (scene.ptr, I(0, 2), 2, None, None), "trees[1]"),
                             ("negative index", (scene.ptr, I(-1), 1, None, None), "trees[0]"), ("named twice", (scene.ptr, I(1, 0, 1), 3, None, None), "twice"),
                             ("reserved word", (scene.ptr, I(0), 1, None, C.byref(dirty)), "reserved[0]"), ("NULL scene", (None, I(0), 1, None, None), "NULL")):
        assert fn(*args) == rtsr.RTX_EINVAL, what
        assert "rtx_scene_rebuild_instance_trees" in rtsr.last_error() and word in rtsr.last_error(), (what, rtsr.last_error())
    cost = C.c_double(0.0)
    assert rtsr.lib.rtx_scene_instance_tree_cost(scene.ptr, 2, C.byref(cost)) == rtsr.RTX_EINVAL and "k is out of range" in rtsr.last_error()
    assert fn(scene.ptr, I(0), 0, None, None) == rtsr.RTX_OK  # n = 0 with a list: nothing to do
    back = _device(scene)
    assert all(np.array_equal(back[k], first[k]) for k in DEVICE_ARRAYS) and scene.max_stack() == stack
    # a chain of 63 nodes: refused after the build into scratch, the resident tree untouched and still rendering the pose
    deep_flat, calls, values, _, fresh_flat = rc.posed(rtsr, "chain63")
    deep = deep_flat.upload()
    d0, s0 = _device(deep), deep.max_stack()
    assert fn(deep.ptr, None, 0, None, None) == rtsr.RTX_EUNSUPPORTED and "walk stack" in rtsr.last_error()
    d1 = _device(deep)
    assert all(np.array_equal(d0[k], d1[k]) for k in DEVICE_ARRAYS) and deep.max_stack() == s0
    cam, cfg, h, _, _ = rc.camera(rtsr, "line")
    _same_screen(deep.render(cam, cfg), fresh_flat.upload().render(cam, cfg), "after a refused rebuild")
    # a scene without instance trees and NULL: nothing to do
    from instance_scenes import box_field
    bh, wh = box_field(rtsr, "hoisted")
    hoisted = bh.flatten(wh).upload()
    assert hoisted.rebuild_instance_trees()["trees_rebuilt"] == 0
