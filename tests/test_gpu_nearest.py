"""Nearest-point queries on the device (Scene.nearest, rtx_scene_nearest*): k_nearest answers what the CPU core answers.

Every comparison with the judge (tests/nearest_host_check.cpp: host_nearest, the culled walk world_nearest<F_ALL>, itself held to
the exhaustive scan and to closed forms by tests/test_nearest_cases.py) is by bit pattern with NaN equal to NaN.  Scenes and
points: tests/nearest_cases.py (at most 2000 points per scene); a case's scene is uploaded once per precision and shared."""
import numpy as np
import pytest

import nearest_cases as nc

pytestmark = pytest.mark.gpu
PRECISIONS = pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
_SCENES = {}


@pytest.fixture(scope="module")
def chk(rtsr, orc, tmp_path_factory):
    return nc.checkers(tmp_path_factory)


def _scene(c, f32):
    key = (c.name, f32)
    if key not in _SCENES:
        _SCENES[key] = c.flat.upload(f32=f32)
    return _SCENES[key]


def _assert_same(name, got, ref):
    bad = nc.differing(got, ref)
    print("%s: %d points, %d found, %d differ from the judge" % (name, len(ref.d), int(ref.found.sum()), len(bad)))
    assert len(bad) == 0, "%s: point %d: device d %r q %r ids %r, judge d %r q %r ids %r" % (
        name, bad[0], got.d[bad[0]], got.q[bad[0]], got.ids[bad[0]], ref.d[bad[0]], ref.q[bad[0]], ref.ids[bad[0]])


# ---- 1. bit for bit against the judge: P_INST (the zoos), P_ANY (the rest), both precisions, media on and off, r_max infinite
# and as a per-point column
@PRECISIONS
@pytest.mark.parametrize("name", list(nc.SCENES))
def test_nearest_equals_the_judge(rtsr, chk, name, f32):
    c = nc.case(rtsr, name)
    assert len(c.points) <= 2000
    scene = _scene(c, f32)
    assert scene.is_f32 == f32
    ref = nc.host(chk, c.flat, c.points, c.time, media=True, f32=f32)
    got = scene.nearest(c.points, c.time, media=True)
    _assert_same(name + " media", got, ref)
    assert got.n == len(c.points) and np.array_equal(got.found, ref.found)
    r_col = np.ascontiguousarray(np.where(np.arange(len(c.points)) % 2 == 0, nc.finite_r_max(ref), ref.d))  # half of them exactly at d
    ref = nc.host(chk, c.flat, c.points, c.time, r_col, f32=f32)
    _assert_same(name + " r_max column", scene.nearest(c.points, c.time, r_col), ref)
    assert 0 < int(ref.found.sum()) < len(c.points) or name.startswith("tie")


@PRECISIONS
def test_closed_form_scenes_equal_the_judge(rtsr, chk, f32):
    for c in nc.closed_form_cases(rtsr, f32):
        got = c.flat.upload(f32=f32).nearest(c.points, c.time, c.r_max, media=c.media)
        _assert_same(c.name, got, nc.host(chk, c.flat, c.points, c.time, c.r_max, media=c.media, f32=f32))
        ed, eq, tol = nc.check_closed(c, got, f32)
        assert ed <= tol and eq <= tol, (c.name, ed, eq, tol)


@pytest.mark.parametrize("K,levels", [(12, 45), (16, 55)])  # tests/test_gpu_lbvh_edges.py: MIN_LEVELS
def test_deep_chains_of_the_gpu_builder(rtsr, chk, K, levels):
    """tests/lbvh_cases.py's chains, built on the device: trees of about 49 and 61 levels, the deepest stacks the LDS walk is given."""
    c = nc.case(rtsr, "chain_%d" % K)
    flat = c.builder.flatten(c.world, max_leaf=1, gpu_builder=True)
    assert flat.info()["max_stack"] + 1 >= levels, flat.info()["max_stack"]
    ref = nc.host(chk, flat, c.points)
    assert len(nc.differing(ref, nc.host(chk, flat, c.points, exhaustive=True))) == 0
    _assert_same("chain_%d, GPU-built" % K, flat.upload().nearest(c.points), ref)


# ---- 2. what is refused
def test_gravity_scenes_are_unsupported(rtsr):
    b = rtsr.Builder(1)
    world, _, _ = b.get_world_cam(rtsr.SCENE_RANDOM_MOVING)
    for f32 in (False, True):
        scene = b.flatten(world).upload(f32=f32)
        with pytest.raises(rtsr.RtxError) as e:
            scene.nearest(np.zeros((4, 3)))
        assert e.value.status == rtsr.RTX_EUNSUPPORTED and "GravitySphere" in str(e.value)


# ---- 3. batch shapes
def test_batch_shapes(rtsr, chk):
    import torch
    c = nc.case(rtsr, "slot_list")
    scene = _scene(c, False)
    rng = np.random.default_rng(77)
    for n in (1, 63, 64, 65, 257):
        p = np.ascontiguousarray(rng.uniform(-4.0, 31.0, (n, 3)))
        _assert_same("n = %d" % n, scene.nearest(p), nc.host(chk, c.flat, p))
    assert scene.nearest(np.zeros((0, 3))).n == 0
    # one grid pass (8 blocks a CU) plus one point: the grid-stride loop's second trip, and two host staging slices
    n = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 + 1
    assert n > 262144  # RTX_CAST_HOST_SLICE
    p = np.ascontiguousarray(rng.uniform(-4.0, 31.0, (n, 3)))
    r = np.ascontiguousarray(rng.uniform(0.5, 6.0, n))
    got = scene.nearest(p, None, r)
    for part in (slice(0, 1500), slice(n - 1500, n)):
        ref = nc.host(chk, c.flat, p[part], None, r[part])
        _assert_same("grid pass + 1, %r" % (part,), nc.Answer(got.d[part], got.q[part], got.ids[part]), ref)
    # a split batch equals the whole
    cut = 262144 + 77
    a, b2 = scene.nearest(p[:cut], None, r[:cut]), scene.nearest(np.ascontiguousarray(p[cut:]), None, np.ascontiguousarray(r[cut:]))
    assert np.array_equal(np.concatenate([a.d, b2.d]), got.d) and np.array_equal(np.concatenate([a.q, b2.q]), got.q)
    assert np.array_equal(np.concatenate([a.ids, b2.ids]), got.ids)


def test_want_subsets_torch_tensors_and_streams(rtsr, chk):
    import torch
    c = nc.case(rtsr, "zoo_middle")
    scene = _scene(c, False)
    full = scene.nearest(c.points, c.time)
    for want in (("d",), ("q",), ("ids",), ("d", "ids"), ("q", "ids"), ()):
        got = scene.nearest(c.points, c.time, want=want)
        for name in rtsr.NEAREST_COLUMNS:
            col = getattr(got, name)
            assert (col is None) == (name not in want), (want, name)
            if col is not None:
                assert np.array_equal(col, getattr(full, name)), (want, name)
    # the device entry writes only the columns it is given: the others keep their sentinel
    import ctypes as C
    n = len(c.points)
    pts = torch.from_numpy(c.points).cuda()
    d, q, ids = torch.full((n,), 7.0, dtype=torch.float64, device="cuda"), torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda"), \
        torch.full((n, 4), 7, dtype=torch.int32, device="cuda")
    batch = rtsr.RtxPointBatch()
    rtsr.lib.rtx_point_batch_defaults(C.byref(batch))
    batch.n, batch.points = n, pts.data_ptr()
    out = rtsr.RtxNearest(d.data_ptr(), None, None)
    assert rtsr.lib.rtx_scene_nearest_device(scene.ptr, C.byref(batch), C.byref(out), None) == rtsr.RTX_OK
    torch.cuda.synchronize()
    assert bool((q == 7.0).all()) and bool((ids == 7).all())
    assert np.array_equal(d.cpu().numpy(), scene.nearest(c.points, want=("d",)).d)
    # torch tensors on the device equal numpy on the host, on the current stream and on one of the caller's
    t = None if c.time is None else torch.from_numpy(c.time).cuda()
    on_dev = scene.nearest(pts, t)
    torch.cuda.synchronize()
    assert on_dev.d.is_cuda and on_dev.ids.dtype == torch.int32
    ref = scene.nearest(c.points, c.time)
    for name in rtsr.NEAREST_COLUMNS:
        assert np.array_equal(getattr(on_dev, name).cpu().numpy(), getattr(ref, name)), name
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = scene.nearest(pts, t, stream=side)
    side.synchronize()
    for name in rtsr.NEAREST_COLUMNS:
        assert np.array_equal(getattr(on_side, name).cpu().numpy(), getattr(ref, name)), name


# ---- 4. after updates of a resident scene: the refitted boxes still hold their primitives
def _update_world(rtsr):
    b = rtsr.Builder(5)
    grey, red = b.lambertian((0.5, 0.5, 0.5)), b.metal((0.8, 0.3, 0.3), 0.1)
    rng = np.random.default_rng(8)
    balls = b.bvh_from_list(b.hittable_list([b.sphere(tuple(rng.uniform(-3.0, 3.0, 3)), float(rng.uniform(0.1, 0.4)), red) for _ in range(80)]), 0.0, 1.0)
    verts = rng.uniform(-1.0, 1.0, (60, 3)) + (6.0, 1.0, 0.0)
    faces = [(k, k + 1, k + 2) for k in range(0, 57)]
    mesh = b.bvh_from_list(b.triangle_mesh(verts, faces, grey), 0.0, 1.0)
    members = [b.translate((2.0 * k - 5.0, 0.0, -6.0), b.rotate_y(11.0 * k, b.rect_prism((-0.4, 0.0, -0.4), (0.4, 0.9, 0.4), grey))) for k in range(6)]
    world = b.hittable_list([b.xz_rect(-20.0, 20.0, -20.0, 20.0, -2.0, grey), b.instance_bvh(b.hittable_list(members)), balls, mesh])
    return b, world, balls, mesh


def test_after_updates_of_a_resident_scene(rtsr, chk):
    b, world, balls, mesh = _update_world(rtsr)
    flat = b.flatten(world)
    scene = flat.upload()
    rng = np.random.default_rng(9)
    p = np.ascontiguousarray(rng.uniform(-9.0, 9.0, (1500, 3)) * (1.0, 0.4, 1.0))
    _assert_same("before", scene.nearest(p), nc.host(chk, flat, p))
    slots = [s for s in range(flat.info()["n_top_level"]) if flat.slot_chain(s) == ["translate", "rotate_y"]]
    assert len(slots) == 6
    upd = {s: [("translate", (float(rng.uniform(-7, 7)), float(rng.uniform(-1, 2)), float(rng.uniform(-7, 7)))), ("rotate_y", float(rng.uniform(0, 360)))] for s in slots}
    scene.set_transforms(upd)
    flat.set_transforms(upd)
    moved = nc.host(chk, flat, p)
    _assert_same("set_transforms", scene.nearest(p), moved)
    ids = flat.sphere_ids(b, balls)
    vals = np.column_stack([rng.uniform(-6.0, 6.0, (len(ids), 3)), rng.uniform(0.05, 0.8, len(ids))])
    scene.set_spheres(ids, vals)
    flat.set_spheres(ids, vals)
    _assert_same("set_spheres", scene.nearest(p), nc.host(chk, flat, p))
    tids = flat.triangle_ids(b, mesh)
    tv = rng.uniform(-2.0, 2.0, (len(tids), 9)) + np.tile((-4.0, 1.0, 5.0), 3)
    scene.set_triangles(tids, tv)
    flat.set_triangles(tids, tv)
    after = nc.host(chk, flat, p)
    _assert_same("set_triangles", scene.nearest(p), after)
    assert len(nc.differing(after, nc.host(chk, flat, p, exhaustive=True))) == 0  # the refitted boxes still hold their primitives
    assert len(nc.differing(after, moved)) > 0 and {0, 2, 3} <= set(after.ids[:, 2].tolist())


# ---- 5. beside a render
def test_a_query_between_two_renders_leaves_the_frames_alone(rtsr, chk):
    import torch
    c = nc.case(rtsr, "zoo_middle")
    from instance_scenes import zoo_cam_cfg
    cam, cfg, _ = zoo_cam_cfg(rtsr, width=32, spp=2, depth=6)
    scene = c.flat.upload()
    first = scene.render(cam, cfg)
    pts = torch.from_numpy(c.points).cuda()
    got = scene.nearest(pts)   # enqueued, not waited for
    second = scene.render(cam, cfg)
    torch.cuda.synchronize()
    ref = nc.host(chk, c.flat, c.points)
    _assert_same("between renders", nc.Answer(got.d.cpu().numpy(), got.q.cpu().numpy(), got.ids.cpu().numpy()), ref)
    plain = c.flat.upload()
    for frame in (first, second):
        again = plain.render(cam, cfg)
        assert np.array_equal(np.asarray(frame.accum), np.asarray(again.accum)) and bytes(frame.rgb8) == bytes(again.rgb8)
