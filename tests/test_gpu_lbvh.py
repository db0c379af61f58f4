"""The GPU BVH builder (csrc/hip/lbvh.hip, RtxBuildOptions.gpu_builder): replaces BvhNode::new (bvh.rs:14-83) at mesh scale.

A BVH is a culling structure: the closest hit (with its tie rule) does not depend on its topology, so an image traced
through a GPU-built tree must equal, bit for bit, the image traced through the host SAH tree and the CPU oracle's."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _room(rtsr, triangles, **flat_kw):
    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(rtsr.SCENE_STANFORD_DRAGON, mesh_triangles=triangles)
    return b, world, cam, bg, b.flatten(world, **flat_kw)


@pytest.mark.parametrize("triangles,max_leaf", [(20000, 0), (20000, 1), (50000, 4), (3000, 8)])
def test_gpu_built_tree_gives_the_same_image(rtsr, orc, triangles, max_leaf):
    b, world, cam, bg, flat_host = _room(rtsr, triangles, max_leaf=max_leaf)
    cfg = rtsr.Config.new(16.0 / 9.0, 128, 4, 50, 10, seed=5, background=bg)
    h = rtsr.image_height(cfg)
    host = flat_host.upload().render(cam, cfg)
    flat_gpu = b.flatten(world, max_leaf=max_leaf, gpu_builder=True)
    info_h, info_g = flat_host.info(), flat_gpu.info()
    assert info_g["n_triangles"] == info_h["n_triangles"] and info_g["n_bvh"] == 1
    assert info_g["bvh_device_ms"] > 0.0 and info_h["bvh_device_ms"] == 0.0
    gpu = flat_gpu.upload().render(cam, cfg)
    assert np.array_equal(gpu.accum, host.accum), "%d pixels differ" % int((np.abs(gpu.accum - host.accum).max(axis=2) > 0).sum())
    assert np.array_equal(gpu.rgb8, host.rgb8)
    # the CPU oracle walking the GPU-built tree (f64 boxes, serial walk) agrees too: the tree is well formed
    ref, ref8 = orc.o2_render(flat_gpu.arrays_ptr(), cam, cfg, h, threads=16)
    assert np.array_equal(gpu.accum, ref) and np.array_equal(gpu.rgb8, ref8)
    # and the literal object-graph oracle (the reference's own builder rule) on a few rows
    a1, r1 = orc.o1_render(b.graph_ptr(), world, cam, cfg, h, threads=16)
    assert np.array_equal(gpu.accum, a1)


def test_every_walker_through_a_gpu_built_tree(rtsr, monkeypatch):
    b, world, cam, bg, flat_host = _room(rtsr, 30000)
    cfg = rtsr.Config.new(16.0 / 9.0, 96, 4, 50, 10, seed=6, background=bg)
    expect = flat_host.upload().render(cam, cfg)
    flat_gpu = b.flatten(world, gpu_builder=True)
    for env in ({}, {"RTX_WIDE": "0"}, {"RTX_WIDE": "1"}, {"RTX_TRACE_KERNEL": "simple"}, {"RTX_TRACE_KERNEL": "world"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = flat_gpu.upload().render(cam, cfg)
        assert np.array_equal(got.accum, expect.accum), env
        for k in env:
            monkeypatch.delenv(k)


def test_sphere_world_and_small_bvhs(rtsr, orc):
    """Book-2's two BVHs (2400 rectangles, 1000 spheres: above the 1024-primitive threshold) on the GPU builder; Book-1's
    485 spheres stay with the host builder (below the threshold) -- both must still render the oracle's image."""
    for sid, width, aspect in ((rtsr.SCENE_BOOK2_FINAL, 80, 1.0), (rtsr.SCENE_BOOK1_CANONICAL, 96, 1.5)):
        b = rtsr.Builder(1)
        world, cam, bg = b.get_world_cam(sid)
        cfg = rtsr.Config.new(aspect, width, 4, 50, 10, seed=3, background=bg)
        h = rtsr.image_height(cfg)
        flat = b.flatten(world, gpu_builder=True)
        screen = flat.upload().render(cam, cfg)
        a1, r1 = orc.o1_render(b.graph_ptr(), world, cam, cfg, h, threads=16)
        assert np.array_equal(screen.accum, a1) and np.array_equal(screen.rgb8, r1)
        assert (flat.info()["bvh_device_ms"] > 0.0) == (sid == rtsr.SCENE_BOOK2_FINAL)


def test_ply_mesh_through_the_gpu_builder(rtsr, orc, tmp_path):
    from test_gpu_compat import _write_ply
    n = 40
    verts, faces = [], []
    for i in range(n + 1):
        for j in range(n + 1):
            x, z = i / n * 2 - 1, j / n * 2 - 1
            verts.append((np.float32(x), np.float32(0.25 * np.sin(4 * x) * np.cos(3 * z)), np.float32(z)))
    for i in range(n):
        for j in range(n):
            a, bb, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
            faces += [(a, bb, c), (a, c, d)]
    path = str(tmp_path / "wave.ply")
    _write_ply(path, verts, faces, binary=True)
    b = rtsr.Builder(1)
    model = b.triangle_model(path, 3.0)  # TriangleModel::load_from_file(path, 3.0).to_hittable()  (model.rs:13-76)
    world = b.hittable_list([b.bvh_from_list(model, 0.0, 1.0), b.xz_rect(-2, 2, -2, 2, 4.0, b.diffuse_light((4.0, 4.0, 4.0)))])
    cam = rtsr.Camera.new((0.0, 4.0, 7.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0, 1.5, 0.0, 7.0, 0.0, 1.0)
    cfg = rtsr.Config.new(1.5, 96, 4, 12, 4, seed=8, background=(0.5, 0.6, 0.8))
    h = rtsr.image_height(cfg)
    flat = b.flatten(world, gpu_builder=True)
    assert flat.info()["n_triangles"] == 2 * n * n and flat.info()["bvh_device_ms"] > 0.0
    screen = flat.upload().render(cam, cfg)
    a1, r1 = orc.o1_render(b.graph_ptr(), world, cam, cfg, h, threads=8)
    assert np.array_equal(screen.accum, a1) and np.array_equal(screen.rgb8, r1)


def test_full_size_mesh_build_time(rtsr, orc):
    """871 200 triangles (BASELINE configs[3]): the device part of the build under 100 ms; the tree passes the exact audit and is the
    same bytes in two builds; spot rows of the 1920x1080 frame traced through the GPU-built tree equal the oracle's."""
    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(rtsr.SCENE_STANFORD_DRAGON, mesh_triangles=871200)
    first = b.flatten(world, gpu_builder=True)  # first call pays one-time costs (code object load, rocPRIM kernel selection)
    t0 = time.perf_counter()
    flat = b.flatten(world, gpu_builder=True)
    wall = time.perf_counter() - t0
    info = flat.info()
    assert info["n_triangles"] == 871200
    # the one build that spreads k_refit over the whole device: every box bit-equal to the union of the triangles under it, leaves
    # in order and full (two triangles each), the reported depth exact, and the two builds the same bytes
    rc, depth = orc.audit_flat_exact(flat.arrays_ptr(), leaf_order=True, full_leaves=2)
    assert rc == 0, "exact audit code %d" % rc
    assert depth == info["max_stack"] + 1
    assert np.array_equal(orc.flat_array(first.arrays_ptr(), "nodes")[0], orc.flat_array(flat.arrays_ptr(), "nodes")[0])
    del first
    print("\n[lbvh] 871200 triangles: device %.1f ms, builder wall %.1f ms, whole flatten %.0f ms, depth %d" % (
        info["bvh_device_ms"], info["bvh_build_ms"], wall * 1e3, info["max_stack"]))
    assert info["bvh_device_ms"] < 100.0
    cfg = rtsr.Config.new(16.0 / 9.0, 1920, 2, 50, 10, seed=1, background=bg)
    h = rtsr.image_height(cfg)
    full = flat.upload().render(cam, cfg)
    import importlib
    rdist = importlib.import_module("ray-tracing-series-rust_amd.dist")
    shard = (5, 181, 1)
    rows = rdist.shard_row_indices(h, shard)
    ref, ref8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, shard=shard, threads=32)
    assert np.array_equal(full.accum[rows], ref) and np.array_equal(full.rgb8[rows], ref8)
