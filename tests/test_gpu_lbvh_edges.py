"""The GPU BVH builder (csrc/hip/lbvh.hip) on the inputs of tests/lbvh_cases.py, judged by the oracle's exact audit
(oracle_audit_flat_exact: every child box bit-equal to the union of the reference boxes below it, leaves in order and full),
by frames that must equal the host-built tree's and the CPU oracles' bit for bit through every walker, and by rays aimed at
every primitive.  The scenes themselves are proven on the CPU in tests/test_lbvh_cases.py.  Tall trees come last: 49 levels
(everything fits), 67 (refused: RTX_EUNSUPPORTED), and 61, where each kernel either renders the oracle's frame or refuses."""
import numpy as np
import pytest

import lbvh_cases

pytestmark = pytest.mark.gpu

WALKERS = ({}, {"RTX_WIDE": "0"}, {"RTX_WIDE": "1"}, {"RTX_TRACE_KERNEL": "simple"}, {"RTX_TRACE_KERNEL": "world"},
           {"RTX_TRACE_KERNEL": "wavefront"})
TALL = ("chain_16", "chain_18")  # their own tests, at the end of the file
MIN_LEVELS = {"chain_12": 45, "chain_16": 55, "chain_18": 65}  # below the CPU restatement's 49 / 61 / 67: see DESIGN.md
PAIRS = [(c, leaf) for c, (_, _, leafs) in lbvh_cases.CASES.items() for leaf in leafs]
_built = {}


class Built:
    """One case at one leaf size: the scene, its host-built and GPU-built flat scenes, the host tree's frame on the device."""

    def __init__(self, rtsr, case_id, leaf):
        self.b, self.world, self.cam, self.cfg, self.probes = lbvh_cases.build(rtsr, case_id)
        self.h = rtsr.image_height(self.cfg)
        self.leaf = leaf
        self.flat_host = self.b.flatten(self.world, max_leaf=leaf)
        self.flat_gpu = self.b.flatten(self.world, max_leaf=leaf, gpu_builder=True)
        self.levels = self.flat_gpu.info()["max_stack"] + 1
        self._host_frame = None

    def host_frame(self):
        if self._host_frame is None:
            self._host_frame = self.flat_host.upload().render(self.cam, self.cfg)
        return self._host_frame


def _get(rtsr, case_id, leaf):
    if (case_id, leaf) not in _built:
        _built[(case_id, leaf)] = Built(rtsr, case_id, leaf)
    return _built[(case_id, leaf)]


def _diff(a, b):
    return "%d pixels differ" % int((np.abs(a - b).max(axis=2) > 0).sum())


@pytest.mark.parametrize("case_id,leaf", PAIRS, ids=["%s-leaf%d" % p for p in PAIRS])
def test_gpu_tree_passes_the_exact_audit(rtsr, orc, case_id, leaf):
    s = _get(rtsr, case_id, leaf)
    info, ptr = s.flat_gpu.info(), s.flat_gpu.arrays_ptr()
    n = info["n_refs"]
    on_device = n >= 1024  # flatten.cpp: smaller BVHs stay with the host builder
    assert (info["bvh_device_ms"] > 0.0) == on_device and s.flat_host.info()["bvh_device_ms"] == 0.0
    assert on_device == (case_id != "threshold_1023") and info["n_bvh"] == 1
    if on_device:
        rc, depth = orc.audit_flat_exact(ptr, leaf_order=True, full_leaves=leaf)
    else:
        rc, depth = orc.audit_flat_exact(ptr, ask_first=True)
    print("\n[lbvh edges] %s max_leaf %d: %d primitives, %d nodes, %d stack levels, audit %d" % (case_id, leaf, n, info["n_nodes"], s.levels, rc))
    assert rc == 0, "exact audit code %d" % rc
    if on_device:
        assert depth == info["max_stack"] + 1  # the builder's report is exact, not a bound
        nodes = orc.flat_nodes(ptr)
        codes = nodes["child"][nodes["child"] < 0].astype(np.int64) & 0x7fffffff
        last = codes[(codes >> 3) + (codes & 7) + 1 == n]
        assert len(last) == 1 and (int(last[0]) & 7) + 1 == (n % leaf or leaf)  # 1025 at max_leaf 8: a last leaf of ONE primitive
        assert len(codes) == (n + leaf - 1) // leaf
    assert depth <= info["max_stack"] + 1 and s.levels >= MIN_LEVELS.get(case_id, 0)
    again = s.b.flatten(s.world, max_leaf=leaf, gpu_builder=True)
    for name in ("nodes", "refs", "triangles"):
        assert np.array_equal(orc.flat_array(ptr, name)[0], orc.flat_array(again.arrays_ptr(), name)[0]), name
    if case_id == "movers":
        rc, checked = orc.audit_motion(ptr, 32)
        assert rc == 0 and checked > 0
    if case_id == "coincident_tris":
        assert info["n_triangles"] == 2 * n - 100  # the non-exclusive relocation path: 1300 triangles, and a private copy of 1400


@pytest.mark.parametrize("case_id,leaf", [p for p in PAIRS if p[0] not in TALL], ids=["%s-leaf%d" % p for p in PAIRS if p[0] not in TALL])
def test_gpu_tree_gives_the_same_image(rtsr, orc, monkeypatch, case_id, leaf):
    s = _get(rtsr, case_id, leaf)
    scene = s.flat_gpu.upload()
    gpu = scene.render(s.cam, s.cfg, want_stats=True)
    kernel = rtsr.trace_kernel_name(gpu.stats.trace_kernel)
    print("\n[lbvh edges] %s max_leaf %d: %d stack levels, kernel %s" % (case_id, leaf, s.levels, kernel))
    assert len(np.unique(gpu.accum.reshape(-1, 3), axis=0)) >= 5
    # the CPU oracle walking the GPU-built tree
    ref, ref8 = orc.o2_render(s.flat_gpu.arrays_ptr(), s.cam, s.cfg, s.h, threads=16)
    print("[lbvh edges] %s max_leaf %d: against o2_render on the GPU-built tree: %s; against the host-built tree's frame: %s" % (
        case_id, leaf, _diff(gpu.accum, ref), _diff(gpu.accum, s.host_frame().accum)))
    assert np.array_equal(gpu.accum, ref), _diff(gpu.accum, ref)
    assert np.array_equal(gpu.rgb8, ref8)
    # the host-built tree's frame
    host = s.host_frame()
    assert np.array_equal(gpu.accum, host.accum), _diff(gpu.accum, host.accum)
    assert np.array_equal(gpu.rgb8, host.rgb8)
    # the literal object graph; for the coincident triangles and the hollow shells (whose inner spheres the reference's BvhNode
    # reaches or not by the luck of its random axes: tests/test_lbvh_cases.py) the graph of the LIST spelling, which has one answer
    if case_id in ("same_centroid", "coplanar"):
        a1, r1 = orc.o1_render(s.b.graph_ptr(), s.world, s.cam, s.cfg, s.h, threads=16)
        assert np.array_equal(gpu.accum, a1), _diff(gpu.accum, a1)
    if case_id in ("coincident_tris", "hollow_shells"):
        b2, listed = lbvh_cases.CASES[case_id][0](rtsr, as_list=True)[:2]
        a1, r1 = orc.o1_render(b2.graph_ptr(), listed, s.cam, s.cfg, s.h, threads=16)
        assert np.array_equal(gpu.accum, a1), _diff(gpu.accum, a1)
    if case_id == "movers":
        if kernel != "k_trace_lds":
            print("[lbvh edges] movers max_leaf %d: the plan did not admit k_trace_lds; %s rendered the frame" % (leaf, kernel))
        monkeypatch.setenv("RTX_MOTION", "0")
        plain = s.flat_gpu.upload().render(s.cam, s.cfg)
        assert np.array_equal(gpu.accum, plain.accum), _diff(gpu.accum, plain.accum)


@pytest.mark.parametrize("case_id,leaf", [("same_centroid", 1), ("coincident_tris", 2), ("odd_cluster", 8), ("chain_12", 1)])
def test_every_walker_through_the_edge_trees(rtsr, monkeypatch, case_id, leaf):
    s = _get(rtsr, case_id, leaf)
    assert s.levels >= MIN_LEVELS.get(case_id, 0)  # chain_12: 45 levels at the least, or the walkers prove nothing about height
    expect = s.host_frame()
    for env in WALKERS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = s.flat_gpu.upload().render(s.cam, s.cfg)
        assert np.array_equal(got.accum, expect.accum), (env, _diff(got.accum, expect.accum))
        for k in env:
            monkeypatch.delenv(k)


def _aimed_rays(s):
    """From two points outside the scene, a ray at every probe and at 256 points scattered about the probes."""
    rng = np.random.default_rng(5)
    targets = np.unique(s.probes, axis=0)
    near = targets[rng.integers(0, len(targets), 256)] + 0.6 * (rng.random((256, 3)) - 0.5)
    targets = np.concatenate([targets, near])
    origins = np.array([[0.37, 7.3, 15.1], [-11.2, 4.9, -9.4]])
    o = np.repeat(origins, len(targets), axis=0)
    d = np.concatenate([targets - origins[0], targets - origins[1]])
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def _check_cast(rtsr, orc, s, case_id):
    o, d = _aimed_rays(s)
    times = np.full(len(o), 0.45)
    hits = s.flat_gpu.upload().cast_rays(o, d, times)
    # the host-built tree answers for the oracle: a box too small in the GPU-built tree cannot hide there as well
    judge = s.flat_host
    n_hit = 0
    for r in range(len(o)):
        rec = orc.core_world_hit_mat(judge.arrays_ptr(), o[r], d[r], time=0.45)
        if rec is None:
            assert hits.ids[r, 0] == 0 and np.isinf(hits.t[r]), r
            continue
        n_hit += 1
        assert hits.ids[r, 0] == 1 and hits.t[r] == rec["t"], (r, hits.t[r], rec["t"])
        assert tuple(hits.normal[r]) == rec["normal"] and hits.ids[r, 3] == int(rec["front_face"]), r
        assert hits.ids[r, 1] == rec["mat"], (r, hits.ids[r], rec["mat"])  # which of the tied primitives was taken
    assert 4 * n_hit >= len(o), (n_hit, len(o))


@pytest.mark.parametrize("case_id,leaf", [p for p in PAIRS if p[0] not in TALL], ids=["%s-leaf%d" % p for p in PAIRS if p[0] not in TALL])
def test_rays_aimed_at_every_primitive(rtsr, orc, case_id, leaf):
    _check_cast(rtsr, orc, _get(rtsr, case_id, leaf), case_id)


def _too_deep(rtsr, call):
    with pytest.raises(rtsr.RtxError) as e:
        call()
    assert e.value.status == rtsr.RTX_EUNSUPPORTED and "too deep" in str(e.value), str(e.value)


def test_a_tree_of_67_levels_is_refused_cleanly(rtsr, orc):
    """chain(18): taller than the 64 levels of LDS stack a block has.  Flatten and upload succeed; every entry that would walk
    the tree says RTX_EUNSUPPORTED, "too deep", and leaves nothing behind: a Book-1 frame rendered next equals its oracle."""
    s = _get(rtsr, "chain_18", 1)
    print("\n[lbvh edges] chain_18: %d stack levels" % s.levels)
    assert s.levels >= MIN_LEVELS["chain_18"]
    scene = s.flat_gpu.upload()
    o, d = _aimed_rays(s)
    _too_deep(rtsr, lambda: scene.render(s.cam, s.cfg))
    _too_deep(rtsr, lambda: scene.render_count(s.cam, s.cfg))
    _too_deep(rtsr, lambda: scene.cast_rays(o, d))
    _too_deep(rtsr, lambda: scene.trace_rays(o[:64], d[:64], spp=2, max_depth=8))
    _too_deep(rtsr, lambda: scene.progressive(s.cam, s.cfg).features(2))
    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(rtsr.SCENE_BOOK1_CANONICAL)
    cfg = rtsr.Config.new(1.5, 64, 4, 50, 10, seed=1, background=bg)
    h = rtsr.image_height(cfg)
    flat = b.flatten(world)
    screen = flat.upload().render(cam, cfg)
    ref, ref8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=8)
    assert np.array_equal(screen.accum, ref) and np.array_equal(screen.rgb8, ref8)


def test_a_tree_of_61_levels_renders_or_is_refused(rtsr, orc, monkeypatch):
    """chain(16): between the 50 levels that fit beside k_trace_world's per-lane slots and the 64 that fit at all.  Under the
    default choice and under every forced kernel the frame equals the oracle's bit for bit, or the call is refused with
    RTX_EUNSUPPORTED, "too deep": no HIP launch error, no other frame.  DESIGN.md records which kernel does which."""
    s = _get(rtsr, "chain_16", 1)
    print("\n[lbvh edges] chain_16: %d stack levels" % s.levels)
    assert s.levels >= MIN_LEVELS["chain_16"]
    ref, ref8 = orc.o2_render(s.flat_gpu.arrays_ptr(), s.cam, s.cfg, s.h, threads=16)
    host, _ = orc.o2_render(s.flat_host.arrays_ptr(), s.cam, s.cfg, s.h, threads=16)
    assert np.array_equal(ref, host)
    rendered = 0
    for env in WALKERS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            got = s.flat_gpu.upload().render(s.cam, s.cfg, want_stats=True)
        except rtsr.RtxError as e:
            assert e.status == rtsr.RTX_EUNSUPPORTED and "too deep" in str(e), (env, str(e))
            print("[lbvh edges] chain_16 %s: refused (%s)" % (env or "default", e))
        else:
            assert np.array_equal(got.accum, ref), (env, _diff(got.accum, ref))
            assert np.array_equal(got.rgb8, ref8)
            rendered += 1
            print("[lbvh edges] chain_16 %s: rendered by %s, equal to the oracle" % (env or "default", rtsr.trace_kernel_name(got.stats.trace_kernel)))
        for k in env:
            monkeypatch.delenv(k)
    assert rendered >= 1
    _check_cast(rtsr, orc, s, "chain_16")
