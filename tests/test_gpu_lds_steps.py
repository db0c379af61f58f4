"""k_trace_lds, the parts its walk and shading steps lean on: the stack that is carried as the
address of its top entry and pops down to its sentinel slot, the LDS layout with the node array at a fixed offset and every
ring capacity / node record size behind it, and shading's choice of path by material kind on a scene whose neighbouring
records all differ in kind (the case a copy of the kind kept beside the LDS sphere record has to get right; that step was
measured and not kept, the case stays).  Every render is held to the CPU oracle bit for bit (tolerance 0, as in
test_gpu_parity.py)."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_REFS = {}


def _reference(orc, key, flat, cam, cfg, h):
    """The oracle's frame for `key`, computed once and shared (read-only) by the tests that render the same thing."""
    if key not in _REFS:
        accum, rgb8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=16)
        accum.setflags(write=False)
        rgb8.setflags(write=False)
        _REFS[key] = (accum, rgb8)
    return _REFS[key]


def _render_lds(rtsr, scene, cam, cfg):
    st = scene.render_device(cam, cfg, want_stats=True)
    assert rtsr.trace_kernel_name(st.trace_kernel) == "k_trace_lds"
    return scene.render(cam, cfg)


def _assert_equal(screen, ref):
    diff = np.abs(screen.accum - ref[0]).max(axis=2)
    assert np.array_equal(screen.accum, ref[0]), "%d of %d pixels differ, max |d| = %g" % (int((diff > 0).sum()), diff.size, diff.max())
    assert np.array_equal(screen.rgb8, ref[1])


# ---- 1. deep stack
NESTED = 30       # spheres, each six times the radius of the one before and containing it
NESTED_GROWTH = 6.0


def _nested_world(rtsr):
    """Spheres nested in one another, radius growing by a factor that makes the surface-area heuristic split the largest one
    off alone at every level (a factor g > sqrt(n) does: peeling one costs A (1 + (n - 1) / g^2), peeling two
    A (2 + (n - 2) / g^4)): the tree is a chain, one level per sphere, and the bounding-leaf-first rule asks that sphere first.
    They all touch the plane x = 0 from behind, near the origin where the camera looks from in front: a ray aimed there
    meets the boxes of both children at every level, stacks the far one each time, and pops all the way down to the sentinel
    slot.  Diffuse and metal surfaces: what scatters back towards the camera leaves the scene and picks up the sky."""
    b = rtsr.Builder(1)
    lst = b.hittable_list()
    for i in range(NESTED):
        r = 0.05 * NESTED_GROWTH ** i
        col = (0.3 + 0.1 * (i % 5), 0.8 - 0.1 * (i % 4), 0.4 + 0.15 * (i % 3))
        m = b.metal(col, 0.1) if i % 4 == 3 else b.lambertian(col)
        b.list_add(lst, b.sphere((-r - 0.004 * i, 0.0, 0.0), r, m))
    world = b.hittable_list([b.bvh_from_list(lst, 0.0, 1.0)])
    cam = rtsr.Camera.new((3.0, 0.6, 1.2), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.5, 0.0, 3.0, 0.0, 1.0)
    return b, world, cam


def test_deep_stack_pops_down_to_the_sentinel(rtsr, orc):
    b, world, cam = _nested_world(rtsr)
    flat = b.flatten(world)
    info = flat.info()
    assert info["max_stack"] >= 24, "the nested-sphere tree is only %d levels tall: the test would pass vacuously" % info["max_stack"]
    cfg = rtsr.Config.new(1.5, 96, 4, 8, 10, seed=5, background=(0.7, 0.8, 1.0))
    h = rtsr.image_height(cfg)
    assert h == 64
    screen = _render_lds(rtsr, flat.upload(), cam, cfg)
    _assert_equal(screen, _reference(orc, "nested", flat, cam, cfg, h))
    assert len(np.unique(screen.rgb8)) > 16  # (a picture, not a constant)


# ---- 2. layout edges
# (scene id, scene seed, leaf size, switches, ring capacity the launcher reports, dwords per LDS node record)
LAYOUT_CASES = [
    ("book1_ring64", 100, 1, 0, {}, 64, 21),
    ("book1_ring48", 100, 2, 0, {}, 48, 21),                      # (a tree one level taller: 2 KB of stack more)
    ("book1_no_ring", 100, 1, 0, {"RTX_RING": "0"}, 0, 21),
    ("head_one_axis", 13, 1, 0, {}, 0, 27),                       # (HEAD's 80-byte records leave no room for a ring)
    ("head_one_axis_leaf4_ring64", 13, 1, 4, {}, 64, 27),         # (... a third of the nodes do)
    ("head_all_axes", 13, 1, 0, {"RTX_MOTION_AXIS": "0"}, 0, 39),
    ("head_all_axes_leaf4_ring48", 13, 1, 4, {"RTX_MOTION_AXIS": "0"}, 48, 39),  # (159 nodes x 48 B more than one axis: 128 B over with 64)
    ("head_static_boxes", 13, 1, 0, {"RTX_MOTION": "0"}, 0, 21),
    ("head_static_boxes_leaf4_ring64", 13, 1, 4, {"RTX_MOTION": "0"}, 64, 21),
]
_RING_LINE = re.compile(r"k_trace_lds (on|off) \(ring of (\d+), (\d+) B of LDS\); time-aware boxes (on|off) \(ring of (\d+), (\d+) B\)")


def _layout_setup(rtsr, sid, scene_seed, max_leaf):
    b = rtsr.Builder(scene_seed)
    world, cam, bg = b.get_world_cam(sid)
    cfg = rtsr.Config.new(1.5, 144, 4, 50, 10, seed=17, background=bg)
    return b, world, cam, cfg, b.flatten(world, max_leaf=max_leaf)


@pytest.mark.parametrize("name,sid,scene_seed,max_leaf,env,ring,node_dwords", LAYOUT_CASES, ids=[c[0] for c in LAYOUT_CASES])
def test_layout_edges(rtsr, orc, monkeypatch, capfd, name, sid, scene_seed, max_leaf, env, ring, node_dwords):
    b, world, cam, cfg, flat = _layout_setup(rtsr, sid, scene_seed, max_leaf)
    h = rtsr.image_height(cfg)
    assert h == 96
    ref = _reference(orc, ("layout", sid, scene_seed, max_leaf), flat, cam, cfg, h)
    monkeypatch.setenv("RTX_SCENE_LDS", "1")  # (the default, said aloud: the launcher then reports what it fitted)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    scene = flat.upload()
    m = _RING_LINE.search(capfd.readouterr().err)
    assert m, "the launcher did not report its LDS plan"
    assert m.group(1) == "on" and int(m.group(3)) <= 160 * 1024
    motion_on = m.group(4) == "on"
    assert motion_on == (node_dwords != 21)
    got_ring = int(m.group(5)) if motion_on else int(m.group(2))
    assert got_ring == ring, "this case is meant to run with a ring of %d, the launcher chose %d" % (ring, got_ring)
    _assert_equal(_render_lds(rtsr, scene, cam, cfg), ref)


def test_two_footprints_alternating_in_one_process(rtsr, orc):
    """Layout offsets are per launch, never per process: two resident scenes with different trees, record kinds and node
    records (static Book-1: 21 dwords, spheres; HEAD: 27 dwords, moving-sphere records) rendered in turn, twice each."""
    scenes = []
    for sid, scene_seed in ((100, 1), (13, 1)):
        b, world, cam, cfg, flat = _layout_setup(rtsr, sid, scene_seed, 0)
        ref = _reference(orc, ("layout", sid, scene_seed, 0), flat, cam, cfg, rtsr.image_height(cfg))
        scenes.append((flat.upload(), cam, cfg, ref, b, flat))
    for _ in range(2):
        for scene, cam, cfg, ref, _b, _flat in scenes:
            _assert_equal(_render_lds(rtsr, scene, cam, cfg), ref)


# ---- 3. material kinds record by record
def _many_materials_world(rtsr):
    """300 small spheres over a ground sphere, every one with a material of its own; kinds cycle Lambertian / Metal /
    Dielectric, so material indices pass 255 and records that are neighbours in LDS differ in kind."""
    b = rtsr.Builder(1)
    lst = b.hittable_list()
    b.list_add(lst, b.sphere((0.0, -1000.0, 0.0), 1000.0, b.lambertian((0.5, 0.5, 0.5))))
    rng = np.random.RandomState(7)
    for i in range(300):
        c = (float(i % 20) - 9.5 + 0.3 * rng.rand(), 0.2, float(i // 20) - 7.0 + 0.3 * rng.rand())
        col = tuple(float(x) for x in 0.1 + 0.8 * rng.rand(3))
        if i % 3 == 0:
            m = b.lambertian(col)
        elif i % 3 == 1:
            m = b.metal(col, float(0.4 * rng.rand()))
        else:
            m = b.dielectric(1.3 + 0.4 * float(rng.rand()))
        b.list_add(lst, b.sphere(c, 0.2, m))
    world = b.hittable_list([b.bvh_from_list(lst, 0.0, 1.0)])
    cam = rtsr.Camera.new((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 64.0 / 48.0, 0.0, 10.0, 0.0, 1.0)
    return b, world, cam


@pytest.mark.parametrize("max_leaf", [1, 4])
def test_every_record_its_own_material_kinds_alternating(rtsr, orc, max_leaf):
    b, world, cam = _many_materials_world(rtsr)
    flat = b.flatten(world, max_leaf=max_leaf)
    assert flat.info()["n_materials"] > 256
    cfg = rtsr.Config.new(64.0 / 48.0, 64, 8, 50, 10, seed=9, background=(0.7, 0.8, 1.0))
    h = rtsr.image_height(cfg)
    assert h == 48
    screen = _render_lds(rtsr, flat.upload(), cam, cfg)
    _assert_equal(screen, _reference(orc, ("materials", max_leaf), flat, cam, cfg, h))
