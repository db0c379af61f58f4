"""Where a walk of k_trace_lds enters its tree (csrc/hip/lds_variant.inc: lds_entry_pair, the function the kernel itself asks
in its prologue), on the host: hand-written node tables, then the worlds of tests/lds_entry_cases.py as the flattener builds
them -- and the two CPU oracles agree on every one of those worlds, the tie world included, so the device test
(tests/test_gpu_lds_entry.py) has a reference that does not share the kernel's walk."""
import os
import subprocess

import numpy as np
import pytest

import lds_entry_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DONE = -1


@pytest.fixture(scope="module")
def entry_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lds_entry") / "lds_entry_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "lds_entry_host_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")

    def run(root, nodes):
        args = [str(root)] + [str(x) for n in nodes for x in n]
        out = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=60)
        assert out.returncode == 0 and "runtime error" not in out.stderr, out.stdout + out.stderr
        first, second = out.stdout.split()
        return int(first), int(second)
    return run


def test_item_encoding_written_out():
    assert ec.leaf_item(0) == -32768 and ec.leaf_item(1) == -32764 and ec.leaf_item(5, 4) == -32768 + 23
    assert ec.leaf_item(8189, 4) == -9  # the last item a leaf can be: 0xFFF7 (done is -1)
    assert ec.node_item(7, 0) == 7 and ec.node_item(7, 2) == 0x4007 and ec.node_item(0, 3) == 0x6000
    assert ec.leaf_code(0) == -2147483648 and ec.leaf_code(2, 3) == -2147483648 + 18


def test_hand_written_tables(entry_exe):
    L = ec.leaf_code
    # leaf-first root over a subtree: the leaf in hand, child 1 (node 1, split along y) under it
    nodes = [(L(0), 1, 3), (L(1), 2, 1), (L(2), L(3), 0)]
    assert entry_exe(0, nodes) == (ec.leaf_item(0), ec.node_item(1, 1))
    # ... the same tree stored with its root last
    nodes = [(L(2), L(3), 0), (L(1), 0, 2), (L(0), 1, 3)]
    assert entry_exe(2, nodes) == (ec.leaf_item(0), ec.node_item(1, 2))
    # ... child 1 itself a leaf-first node: its axis travels with the item
    nodes = [(L(0), 1, 3), (L(1), 2, 3), (L(2), L(3), 0)]
    assert entry_exe(0, nodes) == (ec.leaf_item(0), ec.node_item(1, 3))
    # a leaf-first root whose child 1 is a leaf (of three slots): two leaf items
    nodes = [(L(4), L(0, 3), 3)]
    assert entry_exe(0, nodes) == (ec.leaf_item(4), ec.leaf_item(0, 3))
    # a plain root, for every axis: entered at the root, nothing under it
    for axis in range(3):
        nodes = [(1, 2, axis), (L(0), L(1), 0), (L(2), L(3), 1)]
        assert entry_exe(0, nodes) == (ec.node_item(0, axis), DONE)
        assert entry_exe(2, nodes) == (ec.node_item(2, 1), DONE)
    # plain roots with a leaf for child 0, or two: not leaf-first without axis 3
    assert entry_exe(0, [(L(0), 1, 1), (L(1), L(2), 0)]) == (ec.node_item(0, 1), DONE)
    assert entry_exe(0, [(L(0), L(1), 2)]) == (ec.node_item(0, 2), DONE)
    # "axis 3" over two subtrees is not what the builder writes; such a root is entered like any other
    assert entry_exe(0, [(1, 2, 3), (L(0), L(1), 0), (L(2), L(3), 1)]) == (ec.node_item(0, 3), DONE)
    # the largest indices an item holds
    nodes = [(L(0), L(1), 0)] * 8191
    nodes[8190] = (L(8189), 8189, 3)
    nodes[8189] = (L(0), L(1), 2)
    assert entry_exe(8190, nodes) == (ec.leaf_item(8189), ec.node_item(8189, 2)) == (-12, 0x5FFD)


@pytest.mark.parametrize("name", ec.WORLDS)
def test_worlds_as_the_flattener_builds_them(rtsr, entry_exe, name):
    b, world = ec.build(rtsr, name)
    flat = b.flatten(world)
    root, nodes = ec.node_table(flat)
    c0, c1, axis = nodes[root]
    got = entry_exe(root, nodes)
    if ec.expect_leaf_first(name):
        # the bounding sphere is the first of its list and a leaf of one slot; what is under it is a subtree
        assert axis == 3 and c0 < 0 and c1 >= 0, (name, nodes[root])
        slot = ((c0 & 0x7FFFFFFF) >> 3)
        assert (c0 & 7) == 0
        assert got == (ec.leaf_item(slot), ec.node_item(c1, nodes[c1][2]))
        if name == "twins":
            assert len(nodes) == 2 and nodes[c1][0] < 0 and nodes[c1][1] < 0 and nodes[c1][2] != 3
    else:
        assert axis in (0, 1, 2), (name, nodes[root])
        assert got == (ec.node_item(root, axis), DONE)
        if name == "ground_1":
            assert len(nodes) == 1 and c0 < 0 and c1 < 0
    # the stack the launcher gives a walk holds the entry: level 1 exists (levels = max_stack + 1, slot 0 the sentinel)
    assert flat.info()["max_stack"] >= (2 if ec.expect_leaf_first(name) else 1)


def _frames(rtsr, orc, name, which, max_depth):
    b, world = ec.build(rtsr, name)
    cam = ec.camera(rtsr, which, 0.25, 0.75) if name == "moving" else ec.camera(rtsr, which)
    cfg = ec.config(rtsr, max_depth)
    h = rtsr.image_height(cfg)
    assert (cfg.image_width, h) == (64, 42)
    flat = b.flatten(world)
    a1, r1 = orc.o1_render(b.graph_ptr(), world, cam, cfg, h, threads=8)
    a2, r2 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=8)
    return a1, r1, a2, r2


@pytest.mark.parametrize("name", ec.WORLDS)
@pytest.mark.parametrize("which", ec.CAMERAS)
def test_the_two_oracles_agree(rtsr, orc, name, which):
    for max_depth in (1, 50):
        a1, r1, a2, r2 = _frames(rtsr, orc, name, which, max_depth)
        assert np.isfinite(a2).all()
        assert np.array_equal(a1, a2), "%s / %s / depth %d: %d pixels differ" % (name, which, max_depth, int((a1 != a2).any(axis=2).sum()))
        assert np.array_equal(r1, r2)
    # (depth 50) a picture, not a constant -- except straight up from worlds with nothing overhead, where there is only sky
    if not (which == "up" and name in ("ground_1", "twins")):
        assert len(np.unique(a2.reshape(-1, 3), axis=0)) >= 8, (name, which)


@pytest.mark.parametrize("name", ["ground_3", "moving"])
@pytest.mark.parametrize("width,aspect", ec.THIN_FRAMES, ids=lambda v: str(v))
def test_the_two_oracles_agree_on_thin_frames(rtsr, orc, name, width, aspect):
    """Frames one pixel wide or high: primary rays with infinite or NaN components, which every box rules out and no sphere
    does.  Both oracles see the sky there, although the camera looks at the ground."""
    b, world = ec.build(rtsr, name)
    cam = ec.camera(rtsr, "book1", 0.25, 0.75)
    cfg = rtsr.Config.new(aspect, width, ec.SPP, 50, 8, seed=11, background=ec.SKY)
    h = rtsr.image_height(cfg)
    assert 1 in (width, h)
    flat = b.flatten(world)
    a1, r1 = orc.o1_render(b.graph_ptr(), world, cam, cfg, h, threads=2)
    a2, r2 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=2)
    assert np.array_equal(a1, a2, equal_nan=True) and np.array_equal(r1, r2)
    assert np.array_equal(a2, np.broadcast_to(np.array(ec.SKY) * ec.SPP, a2.shape))


def test_the_tie_goes_to_the_second_twin(rtsr, orc):
    """Every primary ray that meets the ground of `twins` meets both twins at one t; the later one in the list answers (a
    HittableList's rule, core/geometry.hpp: offer_prim), whichever is tested first: the frame is the one of a world without
    the first twin, and not the one of a world without the second."""
    cam, cfg = ec.camera(rtsr, "book1"), ec.config(rtsr, 50)
    h = rtsr.image_height(cfg)
    b, world = ec.build(rtsr, "twins")
    flat = b.flatten(world)
    both, _ = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=8)

    def without(first):
        b1 = rtsr.Builder(1)
        mats = [b1.metal((0.9, 0.6, 0.2), 0.0), b1.lambertian((0.2, 0.7, 0.3)), b1.lambertian((0.9, 0.1, 0.1))]
        objs = [b1.sphere((0.0, -1000.0, 0.0), 1000.0, mats[1 if first else 0]), b1.sphere((0.0, -1000.0, 0.0), 990.0, mats[2])]
        w1 = b1.hittable_list([b1.bvh_from_list(b1.hittable_list(objs), 0.0, 1.0)])
        f1 = b1.flatten(w1)
        return orc.o2_render(f1.arrays_ptr(), cam, cfg, h, threads=8)[0]
    assert np.array_equal(both, without(first=True))
    assert not np.array_equal(both, without(first=False))
