"""rtx_flat_rebuild_instance_trees and rtx_flat_instance_tree_cost on the CPU: a new topology for an instance tree from its
members' boxes at the current pose, and the number that says when to ask for one.

Judges, none of them the code under test: a FRESH flatten at the pose (byte for byte for the SAH builder, ray for ray and
pixel for pixel for the Morton builder) and an audit of the arrays written in numpy (tests/rebuild_cases.py).  Every test
calls a symbol the library did not have before.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rebuild_cases as rc
from cast_rays_cases import same_bits, sphere_rays
from instance_scenes import box_field
from set_transforms_cases import NODE, build, leaf_boxes, random_values, tree_roots, updates_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("entries", "top_level", "nodes", "nodes32", "motion32", "member_local_box")
INFO = ("n_nodes", "n_refs", "n_entries", "n_top_level", "total_bytes", "max_stack", "n_bvh", "sah_cost")  # all but the build times


def _arrays(flat):
    return {name: flat.array(name) for name in ARRAYS}


def _records(orc, flat, o, d):
    out = np.zeros((len(o), 11))
    for r in range(len(o)):
        rec = orc.core_world_hit(flat.arrays_ptr(), tuple(o[r]), tuple(d[r]), 0.0, 0.001, float("inf"), rng_seed=1 + r)
        if rec is not None:
            out[r] = [1.0, rec["t"], *rec["p"], *rec["normal"], rec["u"], rec["v"], float(rec["front_face"])]
    return out


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_sah_rebuild_is_the_fresh_flatten(rtsr, name):
    """After the pose, RTX_REBUILD_SAH of every tree gives the fresh flat scene byte for byte in every array, and its info."""
    flat, calls, values, _, fresh = rc.posed(rtsr, name)
    flat.rebuild_instance_trees(builder="sah")
    got, want = _arrays(flat), _arrays(fresh)
    for k in ARRAYS:
        assert np.array_equal(got[k], want[k]), k
    gi, wi = flat.info(), fresh.info()
    assert all(gi[k] == wi[k] for k in INFO), (gi, wi)
    assert flat.instances() == fresh.instances()
    for k in range(flat.instances()["n_trees"]):
        assert flat.instance_tree(k) == fresh.instance_tree(k)


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_morton_rebuild_passes_the_audit(rtsr, name):
    flat, calls, values, trees, fresh = rc.posed(rtsr, name)
    before = _arrays(flat)
    n_trees = flat.instances()["n_trees"]
    depth_before = [flat.instance_tree(k)["depth"] for k in range(n_trees)]
    member_part = flat.info()["max_stack"] - 1 - max(depth_before)
    flat.rebuild_instance_trees(trees)
    after = _arrays(flat)
    rebuilt = range(n_trees) if trees is None else trees
    for k in range(n_trees):
        t = flat.instance_tree(k)
        if k in rebuilt:
            assert rc.audit_tree(flat, k) == t["depth"]
            assert rc.instance_records(flat)[k][0] == tree_roots(fresh)[k]  # both builders put the root first in the piece
        else:
            assert t["depth"] == depth_before[k]
    depths = [flat.instance_tree(k)["depth"] for k in range(n_trees)]
    assert flat.info()["max_stack"] == member_part + 1 + max(depths) and flat.instances()["max_depth"] == max(depths)
    # nothing outside the rebuilt trees' pieces moved
    nodes, nodes0 = after["nodes"].view(NODE), before["nodes"].view(NODE)
    outside = np.ones(len(nodes), dtype=bool)
    for k in rebuilt:
        root, _, n_slots = rc.instance_records(flat)[k]
        outside[root:root + n_slots - 1] = False
    assert nodes[outside].tobytes() == nodes0[outside].tobytes()
    for k in ("top_level", "member_local_box"):
        assert np.array_equal(after[k], before[k]), k
    assert np.array_equal(after["entries"], fresh.array("entries"))
    if name == "diagonal":
        # the first 21 members sit in 21 different octaves of the 21-bit grid: a chain of at least 21 nodes, deeper than the
        # SAH tree of the same pose, so max_stack rises
        print("diagonal: depth %d (SAH %d), max_stack %d (SAH %d)" % (depths[0], fresh.instance_tree(0)["depth"], flat.info()["max_stack"], fresh.info()["max_stack"]))
        assert depths[0] >= 21 and flat.info()["max_stack"] > fresh.info()["max_stack"]
    if name in ("point", "line"):
        # the degenerate inputs are what they claim: no centroid extent on three / two axes
        boxes = np.array(list(rc.member_boxes(flat, 0).values()))
        c = 0.5 * (boxes[:, :3] + boxes[:, 3:])
        assert int((c.max(axis=0) > c.min(axis=0)).sum()) == (0 if name == "point" else 1)
    if name == "point":
        assert depths[0] == 6  # 33 equal codes: the index tie-break alone gives the balanced tree of 33 leaves


@pytest.mark.parametrize("name", ["size_65", "diagonal", "two_trees", "zoo", "point"])
def test_rays_and_a_frame_on_the_morton_tree_equal_the_fresh_scene(rtsr, orc, name):
    flat, calls, values, trees, fresh = rc.posed(rtsr, name)
    flat.rebuild_instance_trees(trees, builder="morton")
    cam, cfg, h, lo, hi = rc.camera(rtsr, name)
    o, d = sphere_rays(2000, 5, lo, hi, 1.0)
    want = _records(orc, fresh, o, d)
    hits = int(want[:, 0].sum())
    assert 300 <= hits <= 1900, hits
    got = _records(orc, flat, o, d)
    assert same_bits(got, want).all(), "%d rays differ from the fresh scene" % int((~same_bits(got, want)).sum())
    assert (cfg.image_width, h, cfg.samples_per_pixel) == (48, 32, 8)
    a, a8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=4)
    f, f8 = orc.o2_render(fresh.arrays_ptr(), cam, cfg, h, threads=4)
    assert f.std() > 0.01 and np.array_equal(a, f) and np.array_equal(a8, f8)


@pytest.mark.parametrize("builder", ["morton", "sah"])
def test_set_transforms_after_a_rebuild(rtsr, builder):
    """A later pose on the rebuilt tree: every leaf box is the fresh flatten's of that pose, every union exact, and the audit
    still holds."""
    flat, calls, values, trees, _ = rc.posed(rtsr, "size_65")
    flat.rebuild_instance_trees(builder=builder)
    child = flat.array("nodes").view(NODE)["child"].copy()
    later = random_values(calls, seed=77, shift=3.0)
    flat.set_transforms(updates_for(flat, calls, later))
    bf, wf, _ = build(rtsr, rc.CASES["size_65"][0], later)
    fresh = bf.flatten(wf)
    assert np.array_equal(flat.array("entries"), fresh.array("entries"))
    nodes, fresh_nodes = flat.array("nodes").view(NODE), fresh.array("nodes").view(NODE)
    assert np.array_equal(nodes["child"], child)
    leaves, _ = leaf_boxes(nodes, tree_roots(flat)[0])
    fresh_leaves, _ = leaf_boxes(fresh_nodes, tree_roots(fresh)[0])
    assert sorted(leaves) == sorted(fresh_leaves)
    assert all(leaves[s][0].tobytes() == fresh_leaves[s][0].tobytes() and leaves[s][1].tobytes() == fresh_leaves[s][1].tobytes() for s in leaves)
    rc.audit_tree(flat, 0)


def test_cost_of_a_fresh_tree_equals_the_numpy_restatement(rtsr):
    for name in ("size_3", "size_257", "two_trees", "zoo"):
        fn = rc.CASES[name][0]
        b, w = fn(rtsr)[:2]
        flat = b.flatten(w)
        for k in range(flat.instances()["n_trees"]):
            got, want = flat.instance_tree_cost(k), rc.tree_cost(flat, k)
            assert got == want and np.isfinite(got) and got > 0.0, (name, k, got, want)


def test_a_rebuild_lowers_the_cost_of_the_scrambled_field(rtsr):
    """The statement the feature exists for: at the scramble pose the refitted tree costs strictly more than a rebuilt one,
    for both builders."""
    costs = {}
    for builder in ("morton", "sah"):
        flat, _, _, _, fresh = rc.posed(rtsr, "scramble")
        refitted = flat.instance_tree_cost(0)
        assert refitted == rc.tree_cost(flat, 0)
        flat.rebuild_instance_trees(builder=builder)
        costs[builder] = flat.instance_tree_cost(0)
        assert costs[builder] == rc.tree_cost(flat, 0)
        print("scramble, 257 members: cost refitted %.3f, rebuilt (%s) %.3f" % (refitted, builder, costs[builder]))
        assert refitted > costs[builder]
    assert costs["sah"] == rc.posed(rtsr, "scramble")[4].instance_tree_cost(0)


def test_every_refusal_leaves_the_flat_scene_unchanged(rtsr):
    b, w = rc.CASES["two_trees"][0](rtsr)[:2]
    flat = b.flatten(w)
    before, info = _arrays(flat), flat.info()
    fn = rtsr.lib.rtx_flat_rebuild_instance_trees
    I = lambda *v: (C.c_int32 * len(v))(*v)
    for what, args, word in (("negative n", (flat.ptr, I(0), -1, 0), "n < 0"), ("index past the trees", (flat.ptr, I(0, 2), 2, 0), "trees[1]"),
                             ("negative index", (flat.ptr, I(-1), 1, 0), "trees[0]"), ("named twice", (flat.ptr, I(1, 0, 1), 3, 0), "twice"),
                             ("unknown builder", (flat.ptr, I(0), 1, 2), "builder"), ("NULL flat", (None, I(0), 1, 0), "NULL"),
                             ("negative n with NULL", (flat.ptr, None, -1, 0), "n < 0")):
        assert fn(*args) == rtsr.RTX_EINVAL, what
        assert "rtx_flat_rebuild_instance_trees" in rtsr.last_error() and word in rtsr.last_error(), (what, rtsr.last_error())
        assert all(np.array_equal(_arrays(flat)[k], before[k]) for k in ARRAYS) and flat.info() == info, what
    cost = C.c_double(0.0)
    for k in (-1, 2):
        assert rtsr.lib.rtx_flat_instance_tree_cost(flat.ptr, k, C.byref(cost)) == rtsr.RTX_EINVAL and "k is out of range" in rtsr.last_error()
    assert rtsr.lib.rtx_flat_instance_tree_cost(None, 0, C.byref(cost)) == rtsr.RTX_EINVAL
    assert rtsr.lib.rtx_flat_instance_tree_cost(flat.ptr, 0, None) == rtsr.RTX_EINVAL
    with pytest.raises(ValueError):
        flat.rebuild_instance_trees(builder="lbvh")
    # nothing to do: n = 0 with a list; a scene without trees and NULL
    assert fn(flat.ptr, I(0), 0, 0) == rtsr.RTX_OK
    bh, wh = box_field(rtsr, "hoisted")
    hoisted = bh.flatten(wh)
    h0 = _arrays(hoisted)
    hoisted.rebuild_instance_trees()
    assert all(np.array_equal(_arrays(hoisted)[k], h0[k]) for k in ARRAYS)
    assert all(np.array_equal(_arrays(flat)[k], before[k]) for k in ARRAYS)
    # a chain of 63 nodes needs 64 + 1 stack levels: refused, untouched; the SAH builder takes the same pose
    deep, _, _, _, fresh = rc.posed(rtsr, "chain63")
    d0, i0 = _arrays(deep), deep.info()
    assert fn(deep.ptr, None, 0, 0) == rtsr.RTX_EUNSUPPORTED and "walk stack" in rtsr.last_error()
    assert all(np.array_equal(_arrays(deep)[k], d0[k]) for k in ARRAYS) and deep.info() == i0
    deep.rebuild_instance_trees(builder="sah")
    assert np.array_equal(deep.array("nodes"), fresh.array("nodes"))


def test_scene_entries_refuse_before_they_read_the_scene(rtsr):
    """What needs no scene is checked first: run on a scene pointer that must never be dereferenced (no GPU here)."""
    never = C.c_void_p(0x10)
    fn = rtsr.lib.rtx_scene_rebuild_instance_trees
    stats = rtsr.RtxRebuildStats()
    assert fn(None, None, 0, None, C.byref(stats)) == rtsr.RTX_EINVAL and "scene is NULL" in rtsr.last_error()
    assert fn(never, None, -1, None, C.byref(stats)) == rtsr.RTX_EINVAL and "n < 0" in rtsr.last_error()
    stats.reserved[2] = 1
    assert fn(never, None, 0, None, C.byref(stats)) == rtsr.RTX_EINVAL and "reserved[2]" in rtsr.last_error()
    cost = C.c_double(0.0)
    assert rtsr.lib.rtx_scene_instance_tree_cost(None, 0, C.byref(cost)) == rtsr.RTX_EINVAL
    assert rtsr.lib.rtx_scene_instance_tree_cost(never, 0, None) == rtsr.RTX_EINVAL


def test_host_rebuild_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/rebuild_host_check.cpp with the flattener and the builder under -fsanitize=address,undefined: both builders
    against a fresh flatten, a rebuild followed by set_transforms, the refusals."""
    host = os.path.join(ROOT, "ray-tracing-series-rust_amd", "csrc", "host")
    exe = str(tmp_path / "rebuild_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-pthread",
                    os.path.join(ROOT, "tests", "rebuild_host_check.cpp"), os.path.join(host, "scene_graph.cpp"),
                    os.path.join(host, "flatten.cpp"), os.path.join(host, "bvh_build.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "rebuild host check clean" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
