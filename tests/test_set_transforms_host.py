"""rtx_flat_set_transforms on the CPU: new parameters for the Translate / RotateY chains of top-level slots, with a refit of
the instance trees that hold them.

The judge is always the FRESH flat scene: the same world built by Builder with the new offsets and angles and flattened
(tests/set_transforms_cases.py).  Every test calls a symbol the library did not have before.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cast_rays_cases import check_mix, same_bits, sphere_rays
from instance_scenes import box_field, member_zoo, zoo_cam_cfg
from set_transforms_cases import (NODE, NODE32, build, calls_of_slots, leaf_boxes, narrow, random_values, tree_roots, updates_for, values_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCENES = {
    "zoo_middle": (lambda spelling: (lambda r: member_zoo(r, spelling, "middle")), (-8.0, -0.5, -6.5), (8.0, 6.0, 5.5)),
    "zoo_pair": (lambda spelling: (lambda r: member_zoo(r, spelling, "pair")), (-8.0, -0.5, -6.5), (8.0, 6.0, 5.5)),
    "box_field": (lambda spelling: (lambda r: box_field(r, spelling)), (-7.0, -0.5, -5.5), (7.0, 6.0, 5.5)),
}
ARRAYS = ("entries", "top_level", "nodes", "nodes32", "motion32", "member_local_box")


def _arrays(flat):
    return {name: flat.array(name) for name in ARRAYS}


def _records(orc, flat, o, d):
    out = np.zeros((len(o), 11))
    for r in range(len(o)):
        rec = orc.core_world_hit(flat.arrays_ptr(), tuple(o[r]), tuple(d[r]), 0.0, 0.001, float("inf"), rng_seed=1 + r)
        if rec is not None:
            out[r] = [1.0, rec["t"], *rec["p"], *rec["normal"], rec["u"], rec["v"], float(rec["front_face"])]
    return out


@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_moved_flat_scene_is_the_freshly_built_one(rtsr, orc, name):
    scene, lo, hi = SCENES[name]
    b0, w0, calls = build(rtsr, scene("instanced"))
    flat = b0.flatten(w0)
    assert flat.instances()["n_trees"] == 1
    first = _arrays(flat)
    values = random_values(calls, seed=11)
    bf, wf, calls_f = build(rtsr, scene("instanced"), values)
    assert values_of(calls_f) == values
    fresh = bf.flatten(wf)
    bh, wh, _ = build(rtsr, scene("hoisted"), values)
    hoisted = bh.flatten(wh)

    flat.set_transforms(updates_for(flat, calls, values))
    moved = _arrays(flat)
    judge = _arrays(fresh)
    assert np.array_equal(moved["entries"], judge["entries"]) and not np.array_equal(moved["entries"], first["entries"])
    assert np.array_equal(moved["top_level"], judge["top_level"])
    assert np.array_equal(moved["member_local_box"], first["member_local_box"])

    nodes, nodes0, fresh_nodes = moved["nodes"].view(NODE), first["nodes"].view(NODE), judge["nodes"].view(NODE)
    (root,), (fresh_root,) = tree_roots(flat), tree_roots(fresh)
    leaves, internal = leaf_boxes(nodes, root)
    fresh_leaves, _ = leaf_boxes(fresh_nodes, fresh_root)
    tree = flat.instance_tree(0)
    assert sorted(leaves) == sorted(fresh_leaves) == list(range(tree["first_slot"], tree["first_slot"] + tree["n_slots"]))
    for slot in leaves:  # every leaf box, matched by slot: bit for bit the fresh tree's
        assert leaves[slot][0].tobytes() == fresh_leaves[slot][0].tobytes(), slot
        assert leaves[slot][1].tobytes() == fresh_leaves[slot][1].tobytes(), slot
    assert len(internal) == tree["n_nodes"] - 1
    for n, c, child in internal:  # every internal child box: the union of the two boxes under it
        assert np.minimum(nodes["bmin"][child][0], nodes["bmin"][child][1]).tobytes() == nodes["bmin"][n][c].tobytes()
        assert np.maximum(nodes["bmax"][child][0], nodes["bmax"][child][1]).tobytes() == nodes["bmax"][n][c].tobytes()
    n32 = moved["nodes32"].view(NODE32)
    assert np.array_equal(n32["lo"], narrow(nodes["bmin"], up=False)) and np.array_equal(n32["hi"], narrow(nodes["bmax"], up=True))
    assert np.array_equal(nodes["child"], nodes0["child"]) and np.array_equal(nodes["pad"], nodes0["pad"])
    n32_0 = first["nodes32"].view(NODE32)
    assert np.array_equal(n32["child"], n32_0["child"]) and np.array_equal(n32["axis"], n32_0["axis"])
    # nodes outside the tree (the members' own BVHs live in local space) are untouched
    outside = np.ones(len(nodes), dtype=bool)
    outside[[root] + [child for _, _, child in internal]] = False
    assert nodes[outside].tobytes() == nodes0[outside].tobytes()

    # 2000 rays: the mix is counted on the fresh hoisted spelling's answers alone
    o, d = sphere_rays(2000, 5, lo, hi, 1.0)
    want = _records(orc, hoisted, o, d)
    check_mix(name, want)
    got = _records(orc, flat, o, d)
    assert same_bits(got, want).all(), "%d rays differ from the fresh hoisted scene" % int((~same_bits(got, want)).sum())

    cam, cfg, h = zoo_cam_cfg(rtsr, width=48, spp=8)
    assert (cfg.image_width, h, cfg.samples_per_pixel) == (48, 32, 8)
    a, a8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=4)
    f, f8 = orc.o2_render(fresh.arrays_ptr(), cam, cfg, h, threads=4)
    assert f.std() > 0.01 and np.array_equal(a, f) and np.array_equal(a8, f8)

    # the original pose again: every array as it was, byte for byte
    flat.set_transforms(updates_for(flat, calls, values_of(calls)))
    back = _arrays(flat)
    for k in ARRAYS:
        assert np.array_equal(back[k], first[k]), k


def test_partial_updates_and_slots_outside_a_tree(rtsr, orc):
    """One member, then every 7th member: the untouched members keep their ops and the tree is still the fresh one's.  Then the
    zoo spelled WITHOUT a tree: the same update is the scatter alone."""
    scene = lambda r: box_field(r, "instanced")
    b0, w0, calls = build(rtsr, scene)
    flat = b0.flatten(w0)
    tree = flat.instance_tree(0)
    members = [s for s in range(tree["first_slot"], tree["first_slot"] + tree["n_slots"]) if flat.slot_chain(s)]
    for only in ([members[17]], members[::7]):
        values = random_values(calls, seed=len(only), only_calls=calls_of_slots(flat, calls, set(only)))
        upd = updates_for(flat, calls, values, only=set(only))
        assert sorted(upd) == sorted(only)
        flat.set_transforms(upd)
        bf, wf, _ = build(rtsr, scene, values)
        fresh = bf.flatten(wf)
        assert np.array_equal(flat.array("entries"), fresh.array("entries"))
        nodes, fresh_nodes = flat.array("nodes").view(NODE), fresh.array("nodes").view(NODE)
        leaves, _ = leaf_boxes(nodes, tree_roots(flat)[0])
        fresh_leaves, _ = leaf_boxes(fresh_nodes, tree_roots(fresh)[0])
        assert all(leaves[s][0].tobytes() == fresh_leaves[s][0].tobytes() and leaves[s][1].tobytes() == fresh_leaves[s][1].tobytes() for s in leaves)
        flat.set_transforms(updates_for(flat, calls, values_of(calls)))
    bh, wh, calls_h = build(rtsr, lambda r: member_zoo(r, "hoisted", "pair"))
    hoisted = bh.flatten(wh)
    assert hoisted.instances()["n_trees"] == 0
    before = hoisted.array("nodes")
    values = random_values(calls_h, seed=3)
    hoisted.set_transforms(updates_for(hoisted, calls_h, values))
    bf, wf, _ = build(rtsr, lambda r: member_zoo(r, "hoisted", "pair"), values)
    assert np.array_equal(hoisted.array("entries"), bf.flatten(wf).array("entries"))
    assert np.array_equal(hoisted.array("nodes"), before)


def test_inspection_calls(rtsr):
    b, w = member_zoo(rtsr, "instanced", "two")
    flat = b.flatten(w)
    assert flat.instances()["n_trees"] == 2
    t0, t1 = flat.instance_tree(0), flat.instance_tree(1)
    assert t0["first_slot"] == 0 and t0["n_slots"] == 12 and t0["n_nodes"] == 11  # 11 objects, one a list of two: spliced in
    assert t1["first_slot"] == 14 and t1["n_nodes"] == t1["n_slots"] - 1  # the ground and a sphere stand between the trees
    assert t0["n_slots"] + t1["n_slots"] == flat.instances()["n_members"]
    assert max(t0["depth"], t1["depth"]) == flat.instances()["max_depth"]
    with pytest.raises(rtsr.RtxError) as e:
        flat.instance_tree(2)
    assert e.value.status == rtsr.RTX_EINVAL and "k is out of range" in str(e.value)
    kinds = flat.top_level_kinds()
    chains = {s: flat.slot_chain(s) for s in range(len(kinds))}
    assert all(bool(chains[s]) == (kinds[s] == 3) for s in chains)  # no medium over a chain here
    assert sorted(len(c) for c in chains.values() if c) == [1, 1, 2, 2, 2, 2, 2, 3, 4]
    assert ["translate", "rotate_y", "translate", "rotate_y"] in chains.values()
    with pytest.raises(IndexError):
        flat.slot_chain(len(kinds))
    k4 = (C.c_int32 * 4)()
    assert rtsr.lib.rtx_flat_slot_chain(flat.ptr, -1, k4) == -1 and rtsr.lib.rtx_flat_slot_chain(None, 0, k4) == -1
    # a medium over a chain reports the chain of its boundary
    b2 = rtsr.Builder(1)
    grey = b2.lambertian((0.5, 0.5, 0.5))
    smoke = b2.constant_medium((1.0, 1.0, 1.0), 0.01, b2.translate((1.0, 0.0, 0.0), b2.rotate_y(15.0, b2.rect_prism((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), grey))))
    f2 = b2.flatten(b2.hittable_list([b2.sphere((0.0, -100.0, 0.0), 100.0, grey), smoke]))
    assert f2.top_level_kinds() == [0, 4] and f2.slot_chain(0) == [] and f2.slot_chain(1) == ["translate", "rotate_y"]


def _ops(rtsr, slot, *ops):
    u = rtsr.RtxSlotOps()
    u.slot, u.n_ops = slot, len(ops)
    for k, (kind, v) in enumerate(ops):
        u.ops[k].op = kind
        for a, x in enumerate(v):
            u.ops[k].v[a] = x
    return u


T, R = 0, 1
NAN, INF, BIG = float("nan"), float("inf"), 1.7976931348623157e308  # BIG: the largest double


def _refusals(rtsr, slot_tr, slot_plain, n_top):
    """(name, updates or None, n or None, word the message must hold, needs the scene).  slot_tr: a Translate(RotateY(..)) member
    of a tree; slot_plain: a slot without a chain."""
    ok = _ops(rtsr, slot_tr, (T, (1.0, 0.0, 1.0)), (R, (30.0,)))
    return [
        ("null updates", None, 1, "updates is NULL", False),
        ("negative n", [ok], -1, "n < 0", False),
        ("slot negative", [_ops(rtsr, -1, (T, (0.0, 0.0, 0.0)))], None, ".slot", False),
        ("slot past the list", [_ops(rtsr, n_top, (T, (0.0, 0.0, 0.0)))], None, ".slot", True),
        ("slot without a chain", [_ops(rtsr, slot_plain, (T, (0.0, 0.0, 0.0)))], None, "chain", True),
        ("n_ops out of the struct", [_ops(rtsr, slot_tr, *[(T, (0.0, 0.0, 0.0))] * 4)], None, ".n_ops", False),
        ("n_ops not the chain's", [_ops(rtsr, slot_tr, (T, (1.0, 0.0, 1.0)))], None, ".n_ops", True),
        ("op kind unknown", [_ops(rtsr, slot_tr, (7, (1.0, 0.0, 1.0)), (R, (30.0,)))], None, ".op", False),
        ("op kind not the chain's", [_ops(rtsr, slot_tr, (R, (30.0,)), (T, (1.0, 0.0, 1.0)))], None, ".op", True),
        ("slot named twice", [ok, _ops(rtsr, slot_tr + 1, (T, (1.0, 0.0, 1.0)), (R, (30.0,))), ok], None, "twice", False),
        ("NaN offset", [_ops(rtsr, slot_tr, (T, (1.0, NAN, 1.0)), (R, (30.0,)))], None, "not finite", False),
        ("infinite angle", [_ops(rtsr, slot_tr, (T, (1.0, 0.0, 1.0)), (R, (INF,)))], None, "not finite", False),
        ("member box not finite", [_ops(rtsr, slot_tr, (T, (BIG, 0.0, BIG)), (R, (45.0,)))], None, "bounding box", True),
    ]


def _call(rtsr, fn, handle, updates, n, *rest):
    arr = (rtsr.RtxSlotOps * len(updates))(*updates) if updates is not None else None
    return fn(handle, arr, len(updates) if n is None else n, *rest)


def test_every_refusal_leaves_the_flat_scene_unchanged(rtsr):
    b, w = box_field(rtsr, "instanced")
    flat = b.flatten(w)
    tree = flat.instance_tree(0)
    slot_tr = tree["first_slot"] + 3
    assert flat.slot_chain(slot_tr) == flat.slot_chain(slot_tr + 1) == ["translate", "rotate_y"] and flat.slot_chain(0) == []
    before = _arrays(flat)
    cases = _refusals(rtsr, slot_tr, 0, flat.info()["n_top_level"])
    assert len(cases) == 13
    for name, updates, n, word, _ in cases:
        if name == "n_ops out of the struct":
            updates[0].n_ops = 5
        st = _call(rtsr, rtsr.lib.rtx_flat_set_transforms, flat.ptr, updates, n)
        assert st == rtsr.RTX_EINVAL, name
        msg = rtsr.last_error()
        assert "rtx_flat_set_transforms" in msg and word in msg, (name, msg)
        after = _arrays(flat)
        assert all(np.array_equal(after[k], before[k]) for k in ARRAYS), name
    assert rtsr.lib.rtx_flat_set_transforms(None, None, 0) == rtsr.RTX_EINVAL and "NULL" in rtsr.last_error()
    # n = 0 is fine and changes nothing; a good update after all the refusals still goes through
    assert rtsr.lib.rtx_flat_set_transforms(flat.ptr, (rtsr.RtxSlotOps * 1)(), 0) == rtsr.RTX_OK
    assert all(np.array_equal(_arrays(flat)[k], before[k]) for k in ARRAYS)
    flat.set_transforms({slot_tr: [("translate", (1.0, 0.0, 1.0)), ("rotate_y", 30.0)]})
    assert not np.array_equal(flat.array("nodes"), before["nodes"])


def test_scene_entry_refuses_before_it_reads_the_scene(rtsr):
    """rtx_scene_set_transforms checks what needs no scene first: run on a scene pointer that must never be dereferenced (no
    GPU here, and the address is not a scene)."""
    never = C.c_void_p(0x10)
    for name, updates, n, word, needs_scene in _refusals(rtsr, 4, 0, 100):
        if needs_scene:
            continue
        if name == "n_ops out of the struct":
            updates[0].n_ops = 5
        st = _call(rtsr, rtsr.lib.rtx_scene_set_transforms, never, updates, n, None)
        assert st == rtsr.RTX_EINVAL, name
        assert "rtx_scene_set_transforms" in rtsr.last_error() and word in rtsr.last_error(), (name, rtsr.last_error())
    assert rtsr.lib.rtx_scene_set_transforms(None, (rtsr.RtxSlotOps * 1)(), 1, None) == rtsr.RTX_EINVAL and "scene is NULL" in rtsr.last_error()
    assert rtsr.lib.rtx_scene_set_transforms(never, (rtsr.RtxSlotOps * 1)(), 0, None) == rtsr.RTX_OK  # n = 0: nothing to do
    assert rtsr.lib.rtx_device_scene_array(None, 0, None, 0) == rtsr.RTX_EINVAL


def test_python_layer_raises_value_error_before_the_library(rtsr):
    b, w = box_field(rtsr, "instanced")
    flat = b.flatten(w)
    slot = flat.instance_tree(0)["first_slot"] + 2
    before = _arrays(flat)
    good = [("translate", (0.0, 0.0, 0.0)), ("rotate_y", 10.0)]
    bad = [
        [(slot, good)],  # not a dict
        {-1: good}, {10 ** 6: good}, {"3": good}, {0: good},  # out of range, not an integer, no chain
        {slot: good[:1]}, {slot: good[::-1]}, {slot: [("scale", 2.0), good[1]]}, {slot: [good[0], ("rotate_y", (1.0, 2.0))]},
        {slot: [("translate", (0.0, 0.0)), good[1]]}, {slot: [("translate", (0.0, float("nan"), 0.0)), good[1]]},
        {slot: [good[0], ("rotate_y", float("inf"))]}, {slot: [good[0], "rotate_y"]},
    ]
    rtsr.lib.rtx_flat_set_transforms(None, None, 0)
    marker = rtsr.last_error()
    for upd in bad:
        with pytest.raises(ValueError):
            flat.set_transforms(upd)
    assert rtsr.last_error() == marker  # the library was not called
    assert all(np.array_equal(_arrays(flat)[k], before[k]) for k in ARRAYS)
    flat.set_transforms({})
    flat.set_transforms({slot: good})
    assert not np.array_equal(flat.array("entries"), before["entries"])


def test_host_refit_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/set_transforms_host_check.cpp with the flattener and the builder under -fsanitize=address,undefined: full and
    partial updates of the zoo against a fresh flatten byte for byte, the refusals, and the device's narrowing against the
    converter's."""
    host = os.path.join(ROOT, "ray-tracing-series-rust_amd", "csrc", "host")
    exe = str(tmp_path / "set_transforms_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-pthread",
                    os.path.join(ROOT, "tests", "set_transforms_host_check.cpp"), os.path.join(host, "scene_graph.cpp"),
                    os.path.join(host, "flatten.cpp"), os.path.join(host, "bvh_build.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "set_transforms host check clean" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
