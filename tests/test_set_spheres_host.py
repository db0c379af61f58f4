"""rtx_flat_set_spheres and rtx_flat_sphere_ids on the CPU: a new centre and radius for named static spheres of a flat scene,
its BVHs refitted with their topology kept.

The judge is always the FRESH flat scene -- the same world built from scratch with the moved spheres and flattened
(tests/sphere_update_cases.py) -- and the oracle, never the code under test.  Every test calls a symbol the library did not
have before.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cast_rays_cases import same_bits
from sphere_update_cases import (CASES, FLAT_ARRAYS, LIGHT, MOTION32, NODE, NODE32, SPHERE, assert_update_can_show, beside_movers, book1, book1_update,
                                 cam_cfg, instanced, lamp, leaf_boxes, narrow, refusals, rest_and_moved, seeded_rays, tree_roots,
                                 update_of)
from update_cases import assert_same_topology, call_set_prims, flat_arrays, hit_records as _records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_ARRAYS = ("refs", "rects")  # no hook of the library's reads these: the oracle's view of the same FlatScene does


def _arrays(flat):
    return flat_arrays(flat, FLAT_ARRAYS, ORACLE_ARRAYS)


def _same_arrays(flat, first):
    now = _arrays(flat)
    return all(np.array_equal(now[k], first[k]) for k in first)


def _assert_back_at_rest(flat, first):
    """Byte for byte the arrays of the first flatten -- signed zeros aside: where the bytes differ the values must be equal."""
    now = _arrays(flat)
    for k in first:
        if np.array_equal(now[k], first[k]):
            continue
        assert k in ("nodes", "nodes32", "member_local_box", "top_box32"), k
        dt = {"nodes": NODE, "nodes32": NODE32, "member_local_box": np.float64, "top_box32": np.float32}[k]
        a, b = now[k].view(dt), first[k].view(dt)
        for f in (a.dtype.names or [None]):
            x, y = (a[f], b[f]) if f else (a, b)
            assert np.array_equal(x, y), (k, f)  # numeric equality: +0 == -0


def _same_topology(now, first):
    assert_same_topology(now, first, ("entries", "top_level", "triangles") + ORACLE_ARRAYS)


def _check_against_fresh(rtsr, orc, flat, fresh, first):
    """Everything the issue asks of an updated flat scene but the rays and the frame."""
    now, judge = _arrays(flat), _arrays(fresh)
    # spheres by id: an id is the index in the sphere array, and both builds emit the spheres in the same order
    assert np.array_equal(now["spheres"], judge["spheres"])
    assert np.array_equal(now["spheres"].view(SPHERE)["mat"], first["spheres"].view(SPHERE)["mat"])
    rc, depth = orc.audit_flat_exact(flat.arrays_ptr(), ask_first=True)
    assert rc == 0
    _same_topology(now, first)
    nodes, n32 = now["nodes"].view(NODE), now["nodes32"].view(NODE32)
    assert np.array_equal(n32["lo"], narrow(nodes["bmin"], up=False)) and np.array_equal(n32["hi"], narrow(nodes["bmax"], up=True))
    assert (len(now["motion32"]) > 0) == (len(first["motion32"]) > 0)
    if len(now["motion32"]):
        mo, mo0, n32_0 = now["motion32"].view(MOTION32), first["motion32"].view(MOTION32), first["nodes32"].view(NODE32)
        static = np.array([np.array_equal(mo0["lo0"][i], n32_0["lo"][i]) and not mo0["dlo"][i].any() and not mo0["dhi"][i].any() for i in range(len(mo0))])
        assert static.any()
        assert np.array_equal(mo["lo0"][static], n32["lo"][static]) and np.array_equal(mo["hi0"][static], n32["hi"][static])
        assert not mo["dlo"][static].any() and not mo["dhi"][static].any()
        assert mo[~static].tobytes() == mo0[~static].tobytes()
    # instance trees: local boxes and leaf boxes matched by slot (a fresh build may choose another topology above the same leaves)
    assert np.array_equal(now["member_local_box"], judge["member_local_box"])
    for root, fresh_root in zip(tree_roots(flat), tree_roots(fresh)):
        leaves, _ = leaf_boxes(nodes, root)
        fresh_leaves, _ = leaf_boxes(judge["nodes"].view(NODE), fresh_root)
        assert sorted(leaves) == sorted(fresh_leaves)
        for slot in leaves:
            assert leaves[slot][0].tobytes() == fresh_leaves[slot][0].tobytes() and leaves[slot][1].tobytes() == fresh_leaves[slot][1].tobytes(), slot
    assert np.array_equal(now["top_box32"], judge["top_box32"])
    # the light table an upload would build now: that of the fresh build, and its census
    assert np.array_equal(now["lights"], judge["lights"])
    assert len(now["lights"]) // LIGHT.itemsize == fresh.lights()["n_lights"] and flat.lights() == fresh.lights()
    return depth


def _rays_and_frames(rtsr, orc, case, flat, fresh, lit, seed=17):
    """2 000 seeded rays through core_world_hit on the updated flat scene equal those on the fresh one bit for bit; a 48 x 32 x
    4 spp O2 frame of the updated scene equals O2 of the fresh scene AND O1 of the fresh graph `lit` (which also proves the
    case free of ties)."""
    o, d = seeded_rays(2000, seed)
    want = _records(orc, fresh, o, d)
    assert 200 < int(want[:, 0].sum())
    got = _records(orc, flat, o, d)
    assert same_bits(got, want).all(), "%d rays differ from the fresh scene" % int((~same_bits(got, want)).sum())
    cam, cfg, h = cam_cfg(rtsr, case)
    assert (cfg.image_width, h, cfg.samples_per_pixel) == (48, 32, 4)
    a, a8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=4)
    f, f8 = orc.o2_render(fresh.arrays_ptr(), cam, cfg, h, threads=4)
    assert f.std() > 0.01 and np.array_equal(a, f) and np.array_equal(a8, f8)
    if lit is not None:
        l, l8 = orc.o1_render(lit.builder.graph_ptr(), lit.world, cam, cfg, h, threads=4)
        assert np.array_equal(a, l) and np.array_equal(a8, l8)


@pytest.mark.parametrize("name", sorted(CASES))
def test_an_updated_flat_scene_is_the_freshly_built_one(rtsr, orc, name):
    case, moved = CASES[name](rtsr, False), CASES[name](rtsr, True)
    assert_update_can_show(*rest_and_moved(case))  # before anything else: a missing refit must be able to show
    flat, fresh = case.flatten(), moved.flatten()
    first = _arrays(flat)
    _, depth0 = orc.audit_flat_exact(flat.arrays_ptr(), ask_first=True)
    ids, vals = update_of(case, flat)
    flat.set_spheres(ids, vals)
    assert not np.array_equal(flat.array("spheres"), first["spheres"])
    if name not in ("plain", "fog") and not name.startswith("lamp"):  # (worlds without a BVH have no node)
        assert not np.array_equal(flat.array("nodes"), first["nodes"])
    assert _check_against_fresh(rtsr, orc, flat, fresh, first) == depth0
    # the literal oracle has no instance tree (its members are compared through O2 only) and no rule for a sphere of negative
    # radius inside a BvhNode (its inverted box: the cases module says so)
    lit = None if name in ("instanced", "hollow") else moved
    _rays_and_frames(rtsr, orc, case, flat, fresh, lit)
    # back to rest: every array as the first flatten left it
    flat.set_spheres(*update_of(case, flat, moved=False))
    _assert_back_at_rest(flat, first)


@pytest.mark.parametrize("name", ["mixed", "shared", "instanced", "field65", "plain"])
def test_partial_updates(rtsr, orc, name):
    """One id, every 7th id, then two updates in a row: each judged by the scene built from scratch with just those moved."""
    case = CASES[name](rtsr, False)
    flat = case.flatten()
    first = _arrays(flat)
    n_all = len(update_of(case, flat)[0])
    patterns = [(lambda k: k == 0, {"only": 0})] + ([(lambda k: k % 7 == 0, {"every": 7})] if n_all > 7 else [])
    for sel, kw in patterns:
        ids, vals = update_of(case, flat, **kw)
        assert 0 < len(ids) < n_all
        flat.set_spheres(ids, vals)
        fresh = CASES[name](rtsr, sel).flatten()
        _check_against_fresh(rtsr, orc, flat, fresh, first)
        o, d = seeded_rays(300, 5)
        assert same_bits(_records(orc, flat, o, d), _records(orc, fresh, o, d)).all()
        flat.set_spheres(*update_of(case, flat, moved=False, **kw))
        _assert_back_at_rest(flat, first)
    ids, vals = update_of(case, flat)
    half = len(ids) // 2
    flat.set_spheres(ids[:half], vals[:half])
    _check_against_fresh(rtsr, orc, flat, CASES[name](rtsr, lambda k: k < half).flatten(), first)
    flat.set_spheres(ids[half:], vals[half:])
    _check_against_fresh(rtsr, orc, flat, CASES[name](rtsr, True).flatten(), first)


def test_the_light_table_follows_a_sphere_light(rtsr):
    """The lamp's three updates by what they must do to the table: a move into the black cell takes the sphere light's
    probability to 0 without touching its area; a new radius changes the area and the split; and with the rectangle light
    dark too, the move leaves no weight at all -- every light gets the same probability."""
    def table(flat):
        return flat.array("lights").view(LIGHT)

    case = lamp(rtsr, False)
    flat = case.flatten()
    t0 = table(flat).copy()
    assert len(t0) == 2 and list(t0["kind"]) == [1, 0] and 0.0 < t0["pmf"][0] < 1.0 and t0["cdf"][1] == 1.0
    flat.set_spheres(*update_of(case, flat, only=0))
    t1 = table(flat)
    assert t1["area"][0] == t0["area"][0] and t1["pmf"][0] == 0.0 and t1["pmf"][1] == 1.0
    case = lamp(rtsr, False, to="radius")
    flat = case.flatten()
    flat.set_spheres(*update_of(case, flat, only=0))
    t2 = table(flat)
    assert t2["area"][0] == 4.0 * np.pi * 0.17 * 0.17 and 0.0 < t2["pmf"][0] < t0["pmf"][0] and t2["area"][1] == t0["area"][1]
    case = lamp(rtsr, False, dark_rect=True)
    flat = case.flatten()
    t3 = table(flat).copy()
    assert t3["pmf"][0] == 1.0 and t3["pmf"][1] == 0.0  # the only non-zero weight
    flat.set_spheres(*update_of(case, flat, only=0))
    t4 = table(flat)
    assert list(t4["pmf"]) == [0.5, 0.5] and list(t4["cdf"]) == [0.5, 1.0]  # the uniform fallback


def test_book1_final_refits_exactly_and_returns_to_rest(rtsr, orc):
    """Catalogue scene 100, its small spheres moved: the catalogue builds it from its own random stream, so there is no second
    build with other values; the judges are the oracle's exact box audit, the untouched topology and the way back."""
    b, world, cam, bg = book1(rtsr)
    flat = b.flatten(world)
    first = _arrays(flat)
    ids, rest, mv = book1_update(flat, b, world)
    assert len(ids) > 400
    assert_update_can_show(rest, mv)
    _, depth0 = orc.audit_flat_exact(flat.arrays_ptr(), ask_first=True)
    flat.set_spheres(ids, mv)
    now = _arrays(flat)
    rc, depth = orc.audit_flat_exact(flat.arrays_ptr(), ask_first=True)
    assert rc == 0 and depth == depth0
    _same_topology(now, first)
    sph = now["spheres"].view(SPHERE)
    assert np.array_equal(np.column_stack([sph["c"][ids], sph["radius"][ids]]), mv)
    nodes, n32 = now["nodes"].view(NODE), now["nodes32"].view(NODE32)
    assert not np.array_equal(now["nodes"], first["nodes"])
    assert np.array_equal(n32["lo"], narrow(nodes["bmin"], up=False)) and np.array_equal(n32["hi"], narrow(nodes["bmax"], up=True))
    flat.set_spheres(ids, rest)
    _assert_back_at_rest(flat, first)


def test_sphere_ids_on_every_kind_of_handle(rtsr):
    case = instanced(rtsr, False)
    b, flat, hs = case.builder, case.flatten(), case.handles
    sph = flat.array("spheres").view(SPHERE)
    for h, rest, _ in case.parts:  # a sphere handle: its own id, and the record holds its values
        ids = flat.sphere_ids(b, h)
        assert ids.dtype == np.int32 and len(ids) == 1
        assert np.array_equal(np.array([*sph["c"][ids[0]], sph["radius"][ids[0]]]), rest)
    id_of = lambda h: int(flat.sphere_ids(b, h)[0])
    group_ids = [id_of(h) for h, _, _ in case.parts[1:4]]
    bvh_ids = [id_of(h) for h, _, _ in case.parts[4:]]
    assert list(flat.sphere_ids(b, hs["group"])) == group_ids           # a list, in list order
    assert list(flat.sphere_ids(b, hs["bvh"])) == bvh_ids               # a BvhNode lists what its list lists
    assert list(flat.sphere_ids(b, hs["members"][0])) == bvh_ids        # a wrapper around it
    assert list(flat.sphere_ids(b, hs["members"][3])) == []             # a mesh holds none
    ground = 0
    assert list(flat.sphere_ids(b, case.world)) == [ground] + bvh_ids + group_ids + [id_of(hs["one"])]  # the instance tree, member by member
    # a medium around a sphere; a handle listed in the world list and in a BVH has ONE id
    fog = CASES["fog"](rtsr, False)
    fflat = fog.flatten()
    assert len(fflat.sphere_ids(fog.builder, fog.world)) == 5
    sh = CASES["shared"](rtsr, False)
    sflat = sh.flatten()
    both = int(sflat.sphere_ids(sh.builder, sh.handles["both"])[0])
    assert list(sflat.sphere_ids(sh.builder, sh.world)).count(both) == 2 and list(sflat.sphere_ids(sh.builder, sh.handles["bvh"]))[0] == both
    assert len(sflat.array("spheres")) // 40 == 8  # ground, `both` once, six more
    # moving spheres have no id and are skipped
    bm = beside_movers(rtsr, False)
    bflat = bm.flatten()
    assert len(bflat.sphere_ids(bm.builder, bm.handles["timed"])) == 1 and bflat.info()["n_moving_spheres"] == 3
    # an object made after the flatten; bad handles; NULLs; a cap smaller than the count
    with pytest.raises(rtsr.RtxError) as e:
        flat.sphere_ids(b, b.hittable_list([hs["one"]]))
    assert "after this flat scene was flattened" in str(e.value)
    assert rtsr.lib.rtx_flat_sphere_ids(flat.ptr, b.ptr, 10 ** 6, None, 0) == -1 and "handle" in rtsr.last_error()
    assert rtsr.lib.rtx_flat_sphere_ids(None, b.ptr, 0, None, 0) == -1
    assert rtsr.lib.rtx_flat_sphere_ids(flat.ptr, None, 0, None, 0) == -1
    out = (C.c_int32 * 2)(-7, -7)
    assert rtsr.lib.rtx_flat_sphere_ids(flat.ptr, b.ptr, hs["group"], out, 1) == 3 and out[0] == group_ids[0] and out[1] == -7


def test_every_refusal_leaves_the_flat_scene_unchanged(rtsr, orc):
    case = CASES["mixed"](rtsr, False)
    flat = case.flatten()
    before = _arrays(flat)
    n_ids = flat.info()["n_spheres"]
    cases = refusals(n_ids)
    assert len(cases) == 8
    for name, ids, n, vals, word, _ in cases:
        st = call_set_prims(rtsr, rtsr.lib.rtx_flat_set_spheres, flat.ptr, ids, n, vals)
        assert st == rtsr.RTX_EINVAL, name
        assert "rtx_flat_set_spheres" in rtsr.last_error() and word in rtsr.last_error(), (name, rtsr.last_error())
        assert _same_arrays(flat, before), name
    assert call_set_prims(rtsr, rtsr.lib.rtx_flat_set_spheres, None, [0], None, np.ones(4)) == rtsr.RTX_EINVAL and "scene is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, rtsr.lib.rtx_flat_set_spheres, flat.ptr, [0], 0, np.ones(4)) == rtsr.RTX_OK  # n = 0: nothing to do
    assert _same_arrays(flat, before)
    # a negative radius and a radius of zero are legal: rtx_sphere applies no rule to it
    two = flat.array("spheres").view(SPHERE)[:2]
    flat.set_spheres([0, 1], [[*two["c"][0], -abs(two["radius"][0])], [*two["c"][1], 0.0]])
    flat.set_spheres([0, 1], [[*two["c"][0], two["radius"][0]], [*two["c"][1], two["radius"][1]]])
    assert _same_arrays(flat, before)
    # a BVH that holds a MovingSphere: its time-aware slopes would have to be derived again; the field beside it still moves
    bm = beside_movers(rtsr, False)
    mflat = bm.flatten()
    mbefore = _arrays(mflat)
    bad = mflat.sphere_ids(bm.builder, bm.handles["timed_static"])
    with pytest.raises(rtsr.RtxError) as e:
        mflat.set_spheres(bad, [[0.9, 2.7, 5.1, 0.2]])
    assert e.value.status == rtsr.RTX_EUNSUPPORTED and "MovingSphere" in str(e.value) and "rtx_flat_set_spheres" in str(e.value)
    ids, vals = update_of(bm, mflat)
    with pytest.raises(rtsr.RtxError):
        mflat.set_spheres(np.concatenate([ids, bad]), np.concatenate([vals, [[0.9, 2.7, 5.1, 0.2]]]))  # one bad id refuses the whole call
    assert _same_arrays(mflat, mbefore)
    # the Python layer counts the values before the library sees them
    with pytest.raises(ValueError):
        flat.set_spheres([0, 1], np.ones(4))
    # a good update after all the refusals still goes through
    flat.set_spheres(*update_of(case, flat))
    assert not np.array_equal(flat.array("nodes"), before["nodes"])


def test_host_update_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/set_spheres_host_check.cpp with the flattener and the builder under -fsanitize=address,undefined: full and partial
    updates of sphere fields, a sphere light and an instance tree against a fresh flatten, a hand-made BVH whose root is a leaf
    code, the refusals.  A stand-alone CPU program; nothing is loaded into Python."""
    host = os.path.join(ROOT, "ray-tracing-series-rust_amd", "csrc", "host")
    exe = str(tmp_path / "set_spheres_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-pthread",
                    os.path.join(ROOT, "tests", "set_spheres_host_check.cpp"), os.path.join(host, "scene_graph.cpp"),
                    os.path.join(host, "flatten.cpp"), os.path.join(host, "bvh_build.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "set_spheres host check clean" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
