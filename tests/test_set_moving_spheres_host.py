"""rtx_flat_set_moving_spheres and rtx_flat_moving_sphere_ids on the CPU: new end centres and a radius for named MovingSpheres
of a flat scene, its BVHs and their time-aware boxes refitted bottom-up with their topology kept.

The judge is always the FRESH flat scene -- the same world built from scratch with the new values and flattened
(tests/mover_update_cases.py), whose boxes the flattener derives top-down -- and the oracle, never the code under test.  Every
test calls a symbol the library did not have before.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_py
from mover_update_cases import (CASES, FLAT_ARRAYS, INTERVALS, LDS_CASES, MOTION32, MOVER, NAN_CASES, NODE, NODE32, NO_TIME_BOXES, SLOPE_CASES,
                                book1_head, book1_update, cam_cfg, narrow, refusals, two_bvhs, update_of, with_gravity, wrapped)
from update_cases import assert_same_topology, call_set_prims, flat_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_ARRAYS = ("refs", "rects")  # no hook of the library's reads these: the oracle's view of the same FlatScene does
# the audit of the time-aware boxes knows spheres only (a BVH with triangles: 2) and finite centres (a mover whose own interval
# is empty has none: 3); on every other case it must return 0
AUDIT_MOTION = {"tri_mover": 2, "interval_degenerate": 3}


def _arrays(flat):
    return flat_arrays(flat, FLAT_ARRAYS, ORACLE_ARRAYS)


def _same_arrays(flat, first):
    now = _arrays(flat)
    return all(np.array_equal(now[k], first[k]) for k in first)


def _same_topology_as(now, judge):
    """The child codes, split axes and reference order the byte comparison relies on."""
    n, j = now["nodes"].view(NODE), judge["nodes"].view(NODE)
    return n.shape == j.shape and np.array_equal(n["child"], j["child"]) and np.array_equal(n["pad"], j["pad"]) and np.array_equal(now["refs"], judge["refs"])


def _slopes(arrays):
    """The axes along which any time-aware record has a slope, as a string."""
    mo = arrays["motion32"].view(MOTION32)
    return "".join("xyz"[a] for a in range(3) if (mo["dlo"][:, :, a] != 0).any() or (mo["dhi"][:, :, a] != 0).any())


def _check_against_fresh(orc, name, flat, fresh, first):
    """-> whether the fresh build chose the same topology (and the arrays were compared byte for byte)."""
    now, judge = _arrays(flat), _arrays(fresh)
    # movers by id: an id is the index in the moving-sphere array, and both builds emit the movers in the same order
    assert np.array_equal(now["moving_spheres"], judge["moving_spheres"])
    m, m0 = now["moving_spheres"].view(MOVER), first["moving_spheres"].view(MOVER)
    for f in ("time0", "time1", "mat", "pad"):
        assert np.array_equal(m[f], m0[f]), f
    # topology, and everything a mover's value does not reach, stay
    assert_same_topology(now, first, ("entries", "top_level", "triangles", "spheres", "top_box32", "member_local_box", "lights", "materials") + ORACLE_ARRAYS)
    rc, _ = orc.audit_flat_exact(flat.arrays_ptr(), ask_first=True)
    assert rc == 0
    assert orc.audit_motion(flat.arrays_ptr())[0] == AUDIT_MOTION.get(name, 0) == orc.audit_motion(fresh.arrays_ptr())[0]
    nodes, n32 = now["nodes"].view(NODE), now["nodes32"].view(NODE32)
    assert np.array_equal(n32["lo"], narrow(nodes["bmin"], up=False)) and np.array_equal(n32["hi"], narrow(nodes["bmax"], up=True))
    assert len(now["motion32"]) == len(judge["motion32"]) == len(first["motion32"])
    assert _slopes(now) == _slopes(judge)  # what k_trace_lds's instantiation is planned by
    same = _same_topology_as(now, judge)
    if same:
        for k in ("nodes", "nodes32", "motion32"):
            assert np.array_equal(now[k], judge[k]), k
    return same


def _frames(rtsr, orc, name, case, flat, fresh):
    """A 48 x 27 x 4 spp O2 frame of the updated scene equals O2 of the fresh one; so does the LDS walk's CPU restatement, with
    the time-aware boxes on and off, on the worlds k_trace_lds takes."""
    cam, cfg, h = cam_cfg(rtsr, case)
    assert (cfg.image_width, h, cfg.samples_per_pixel) == (48, 27, 4)
    a, a8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=4)
    f, f8 = orc.o2_render(fresh.arrays_ptr(), cam, cfg, h, threads=4)
    # (movers without a finite centre poison every path that meets one: that frame is what it is, and must still be the fresh one's)
    assert (f.std() > 0.01 or name in NAN_CASES) and np.array_equal(a, f, equal_nan=True) and np.array_equal(a8, f8)
    if name in LDS_CASES:
        for use_motion in ((True, False) if len(flat.array("motion32")) else (False,)):  # (no time-aware box: nothing to switch on)
            w, _ = orc.lds_walk_render(flat.arrays_ptr(), cam, cfg, h, use_motion, threads=4)
            assert np.array_equal(w, f), (name, use_motion)


@pytest.fixture(scope="module")
def census():
    return {}


@pytest.mark.parametrize("name", sorted(CASES))
def test_an_updated_flat_scene_is_the_freshly_built_one(rtsr, orc, census, name):
    case, moved = CASES[name](rtsr, False), CASES[name](rtsr, True)
    flat, fresh = case.flatten(), moved.flatten()
    first = _arrays(flat)
    ids, vals = update_of(case, flat)
    flat.set_moving_spheres(ids, vals)
    assert not np.array_equal(flat.array("moving_spheres"), first["moving_spheres"])
    if name not in ("one", "plain", "plain_overflow", "wrapped", "interval_degenerate"):  # (no node above a mover; boxes that hold no finite plane)
        assert not np.array_equal(flat.array("nodes"), first["nodes"])
    census[name] = _check_against_fresh(orc, name, flat, fresh, first)
    _frames(rtsr, orc, name, case, flat, fresh)
    # the way back to rest restores every byte
    flat.set_moving_spheres(*update_of(case, flat, moved=False))
    assert _same_arrays(flat, first)


def test_two_thirds_of_the_cases_were_compared_byte_for_byte(rtsr, orc, census):
    """The displacements are chosen so that the fresh build keeps the rest build's topology; where it does not, the audits, the
    top-down restatement (tests/set_moving_spheres_host_check.cpp) and the frames still judge the refit."""
    for name in sorted(set(CASES) - set(census)):  # (run alone: take the census here)
        case, moved = CASES[name](rtsr, False), CASES[name](rtsr, True)
        flat = case.flatten()
        flat.set_moving_spheres(*update_of(case, flat))
        census[name] = _same_topology_as(_arrays(flat), _arrays(moved.flatten()))
    assert 3 * sum(census.values()) >= 2 * len(CASES), sorted(k for k in census if not census[k])


def test_the_slope_transitions_show_in_the_time_aware_boxes(rtsr, orc):
    """What the slope mask is judged on: which axes carry a slope at rest and after the update."""
    want = {"y_only": ("y", "y"), "y_to_xy": ("y", "xy"), "xy_to_y": ("xy", "y"), "still": ("y", ""), "z_only": ("y", "z")}
    assert sorted(want) == sorted(SLOPE_CASES)
    for name, (rest, after) in want.items():
        case = CASES[name](rtsr, False)
        flat = case.flatten()
        assert _slopes(_arrays(flat)) == rest, name
        flat.set_moving_spheres(*update_of(case, flat))
        assert _slopes(_arrays(flat)) == after, name
    for which in INTERVALS:  # a BVH whose interval is not ordered gets no time-aware box at all, before or after
        case = CASES["interval_" + which](rtsr, False)
        flat = case.flatten()
        flat.set_moving_spheres(*update_of(case, flat))
        assert (len(flat.array("motion32")) == 0) == (which in NO_TIME_BOXES), which


@pytest.mark.parametrize("pattern", ["one of 40", "every 7th", "reversed", "two halves"])
def test_partial_updates_and_id_order(rtsr, orc, pattern):
    case = CASES["y_only"](rtsr, False)
    flat = case.flatten()
    first = _arrays(flat)
    n_all = len(case.parts)
    if pattern == "one of 40":
        sel, upd = (lambda k: k == 5), [update_of(case, flat, only=5)]
    elif pattern == "every 7th":
        sel, upd = (lambda k: k % 7 == 0), [update_of(case, flat, every=7)]
    elif pattern == "reversed":
        sel, upd = True, [update_of(case, flat, reverse=True)]
        assert list(upd[0][0]) == sorted(upd[0][0], reverse=True)
    else:
        ids, vals = update_of(case, flat)
        sel, upd = True, [(ids[:n_all // 2], vals[:n_all // 2]), (ids[n_all // 2:], vals[n_all // 2:])]
    for ids, vals in upd:
        assert 0 < len(ids) <= n_all
        flat.set_moving_spheres(ids, vals)
    fresh = CASES["y_only"](rtsr, sel).flatten()
    _check_against_fresh(orc, "y_only", flat, fresh, first)
    _frames(rtsr, orc, "y_only", case, flat, fresh)


def test_only_the_named_bvh_is_written(rtsr, orc):
    case = two_bvhs(rtsr, False)
    flat = case.flatten()
    first = _arrays(flat)
    flat.set_moving_spheres(*update_of(case, flat))
    now = _arrays(flat)
    n, n0 = now["nodes"].view(NODE), first["nodes"].view(NODE)
    changed = np.array([n[i].tobytes() != n0[i].tobytes() for i in range(len(n))])
    n_first = len(case.parts) - 1  # a BVH of k one-primitive leaves has k - 1 nodes, and the builder appends a tree in one piece
    assert changed[:n_first].any() and not changed[n_first:].any()
    for k in ("nodes32", "motion32"):
        rec = len(now[k]) // len(n)
        assert np.array_equal(now[k][n_first * rec:], first[k][n_first * rec:]), k


def test_book1_at_head_refits_exactly_and_returns_to_rest(rtsr, orc):
    """Catalogue scene 13, all movers moved: the catalogue builds it from its own random stream, so there is no second build
    with other values; the judges are the oracle's audits, the untouched topology, the slopes and the way back."""
    b, world, cam, bg = book1_head(rtsr)
    flat = b.flatten(world)
    first = _arrays(flat)
    ids, rest, mv = book1_update(flat, b, world)
    assert len(ids) > 300 and _slopes(first) == "y"
    flat.set_moving_spheres(ids, mv)
    now = _arrays(flat)
    assert orc.audit_flat_exact(flat.arrays_ptr(), ask_first=True)[0] == 0 and orc.audit_motion(flat.arrays_ptr())[0] == 0
    assert_same_topology(now, first, ("entries", "top_level", "spheres") + ORACLE_ARRAYS)
    mov = now["moving_spheres"].view(MOVER)
    assert np.array_equal(np.column_stack([mov["c0"][ids], mov["c1"][ids], mov["radius"][ids]]), mv)
    assert not np.array_equal(now["motion32"], first["motion32"]) and _slopes(now) == "y"
    flat.set_moving_spheres(ids, book1_update(flat, b, world, axes="xy")[2])
    assert _slopes(_arrays(flat)) == "xy" and orc.audit_motion(flat.arrays_ptr())[0] == 0
    flat.set_moving_spheres(ids, rest)
    assert _same_arrays(flat, first)


def test_moving_sphere_ids_on_every_kind_of_handle(rtsr):
    case = wrapped(rtsr, False)
    b, flat = case.builder, case.flatten()
    mov = flat.array("moving_spheres").view(MOVER)
    for h, rest, _ in case.parts:  # a mover's handle: its own id, and the record holds its values
        ids = flat.moving_sphere_ids(b, h)
        assert ids.dtype == np.int32 and len(ids) == 1
        assert np.array_equal(np.array([*mov["c0"][ids[0]], *mov["c1"][ids[0]], mov["radius"][ids[0]]]), rest)
    every = [int(flat.moving_sphere_ids(b, h)[0]) for h, _, _ in case.parts]
    assert list(flat.moving_sphere_ids(b, case.world)) == every and len(every) == 5  # a list: wrappers, a medium and a group, in list order
    two = two_bvhs(rtsr, False)
    tflat = two.flatten()
    in_first = [int(tflat.moving_sphere_ids(two.builder, h)[0]) for h, _, _ in two.parts]
    assert list(tflat.moving_sphere_ids(two.builder, two.handles["first"])) == in_first  # a BvhNode lists what its list lists
    assert len(tflat.moving_sphere_ids(two.builder, two.handles["second"])) == 5 and tflat.info()["n_moving_spheres"] == 11
    ground = two.builder.sphere((0.0, 0.0, 0.0), 1.0, two.builder.lambertian((0.5, 0.5, 0.5)))
    assert len(flat.sphere_ids(b, case.world)) == 2 and len(flat.moving_sphere_ids(b, case.parts[0][0])) == 1
    plain_sphere = CASES["plain"](rtsr, False)
    pflat = plain_sphere.flatten()
    assert len(pflat.moving_sphere_ids(plain_sphere.builder, plain_sphere.world)) == 3
    static_only = rtsr.Builder(3)
    s = static_only.sphere((0.0, 0.0, 0.0), 1.0, static_only.lambertian((0.5, 0.5, 0.5)))
    assert list(static_only.flatten(s).moving_sphere_ids(static_only, s)) == []  # an object without movers gives 0
    # an object made after the flatten; bad handles; NULLs; a cap smaller than the count
    with pytest.raises(rtsr.RtxError) as e:
        tflat.moving_sphere_ids(two.builder, ground)
    assert "after this flat scene was flattened" in str(e.value)
    assert rtsr.lib.rtx_flat_moving_sphere_ids(flat.ptr, b.ptr, 10 ** 6, None, 0) == -1 and "handle" in rtsr.last_error()
    assert rtsr.lib.rtx_flat_moving_sphere_ids(None, b.ptr, 0, None, 0) == -1
    assert rtsr.lib.rtx_flat_moving_sphere_ids(flat.ptr, None, 0, None, 0) == -1
    out = (C.c_int32 * 2)(-7, -7)
    assert rtsr.lib.rtx_flat_moving_sphere_ids(flat.ptr, b.ptr, case.world, out, 1) == 5 and out[0] == every[0] and out[1] == -7


def test_every_refusal_leaves_the_flat_scene_unchanged(rtsr, orc):
    case = with_gravity(rtsr, False)
    flat = case.flatten()
    before = _arrays(flat)
    fn = rtsr.lib.rtx_flat_set_moving_spheres
    cases = refusals(flat.info()["n_moving_spheres"])
    assert len(cases) == 8
    for name, ids, n, vals, word, _ in cases:  # the ladder's first rung, in its order
        assert call_set_prims(rtsr, fn, flat.ptr, ids, n, vals) == rtsr.RTX_EINVAL, name
        assert "rtx_flat_set_moving_spheres" in rtsr.last_error() and word in rtsr.last_error(), (name, rtsr.last_error())
        assert _same_arrays(flat, before), name
    assert call_set_prims(rtsr, fn, None, [0], None, np.ones(7)) == rtsr.RTX_EINVAL and "scene is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, flat.ptr, [0], 0, np.ones(7)) == rtsr.RTX_OK  # n = 0: nothing to do
    assert _same_arrays(flat, before)
    # an id out of range is named before the GravitySphere is (RTX_EINVAL comes first)
    bad = flat.moving_sphere_ids(case.builder, case.handles["bad"])
    assert call_set_prims(rtsr, fn, flat.ptr, [int(bad[0]), 99], None, np.ones(14)) == rtsr.RTX_EINVAL
    # a mover inside a BVH that also holds a GravitySphere: the message says why; one such id refuses the whole call
    with pytest.raises(rtsr.RtxError) as e:
        flat.set_moving_spheres(bad, [[4.2, 1.1, 2.1, 4.5, 1.5, 2.3, 0.3]])
    assert e.value.status == rtsr.RTX_EUNSUPPORTED and "GravitySphere" in str(e.value) and "not linear in time" in str(e.value)
    assert "height table" in str(e.value) and "rtx_flat_set_moving_spheres" in str(e.value)
    ids, vals = update_of(case, flat)
    with pytest.raises(rtsr.RtxError):
        flat.set_moving_spheres(ids, vals)
    assert _same_arrays(flat, before)
    # the BVH of movers alone beside it still updates
    n_clean = case.handles["n_clean"]
    flat.set_moving_spheres(ids[:n_clean], vals[:n_clean])
    assert not np.array_equal(flat.array("nodes"), before["nodes"])
    flat.set_moving_spheres(ids[:n_clean], update_of(case, flat, moved=False)[1][:n_clean])
    assert _same_arrays(flat, before)
    # set_spheres and set_triangles keep refusing a BVH that holds a mover
    mixed = CASES["mixed5_leaf1"](rtsr, False)
    mflat = mixed.flatten()
    with pytest.raises(rtsr.RtxError) as e:
        mflat.set_spheres([1], [[1.3, 0.9, 2.1, 0.2]])
    assert e.value.status == rtsr.RTX_EUNSUPPORTED and "MovingSphere" in str(e.value)
    # the Python layer counts the values before the library sees them
    with pytest.raises(ValueError):
        flat.set_moving_spheres([0, 1], np.ones(7))


def _build_host_check(tmp_path, sanitize):
    host = os.path.join(ROOT, "ray-tracing-series-rust_amd", "csrc", "host")
    exe = str(tmp_path / ("set_moving_spheres_host_check" + ("_san" if sanitize else "")))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-omit-frame-pointer"] + flags +
                   ["-Wall", "-Wno-unused-function", "-pthread", os.path.join(ROOT, "tests", "set_moving_spheres_host_check.cpp"),
                    os.path.join(host, "scene_graph.cpp"), os.path.join(host, "flatten.cpp"), os.path.join(host, "bvh_build.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_top_down_rule_restated_agrees_with_the_refit(tmp_path, sanitize):
    """tests/set_moving_spheres_host_check.cpp, plain and with the flattener and the builder under -fsanitize=address,undefined:
    full and partial updates against a fresh flatten and against motion_box_at's rule written out again on the UPDATED topology,
    every motion32 record bit for bit; a hand-made BVH whose root is a leaf code; the refusals.  A stand-alone CPU program;
    nothing is loaded into Python."""
    exe = _build_host_check(tmp_path, sanitize)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "set_moving_spheres host check clean" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
