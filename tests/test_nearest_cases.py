"""Nearest-point queries on the CPU (core/nearest.hpp through tests/nearest_host_check.cpp): closed forms judge prim_nearest and
the transforms, the exhaustive scan judges the culled walk bit for bit, the counters show that culling saves work.  Scenes, points
and judges: tests/nearest_cases.py."""
import numpy as np
import pytest

import nearest_cases as nc

PRECISIONS = pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])


@pytest.fixture(scope="module")
def chk(rtsr, orc, tmp_path_factory):
    return nc.checkers(tmp_path_factory)


# ---- judge 1
@PRECISIONS
def test_closed_forms(rtsr, chk, f32):
    names = []
    for c in nc.closed_form_cases(rtsr, f32):
        for exhaustive in (False, True):
            got = nc.host(chk, c.flat, c.points, c.time, c.r_max, media=c.media, f32=f32, exhaustive=exhaustive)
            ed, eq, tol = nc.check_closed(c, got, f32)
            print("%s (%s): |d| error %.3g, |q| error %.3g, tolerance %.3g" % (c.name, "exhaustive" if exhaustive else "culled", ed, eq, tol))
            assert ed <= tol and eq <= tol, (c.name, ed, eq, tol)
        names.append(c.name)
    assert len(names) == len(set(names)) >= 17


def test_a_medium_boundary_reports_the_phase_material(rtsr, chk):
    b = rtsr.Builder(1)
    ball = b.sphere((0.0, 0.0, 0.0), 1.0, b.lambertian((0.5, 0.5, 0.5)))
    flat = b.flatten(b.hittable_list([b.constant_medium((0.8, 0.8, 0.8), 0.4, ball), b.translate((5.0, 0.0, 0.0), ball)]))
    p = np.array([[0.0, 2.0, 0.0], [5.0, 2.0, 0.0]])
    off = nc.host(chk, flat, p, media=False)
    on = nc.host(chk, flat, p, media=True)
    assert list(off.ids[:, 1]) == [1, 1] and list(on.ids[:, 1]) == [0, 1]
    assert on.ids[0, 0] != on.ids[1, 0] and on.ids[1, 0] == off.ids[1, 0]  # the phase material, not the boundary's own
    assert flat.material(int(on.ids[0, 0]))["kind"] == "isotropic"


# ---- judge 2 and judge 3
@PRECISIONS
@pytest.mark.parametrize("name", list(nc.SCENES))
def test_culled_walk_equals_the_exhaustive_scan(rtsr, chk, name, f32):
    c = nc.case(rtsr, name)
    info = c.flat.info()
    for media in (False, True):
        full = nc.host(chk, c.flat, c.points, c.time, media=media, f32=f32, exhaustive=True)
        r_fin = nc.finite_r_max(full)
        for r_max_all in (nc.INF, r_fin):
            ref = full if r_max_all == nc.INF else nc.host(chk, c.flat, c.points, c.time, r_max_all=r_max_all, media=media, f32=f32, exhaustive=True)
            got = nc.host(chk, c.flat, c.points, c.time, r_max_all=r_max_all, media=media, f32=f32)
            bad = nc.differing(got, ref)
            share = float(ref.found.mean())
            print("%s media=%d r_max=%g: %d points, %.0f %% found, primitive tests %d culled / %d exhaustive (%.4f), %d box tests, %d differ" %
                  (name, media, r_max_all, len(c.points), 100 * share, got.prim_tests, ref.prim_tests,
                   got.prim_tests / max(ref.prim_tests, 1), got.box_tests, len(bad)))
            assert len(bad) == 0, (name, int(bad[0]), got.d[bad[0]], ref.d[bad[0]], got.ids[bad[0]], ref.ids[bad[0]])
            if r_max_all != nc.INF:
                assert 0.1 <= share <= 0.9, (name, share)
            # judge 3: a scene with a BVH of more than 64 primitives must save primitive tests
            if (nc.bvh_ref_counts(c.flat) > 64).any():
                assert got.prim_tests < ref.prim_tests, (name, got.prim_tests, ref.prim_tests)
        # conditions on the exhaustive scan's own answers: every kind of primitive the scene holds wins at least once
        if media:
            kinds = set(full.ids[full.found, 2].tolist())
            held = {k for k, n in ((nc.PRIM_SPHERE, info["n_spheres"]), (nc.PRIM_MOVING_SPHERE, info["n_moving_spheres"]), (nc.PRIM_RECT, info["n_rects"]), (nc.PRIM_TRIANGLE, info["n_triangles"])) if n}
            assert held <= kinds, (name, held, kinds)
            if name in nc.ZOOS:
                trees = [c.flat.instance_tree(k) for k in range(c.flat.instances()["n_trees"])]
                members = {s for t in trees for s in range(t["first_slot"], t["first_slot"] + t["n_slots"])}
                winners = members & set(full.ids[full.found, 1].tolist())
                assert 2 * len(winners) >= len(members), (name, len(winners), len(members))


def check_tie_winners(rtsr, chk, kind, f32=False):
    """The ids the key's tie rule gives on the mirrored pairs: at top level slot 0; inside one BVH the primitive at the LOWER
    position of the BVH's ref list, read from the flat arrays (nearest_cases.slot_refs), whichever half of the pair that is."""
    c = nc.case(rtsr, "tie_%s_list" % kind)
    got = nc.host(chk, c.flat, c.points, f32=f32)
    assert np.all(got.ids[:, 1] == 0) and np.all(got.q[:, 0] < 0), c.name  # slot 0 is the pair's -x half
    in_bvh = nc.case(rtsr, "tie_%s_bvh" % kind)
    tied = nc.host(chk, in_bvh.flat, in_bvh.points, f32=f32)
    assert np.array_equal(tied.d, got.d), in_bvh.name  # the same pair: the same distances, bit for bit
    refs = nc.slot_refs(chk, in_bvh.flat, 0)
    kind_id = nc.PRIM_SPHERE if kind == "spheres" else nc.PRIM_TRIANGLE
    assert len(refs) == 4 and np.all(refs[:, 0] == kind_id)
    # which two refs are the pair: the winners of points next to either half (no tie there)
    probe = np.array([[-2.0, 0.5, 0.25], [2.0, 0.5, 0.25]]) if kind == "spheres" else np.array([[-2.0, 0.3, 1.2], [2.0, 0.3, 1.2]])
    pair = nc.host(chk, in_bvh.flat, probe, f32=f32, exhaustive=True).ids[:, 3]
    assert pair[0] != pair[1] and np.all(nc.host(chk, in_bvh.flat, probe, f32=f32, exhaustive=True).q[:, 0] * [-1, 1] > 0)
    position = {int(i): int(np.flatnonzero(refs[:, 1] == i)[0]) for i in pair}
    lower = min(pair, key=lambda i: position[int(i)])
    assert np.all(tied.ids[:, 2] == kind_id) and np.all(tied.ids[:, 3] == lower), (in_bvh.name, position, set(tied.ids[:, 3].tolist()))
    side = -1.0 if lower == pair[0] else 1.0
    assert np.all(tied.q[:, 0] * side > 0), in_bvh.name


@PRECISIONS
@pytest.mark.parametrize("kind", ["spheres", "triangles"])
def test_exact_ties_go_to_the_lower_slot_and_ref(rtsr, chk, kind, f32):
    for name in ("tie_%s_list" % kind, "tie_%s_bvh" % kind):
        c = nc.case(rtsr, name)
        assert len(nc.differing(nc.host(chk, c.flat, c.points, f32=f32), nc.host(chk, c.flat, c.points, f32=f32, exhaustive=True))) == 0
    check_tie_winners(rtsr, chk, kind, f32)


@PRECISIONS
def test_the_second_leaf_is_judged_against_the_current_bound(rtsr, chk, f32):
    """Judge 3 on a scene where the count is known by reasoning (nearest_cases.two_leaves): one primitive test a point."""
    c = nc.two_leaves(rtsr)
    got = nc.host(chk, c.flat, c.points, f32=f32)
    assert np.all(got.ids[:, 3] == 0) and got.prim_tests == len(c.points), (got.prim_tests, len(c.points))
    assert nc.host(chk, c.flat, c.points, f32=f32, exhaustive=True).prim_tests == 2 * len(c.points)


@pytest.mark.parametrize("name", ["tie_spheres_bvh", "tie_triangles_bvh", "mesh_room"])
def test_the_answer_does_not_depend_on_the_build(rtsr, chk, name):
    """Under every leaf size and builder the culled walk equals the exhaustive scan of THAT build bit for bit, and d is the same
    bytes across builds.  On mesh_room material, slot and kind are the same too, and so is the index of every winner that is not
    a triangle.  What is NOT the same bytes across builds is the winner among triangles that tie exactly: the builder orders a
    BVH's ref list (and stores the triangles in that order), the key's `order` IS the ref position, and a point next to a mesh
    vertex or edge ties between the triangles that share it.  They name the same geometric point, each through its own
    barycentric arithmetic: q is held to 64 ulps at the scene's magnitude across builds, and is the same bytes wherever the
    same triangle (by Flat.array("triangle_id")) wins."""
    base = nc.case(rtsr, name)
    pts = base.points[:300]

    def tri_id(flat, ans):
        table = np.frombuffer(flat.array("triangle_id"), dtype=np.int32)
        return np.where(ans.ids[:, 2] == nc.PRIM_TRIANGLE, table[np.clip(ans.ids[:, 3], 0, len(table) - 1)], -1)
    ref = nc.host(chk, base.flat, pts)
    builds = [dict(max_leaf=k) for k in range(1, 9)] + [dict(reference_bvh=True)]
    for kw in builds:
        flat = base.builder.flatten(base.world, **kw)
        got = nc.host(chk, flat, pts)
        exh = nc.host(chk, flat, pts, exhaustive=True)
        assert len(nc.differing(got, exh)) == 0, (name, kw)
        assert np.array_equal(got.d, ref.d), (name, kw)
        if not name.startswith("tie"):
            assert np.array_equal(got.ids[:, :3], ref.ids[:, :3]), (name, kw)
            other = ref.ids[:, 2] != nc.PRIM_TRIANGLE
            assert other.any() and np.array_equal(got.ids[other, 3], ref.ids[other, 3]), (name, kw)
            same_tri = ~other & (tri_id(flat, got) == tri_id(base.flat, ref))
            assert same_tri.any() and np.array_equal(got.q[other | same_tri], ref.q[other | same_tri]), (name, kw)
            assert np.abs(got.q - ref.q).max() <= 64 * 2.0 ** -52 * np.abs(pts).max(), (name, kw)
