"""Instance trees on the CPU: rtx_instance_bvh_from_list is the HittableList of its members, culled by their true boxes.

The one invariant: a world spelled with an instance tree gives, bit for bit, the frame of the same world with the members written
into the world list at that position (the "hoisted" spelling), which O1 -- the literal oracle, which never sees the new node --
and O2 already agree on.  Every test here fails on a tree without the constructor.
"""
import numpy as np
import pytest

from instance_scenes import box_field, field_cam_cfg, tie_cam_cfg, tie_scene

ENTRY_PRIM, ENTRY_GROUP, ENTRY_BVH, ENTRY_XFORM = 0, 1, 2, 3


@pytest.mark.parametrize("max_leaf", [0, 1, 4])
def test_o2_instanced_equals_hoisted_equals_o1(rtsr, orc, max_leaf):
    """N = 60 at 120 x 80 x 16 spp: O2(instanced flat) == O2(hoisted flat) == O1(hoisted graph), for the default leaf size and
    max_leaf 1 and 4, three thread counts and three shards reassembled."""
    cam, cfg, h = field_cam_cfg(rtsr)
    assert (cfg.image_width, h, cfg.samples_per_pixel) == (120, 80, 16)
    bh, wh = box_field(rtsr, "hoisted")
    o1, _ = orc.o1_render(bh.graph_ptr(), wh, cam, cfg, h, threads=8)
    assert o1.std() > 0.01
    fh = bh.flatten(wh, max_leaf=max_leaf)
    bi, wi = box_field(rtsr, "instanced")
    fi = bi.flatten(wi, max_leaf=max_leaf)
    assert fi.instances()["n_trees"] == 1 and fi.instances()["n_members"] == 61
    assert fi.top_level_kinds() == fh.top_level_kinds()
    hoisted, hoisted8 = orc.o2_render(fh.arrays_ptr(), cam, cfg, h, threads=8)
    assert np.array_equal(hoisted, o1)
    for threads in (1, 3, 8):
        inst, inst8 = orc.o2_render(fi.arrays_ptr(), cam, cfg, h, threads=threads)
        bad = int((inst != hoisted).any(axis=2).sum())
        assert bad == 0, "max_leaf %d, %d threads: %d pixels differ from the hoisted spelling" % (max_leaf, threads, bad)
        assert np.array_equal(inst8, hoisted8)
    whole = np.zeros_like(hoisted)
    for s in range(3):
        part, _ = orc.o2_render(fi.arrays_ptr(), cam, cfg, h, shard=(s, 3, 1), threads=4)
        whole[[j for j in range(h) if j % 3 == s]] = part
    assert np.array_equal(whole, hoisted)


def test_exact_ties_go_to_the_later_member_whatever_the_walk_order(rtsr, orc):
    """Two prisms whose top faces coincide where they overlap: the list [A, B] shows B there, [B, A] shows A.  An instance tree
    meets its members in tree order and must still give the list's answer, in both orders."""
    cam, cfg, h = tie_cam_cfg(rtsr)
    o1 = {}
    for order in ("AB", "BA"):
        b, w = tie_scene(rtsr, order, "list")
        o1[order], _ = orc.o1_render(b.graph_ptr(), w, cam, cfg, h, threads=4)
    differ = int((o1["AB"] != o1["BA"]).any(axis=2).sum())
    print("the two list orders differ in %d of %d pixels" % (differ, h * cfg.image_width))
    assert differ > 20  # the overlap is in view: the test is not vacuous
    for order in ("AB", "BA"):
        b, w = tie_scene(rtsr, order, "instanced")
        flat = b.flatten(w)
        assert flat.instances()["n_trees"] == 1
        got, _ = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=4)
        assert np.array_equal(got, o1[order]), "order %s: %d pixels differ" % (order, int((got != o1[order]).any(axis=2).sum()))


def test_a_rotated_member_is_hit_outside_its_unrotated_box(rtsr, orc):
    """The ray of test_rotate_y_keeps_the_unrotated_box_and_a_bvh_culls_by_it, which a BvhNode of the rotated prism misses
    because RotateY keeps the un-rotated box: the instance tree of that member (plus a far sphere) hits, with the t and the
    normal of the bare member."""
    b = rtsr.Builder(1)
    grey = b.lambertian((0.5, 0.5, 0.5))
    rot = b.rotate_y(45.0, b.rect_prism((-1.0, 0.0, -1.0), (1.0, 1.0, 1.0), grey))
    far = b.sphere((50.0, 0.0, 50.0), 1.0, grey)
    o, d = (1.2, 5.0, 0.05), (0.001, -1.0, 0.002)
    bare = orc.o1_hit(b.graph_ptr(), rot, o, d)
    assert bare is not None and bare["p"][0] > 1.0
    assert orc.o1_hit(b.graph_ptr(), b.bvh_from_list(b.hittable_list([rot]), 0.0, 1.0), o, d) is None
    flat = b.flatten(b.hittable_list([b.instance_bvh(b.hittable_list([rot, far]))]))
    assert flat.instances()["n_trees"] == 1
    got = orc.core_world_hit(flat.arrays_ptr(), o, d)
    assert got is not None
    assert got["t"] == bare["t"] and tuple(got["normal"]) == tuple(bare["normal"]) and tuple(got["p"]) == tuple(bare["p"])


def test_the_tree_culls_a_grid_of_1024_boxes(rtsr, orc):
    """O2's work counters at N = 1024 (32 x 32): the hoisted scan tests all 6 N rectangles for every ray, a ray through the
    tree only those of the cells it crosses -- at most about 64 of 1024.  Cap: one tenth (a cap, not a target; the measured
    ratio is printed and recorded in DESIGN.md 8.1).  samples, rays and scatters do not depend on the spelling."""
    n = 1024
    cam, cfg, h = field_cam_cfg(rtsr, n=n, width=48, spp=2, depth=12)
    bh, wh = box_field(rtsr, "hoisted", n=n)
    bi, wi = box_field(rtsr, "instanced", n=n)
    fi = bi.flatten(wi)
    info = fi.instances()
    assert info["n_trees"] == 1 and info["n_members"] == n + 1 and info["n_nodes"] == n and info["max_depth"] >= 10
    fh = bh.flatten(wh)
    ha, _, hc = orc.o2_render(fh.arrays_ptr(), cam, cfg, h, threads=8, counters=True)
    ia, _, ic = orc.o2_render(fi.arrays_ptr(), cam, cfg, h, threads=8, counters=True)
    assert np.array_equal(ia, ha)
    for name in ("samples", "rays", "scatters"):
        assert ic[name] == hc[name], name
    per_ray_h, per_ray_i = hc["rect_tests"] / hc["rays"], ic["rect_tests"] / ic["rays"]
    print("rect tests per ray: hoisted %.1f, instanced %.2f (ratio %.5f); box tests per ray: hoisted %.1f, instanced %.1f"
          % (per_ray_h, per_ray_i, per_ray_i / per_ray_h, hc["box_tests"] / hc["rays"], ic["box_tests"] / ic["rays"]))
    assert per_ray_h >= 6 * n
    assert per_ray_i <= 0.1 * per_ray_h


def _refused(rtsr, b, world, *words):
    with pytest.raises(rtsr.RtxError) as e:
        b.flatten(world)
    assert e.value.status == rtsr.RTX_EUNSUPPORTED
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_refusals_name_the_cause_and_the_spelling_that_works(rtsr):
    b = rtsr.Builder(1)
    grey = b.lambertian((0.5, 0.5, 0.5))
    s = b.sphere((0.0, 0.0, 0.0), 1.0, grey)
    s2 = b.sphere((3.0, 0.0, 0.0), 1.0, grey)
    tree = b.instance_bvh(b.hittable_list([s, s2]))
    _refused(rtsr, b, b.hittable_list([b.instance_bvh(b.hittable_list([b.constant_medium((1.0, 1.0, 1.0), 0.1, s), s2]))]),
             "ConstantMedium", "hit.rs:955-986", "visiting order", "world list")
    moving = b.moving_sphere((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.0, 1.0, 0.5, grey)
    _refused(rtsr, b, b.hittable_list([b.instance_bvh(b.hittable_list([b.translate((1.0, 0.0, 0.0), moving), s2]))]),
             "MovingSphere", "time interval", "world list")
    _refused(rtsr, b, b.hittable_list([b.instance_bvh(b.hittable_list([b.bvh_from_list(b.hittable_list([moving, s]), 0.0, 1.0), s2]))]),
             "MovingSphere", "time interval")
    _refused(rtsr, b, b.hittable_list([b.instance_bvh(b.hittable_list([b.gravity_sphere((0.0, 3.0, 0.0), 0.0, 0.5, grey), s2]))]),
             "GravitySphere", "time interval")
    _refused(rtsr, b, b.hittable_list([b.instance_bvh(b.hittable_list([tree, s2]))]), "INSIDE an instance tree", "outer list")
    _refused(rtsr, b, b.hittable_list([b.translate((1.0, 0.0, 0.0), tree)]), "UNDER a Translate", "Wrap the members")
    _refused(rtsr, b, b.hittable_list([b.rotate_y(10.0, tree)]), "UNDER a Translate", "Wrap the members")
    _refused(rtsr, b, b.hittable_list([b.constant_medium((1.0, 1.0, 1.0), 0.1, tree)]), "UNDER a Translate", "ConstantMedium")
    _refused(rtsr, b, b.hittable_list([b.bvh_from_list(b.hittable_list([tree, s2]), 0.0, 1.0)]), "INSIDE a BvhNode", "world list")
    # a BvhNode of wrapped members stays refused exactly as it was
    _refused(rtsr, b, b.bvh_from_list(b.hittable_list([b.rotate_y(20.0, s), s2]), 0.0, 1.0), "instanced sub-tree", "hit.rs:886")


def test_counts_small_trees_and_two_trees(rtsr, orc):
    b = rtsr.Builder(1)
    grey, red = b.lambertian((0.5, 0.5, 0.5)), b.lambertian((0.8, 0.2, 0.2))
    ground = b.sphere((0.0, -100.5, 0.0), 100.0, grey)
    left = [b.translate((-2.0 + 0.6 * k, 0.0, 0.0), b.rotate_y(10.0 * k, b.rect_prism((-0.2, -0.5, -0.2), (0.2, 0.3, 0.2), red))) for k in range(5)]
    right = [b.sphere((0.5 + 0.5 * k, 0.0, -1.0), 0.25, grey) for k in range(3)] + [b.rect_prism((2.0, -0.5, 0.0), (2.4, 0.2, 0.4), red)]
    nested = b.hittable_list([left[3], left[4]])  # a list member is spliced in
    one = b.sphere((0.0, 1.0, 0.0), 0.3, red)
    spelled = b.hittable_list([b.instance_bvh(b.hittable_list(left[:3] + [nested])), ground, b.instance_bvh(b.hittable_list([])),
                               b.instance_bvh(b.hittable_list([one])),
                               b.hittable_list([b.instance_bvh(b.hittable_list(right))])])  # a tree in a list nested in the world
    plain = b.hittable_list(left + [ground, one] + right)
    fi, fp = b.flatten(spelled), b.flatten(plain)
    assert fi.instances() == {"n_trees": 2, "n_members": 9, "n_nodes": 7, "max_depth": fi.instances()["max_depth"]}
    assert 2 <= fi.instances()["max_depth"] <= 4
    assert fp.instances() == {"n_trees": 0, "n_members": 0, "n_nodes": 0, "max_depth": 0}
    assert fi.top_level_kinds() == fp.top_level_kinds() == [ENTRY_XFORM] * 5 + [ENTRY_PRIM] * 5 + [ENTRY_GROUP]
    assert fi.info()["n_top_level"] == 11 and fi.info()["n_entries"] == fp.info()["n_entries"] + 3  # two records and the end mark
    assert orc.audit_flat(fi.arrays_ptr())[0] == 0
    cam = rtsr.Camera.new((0.5, 1.5, 5.0), (0.3, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 1.5, 0.0, 5.0, 0.0, 1.0)
    cfg = rtsr.Config.new(1.5, 72, 8, 12, 4, seed=3, background=(0.7, 0.8, 1.0))
    h = rtsr.image_height(cfg)
    o1, _ = orc.o1_render(b.graph_ptr(), plain, cam, cfg, h, threads=4)
    got, _ = orc.o2_render(fi.arrays_ptr(), cam, cfg, h, threads=4)
    assert np.array_equal(got, o1)
    # the world itself may be an instance tree, and a tree of nothing is an empty world
    alone = b.flatten(b.instance_bvh(b.hittable_list(right)))
    assert alone.instances()["n_trees"] == 1 and alone.info()["n_top_level"] == 4
    assert b.flatten(b.instance_bvh(b.hittable_list([]))).info()["n_top_level"] == 0
    with pytest.raises(rtsr.RtxError):
        b.instance_bvh(one)  # not a list


def test_f32_oracle_instanced_equals_hoisted(rtsr, orc):
    """The float build of the shared core walks the same trees: O2f(instanced) == O2f(hoisted), bit for bit."""
    cam, cfg, h = field_cam_cfg(rtsr, width=60, spp=4)
    bh, wh = box_field(rtsr, "hoisted")
    bi, wi = box_field(rtsr, "instanced")
    fh, fi = bh.flatten(wh), bi.flatten(wi)
    hoisted, hoisted8 = orc.o2f_render(fh.arrays_ptr(), cam, cfg, h, threads=8)
    inst, inst8 = orc.o2f_render(fi.arrays_ptr(), cam, cfg, h, threads=8)
    assert hoisted.std() > 0.01
    assert np.array_equal(inst, hoisted) and np.array_equal(inst8, hoisted8)
