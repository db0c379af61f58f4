"""What the literal oracle O1 makes of an instanced sub-tree: a BvhNode whose members are Translate / RotateY wrappers.

DESIGN.md section 8 said "O1 handles it"; nothing pinned it.  These tests do, on the CPU, and they are why such a node still
flattens to RTX_EUNSUPPORTED:

  * Translate members: Translate::bounding_box is the child's box moved by the offset (hit.rs:824-832), it holds the moved
    object, and O1's image of BvhNode(members) is the image of the same members listed in the world list, bit for bit, whatever
    the random split axes of its tree (bvh.rs:24).
  * RotateY members: RotateY::new computes the eight rotated corners and then stores the child's UN-rotated box
    (hit.rs:857-886: `bbox: Some(bbox)` names the shadowed child box; oracle/o1_literal.cpp restates it).  BvhNode::hit culls by
    the union box of its two children (bvh.rs:99), so the part of a rotated member outside its un-rotated box is visible only to
    rays that happen to cross the box of a neighbour in the same sub-tree.  The image depends on the tree: O1 gives a different
    frame per bvh_seed, none equal to the hoisted spelling.  There is no one image of the reference's for a culling structure of
    ours to reproduce -- the reason a ConstantMedium member is refused, for another cause (the number of draws of hit.rs:969
    depends on the visiting order).
The flattener's message for each shape says so (the last test: it fails before this change).
"""
import numpy as np
import pytest


def _box_field(rtsr, spelling, rotate, n=60):
    """A ground sphere, a lamp, and n boxes + 12 spheres either in ONE BvhNode ("instanced") or every wrapped box as its own slot
    of the world list beside a BvhNode of the spheres ("hoisted").  No two surfaces coincide (per-box offsets)."""
    b = rtsr.Builder(7)
    m = [b.lambertian((0.8, 0.3, 0.3)), b.metal((0.8, 0.8, 0.9), 0.3), b.lambertian((0.2, 0.7, 0.3)), b.lambertian((0.3, 0.3, 0.8))]
    members = []
    for k in range(n):
        w = 0.25 + 0.013 * (k % 7)
        box = b.rect_prism((-w, 0.0, -w), (w, 0.3 + 0.05 * (k % 5), w), m[k % 4])
        inner = b.rotate_y(7.0 + 5.3 * k, box) if rotate else box
        members.append(b.translate((-4.5 + 1.0 * (k % 10) + 0.0137 * k, 0.0, -3.0 + 1.0 * (k // 10) + 0.0071 * k), inner))
    balls = [b.sphere((-4.0 + 0.7 * k, 1.2 + 0.01 * k, 0.5 * (k % 3) - 3.5), 0.2, m[k % 4]) for k in range(12)]
    fixed = [b.sphere((0.0, -500.0, 0.0), 500.0, m[2]), b.sphere((0.0, 6.0, 1.0), 1.0, b.diffuse_light((4.0, 4.0, 4.0)))]
    if spelling == "hoisted":
        return b, b.hittable_list(fixed + members + [b.bvh_from_list(b.hittable_list(balls), 0.0, 1.0)])
    return b, b.hittable_list(fixed + [b.bvh_from_list(b.hittable_list(members + balls), 0.0, 1.0)])


def _cam_cfg(rtsr):
    cam = rtsr.Camera.new((1.0, 4.2, 9.5), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0), 42.0, 1.5, 0.05, 9.0, 0.0, 1.0)
    cfg = rtsr.Config.new(1.5, 120, 16, 30, 4, seed=11, background=(0.35, 0.4, 0.55))
    return cam, cfg, rtsr.image_height(cfg)


SEEDS = (12345, 1, 2, 3)


def test_rotate_y_keeps_the_unrotated_box_and_a_bvh_culls_by_it(rtsr, orc):
    """One ray, no random tree: a BvhNode of ONE member (bvh.rs:53-55: left = right = the member, bbox = its box).  The ray comes
    down on the corner a 45-degree turn pushes out to x = sqrt(2), outside the prism's own x range [-1, 1]."""
    b = rtsr.Builder(1)
    rot = b.rotate_y(45.0, b.rect_prism((-1.0, 0.0, -1.0), (1.0, 1.0, 1.0), b.lambertian((0.5, 0.5, 0.5))))
    node = b.bvh_from_list(b.hittable_list([rot]), 0.0, 1.0)
    o, d = (1.2, 5.0, 0.05), (0.001, -1.0, 0.002)
    bare = orc.o1_hit(b.graph_ptr(), rot, o, d)
    assert bare is not None and abs(bare["p"][1] - 1.0) < 1e-12 and bare["p"][0] > 1.0  # the top face, beyond the un-rotated box
    assert orc.o1_hit(b.graph_ptr(), node, o, d) is None                               # culled by Aabb(p0, p1) of the child
    inside = orc.o1_hit(b.graph_ptr(), node, (0.3, 5.0, 0.05), d)                        # a ray through that box sees the member
    assert inside is not None and inside["t"] == orc.o1_hit(b.graph_ptr(), rot, (0.3, 5.0, 0.05), d)["t"]


def test_o1_translate_members_render_like_the_hoisted_spelling(rtsr, orc):
    cam, cfg, h = _cam_cfg(rtsr)
    b, world = _box_field(rtsr, "hoisted", rotate=False)
    hoisted, _ = orc.o1_render(b.graph_ptr(), world, cam, cfg, h, threads=8)
    assert hoisted.std() > 0.01
    for seed in SEEDS:
        b, world = _box_field(rtsr, "instanced", rotate=False)
        accum, _ = orc.o1_render(b.graph_ptr(), world, cam, cfg, h, threads=8, bvh_seed=seed)
        assert np.array_equal(accum, hoisted), "bvh_seed %d: %d pixels differ" % (seed, int((np.abs(accum - hoisted).max(axis=2) > 0).sum()))


def test_o1_rotate_y_members_render_a_different_image_per_tree(rtsr, orc):
    cam, cfg, h = _cam_cfg(rtsr)
    b, world = _box_field(rtsr, "hoisted", rotate=True)
    hoisted, _ = orc.o1_render(b.graph_ptr(), world, cam, cfg, h, threads=8)
    frames = []
    for seed in SEEDS:
        b, world = _box_field(rtsr, "instanced", rotate=True)
        frames.append(orc.o1_render(b.graph_ptr(), world, cam, cfg, h, threads=8, bvh_seed=seed)[0])
    for seed, f in zip(SEEDS, frames):
        bad = int((np.abs(f - hoisted).max(axis=2) > 0).sum())
        print("bvh_seed %d: %d of %d pixels differ from the hoisted spelling" % (seed, bad, h * cfg.image_width))
        assert bad > 0
    for k in range(1, len(frames)):
        assert not np.array_equal(frames[0], frames[k]), "bvh_seed %d" % SEEDS[k]
    # the same tree gives the same frame: what differs is the tree, not the run
    b, world = _box_field(rtsr, "instanced", rotate=True)
    assert np.array_equal(orc.o1_render(b.graph_ptr(), world, cam, cfg, h, threads=3, bvh_seed=SEEDS[0])[0], frames[0])


def test_the_refusal_says_why_and_what_to_write_instead(rtsr):
    b = rtsr.Builder(1)
    s = b.sphere((0.0, 0.0, 0.0), 1.0, b.lambertian((0.5, 0.5, 0.5)))
    for kw in ({}, {"max_leaf": 4}, {"reference_bvh": True}):
        for member in (b.rotate_y(20.0, s), b.translate((1.0, 0.0, 0.0), b.rotate_y(20.0, s))):
            with pytest.raises(rtsr.RtxError) as e:
                b.flatten(b.bvh_from_list(b.hittable_list([member, s]), 0.0, 1.0), **kw)
            assert e.value.status == rtsr.RTX_EUNSUPPORTED
            msg = str(e.value)
            assert "instanced sub-tree" in msg and "hit.rs:886" in msg and "bvh.rs:24" in msg and "world list" in msg
        with pytest.raises(rtsr.RtxError) as e:
            b.flatten(b.bvh_from_list(b.hittable_list([b.constant_medium((1.0, 1.0, 1.0), 0.1, s), s]), 0.0, 1.0), **kw)
        assert e.value.status == rtsr.RTX_EUNSUPPORTED
        msg = str(e.value)
        assert "ConstantMedium" in msg and "hit.rs:955-986" in msg and "draws" in msg and "world list" in msg
    # the spelling the message names flattens
    hoisted = b.hittable_list([b.translate((1.0, 0.0, 0.0), b.rotate_y(20.0, s)), b.bvh_from_list(b.hittable_list([s, s]), 0.0, 1.0)])
    assert b.flatten(hoisted).info()["n_top_level"] == 2
