"""Scenes shared by tests/test_instance_tree.py and tests/test_gpu_instance_tree.py (a helper module, not a test file).

The field is that of tests/test_instances_oracle.py (copied, not imported): a ground sphere, a lamp, n Translate(RotateY(
RectPrism)) boxes and a BvhNode of 12 spheres -- in two spellings.  "hoisted": every box is its own slot of the world list and
the sphere BVH follows them.  "instanced": the boxes AND the sphere BVH are the members of ONE instance tree standing at the
same position of the list.  The contract under test: both spellings give the same frame, bit for bit, everywhere.
"""


def box_field(rtsr, spelling, n=60, lamp_member=False):
    """n <= 60: the field of test_instances_oracle.py exactly (rows of 10).  Larger n: a square grid (1024 -> 32 x 32) with a
    small per-box jitter so that no two surfaces coincide.  lamp_member: the lamp, a plain sphere light, is the FIRST member
    instead of a slot before the members (same position in the list either way)."""
    b = rtsr.Builder(7)
    m = [b.lambertian((0.8, 0.3, 0.3)), b.metal((0.8, 0.8, 0.9), 0.3), b.lambertian((0.2, 0.7, 0.3)), b.lambertian((0.3, 0.3, 0.8))]
    cols = 10 if n <= 60 else int(round(n ** 0.5))
    members = []
    for k in range(n):
        w = 0.25 + 0.013 * (k % 7)
        box = b.rect_prism((-w, 0.0, -w), (w, 0.3 + 0.05 * (k % 5), w), m[k % 4])
        if n <= 60:
            x, z = -4.5 + 1.0 * (k % 10) + 0.0137 * k, -3.0 + 1.0 * (k // 10) + 0.0071 * k
        else:
            x, z = -0.5 * cols + 1.0 * (k % cols) + 0.0137 * (k % 7), -0.5 * cols + 1.0 * (k // cols) + 0.0071 * (k % 5)
        members.append(b.translate((x, 0.0, z), b.rotate_y(7.0 + 5.3 * k, box)))
    balls = [b.sphere((-4.0 + 0.7 * k, 1.2 + 0.01 * k, 0.5 * (k % 3) - 3.5), 0.2, m[k % 4]) for k in range(12)]
    ground = b.sphere((0.0, -500.0, 0.0), 500.0, m[2])
    lamp = b.sphere((0.0, 6.0, 1.0), 1.0, b.diffuse_light((4.0, 4.0, 4.0)))
    ball_bvh = b.bvh_from_list(b.hittable_list(balls), 0.0, 1.0)
    before = [ground] if lamp_member else [ground, lamp]
    group = ([lamp] if lamp_member else []) + members + [ball_bvh]
    if spelling == "hoisted":
        return b, b.hittable_list(before + group)
    assert spelling == "instanced"
    return b, b.hittable_list(before + [b.instance_bvh(b.hittable_list(group))])


def field_cam_cfg(rtsr, n=60, width=120, spp=16, depth=30):
    """n = 60: the camera of test_instances_oracle.py.  A larger field is seen from higher up and farther away."""
    if n <= 60:
        cam = rtsr.Camera.new((1.0, 4.2, 9.5), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0), 42.0, 1.5, 0.05, 9.0, 0.0, 1.0)
    else:
        s = n ** 0.5
        cam = rtsr.Camera.new((0.1 * s, 0.55 * s, 1.05 * s), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0), 42.0, 1.5, 0.0, 1.0 * s, 0.0, 1.0)
    cfg = rtsr.Config.new(1.5, width, spp, depth, 4, seed=11, background=(0.35, 0.4, 0.55))
    return cam, cfg, rtsr.image_height(cfg)


def tie_scene(rtsr, order, spelling):
    """Two bare prisms of equal height that overlap in plan: both top faces lie at y = 1, so a ray from above meets them at the
    same t.  HittableList::hit lets the LATER one win (hit.rs:676-680).  order: "AB" or "BA"; spelling: "list" or "instanced"."""
    b = rtsr.Builder(3)
    red, blue, grey = b.lambertian((0.9, 0.1, 0.1)), b.lambertian((0.1, 0.1, 0.9)), b.lambertian((0.5, 0.5, 0.5))
    a_box = b.rect_prism((-1.5, 0.0, -1.0), (0.5, 1.0, 1.0), red)
    b_box = b.rect_prism((-0.5, 0.0, -1.0), (1.5, 1.0, 1.0), blue)
    floor = b.xz_rect(-6.0, 6.0, -6.0, 6.0, 0.0, grey)
    pair = [a_box, b_box] if order == "AB" else [b_box, a_box]
    if spelling == "list":
        return b, b.hittable_list([floor] + pair)
    return b, b.hittable_list([floor, b.instance_bvh(b.hittable_list(pair))])


def tie_cam_cfg(rtsr, width=60, spp=4):
    cam = rtsr.Camera.new((0.0, 8.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 40.0, 1.5, 0.0, 8.0, 0.0, 1.0)
    cfg = rtsr.Config.new(1.5, width, spp, 8, 4, seed=5, background=(0.7, 0.8, 1.0))
    return cam, cfg, rtsr.image_height(cfg)
