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


# ---- the member zoo: every member kind emit_solid_entry accepts, in every slot layout the scans branch on ----
ZOO_LAYOUTS = ("middle", "first", "after_bvh", "last", "alone", "two", "pair", "one", "empty")


def zoo_image(width=16, height=8):
    """A procedural image texture (height x width x 3 in [0, 1]): no two neighbouring texels are equal."""
    return [[[(3 * i + 5 * j) % 7 / 7.0, (i * j + 2) % 5 / 5.0, (i + 2 * j) % 3 / 3.0] for i in range(width)] for j in range(height)]


def _zoo_members(b, plain=False):
    """(members in list order, aim points).  A BvhNode of spheres comes FIRST (layout "first" needs a BVH at slot 0).
    plain: the noise and image textures become solid colours (the checker and the glass stay), so that no sample reaches the
    VALUE of a platform function: tier A of tests/test_gpu_f32_parity.py."""
    grey, red = b.lambertian((0.5, 0.5, 0.5)), b.lambertian((0.8, 0.2, 0.2))
    green, blue = b.lambertian((0.2, 0.7, 0.3)), b.lambertian((0.2, 0.3, 0.8))
    checker = b.lambertian(b.checker_from_colors((0.1, 0.3, 0.1), (0.9, 0.9, 0.9)))
    noise = b.lambertian((0.7, 0.6, 0.3)) if plain else b.lambertian(b.noise(4.0))
    image = b.lambertian((0.3, 0.6, 0.7)) if plain else b.lambertian(b.image_from_texels(zoo_image()))
    metal, glass = b.metal((0.8, 0.8, 0.9), 0.2), b.dielectric(1.5)
    light = b.diffuse_light((6.0, 6.0, 5.0))
    m, aim = [], []

    def add(obj, *points):
        m.append(obj)
        aim.extend(points)

    def ball_row(x0, z, n, mat, y=0.3):
        return b.bvh_from_list(b.hittable_list([b.sphere((x0 + 0.7 * k, y + 0.02 * k, z + 0.1 * (k % 2)), 0.3, mat) for k in range(n)]), 0.0, 1.0)

    def fan(x0, z, mat):
        # six triangles standing on y = 0.05, none of them in an axis plane: the reference's Aabb::hit (aabb.rs:23-61) never
        # passes a box of zero thickness, so a BvhNode never shows such a triangle, and O1 follows it
        return b.bvh_from_list(b.hittable_list([b.triangle((x0 + 0.5 * k, 0.05, z), (x0 + 0.5 * k + 0.45, 0.05, z + 0.03 + 0.1 * (k % 3)),
                                                           (x0 + 0.5 * k + 0.2, 0.9, z - 0.07 - 0.05 * k), mat) for k in range(6)]), 0.0, 1.0)

    add(ball_row(-4.5, -1.5, 6, red), (-4.5, 0.3, -1.5), (-1.0, 0.4, -1.4))                   # an unwrapped BvhNode of spheres
    add(b.sphere((-4.0, 0.6, 1.0), 0.6, checker), (-4.0, 0.6, 1.0))                           # bare primitives
    add(b.xy_rect(-3.0, -2.0, 0.2, 1.2, -0.5, noise), (-2.5, 0.7, -0.5))
    add(b.xz_rect(-2.5, -1.5, 0.5, 1.5, 0.4, metal), (-2.0, 0.4, 1.0))
    add(b.yz_rect(0.2, 1.2, 0.0, 1.0, -1.2, image), (-1.2, 0.7, 0.5))
    add(b.triangle((-1.0, 0.1, 1.5), (0.0, 0.1, 1.5), (-0.5, 1.1, 1.2), red), (-0.5, 0.4, 1.4))
    add(b.sphere((1.0, 0.7, 1.2), 0.7, glass), (1.0, 0.7, 1.2))                               # the hollow-glass pair ...
    add(b.sphere((1.0, 0.7, 1.2), -0.6, glass), (1.0, 1.25, 1.2))
    add(b.sphere((2.3, 0.5, 1.2), 0.5, blue), (2.3, 0.5, 1.2))                                # ... and its neighbour in the tree
    add(b.rect_prism((3.0, 0.0, 0.5), (3.8, 0.9, 1.3), green), (3.4, 0.45, 0.9))              # a bare RectPrism
    add(b.hittable_list([b.sphere((4.6, 0.4, 1.0), 0.4, metal), b.xz_rect(4.2, 5.0, 1.5, 2.1, 0.3, red)]),  # a list: spliced in
        (4.6, 0.4, 1.0), (4.6, 0.3, 1.8))
    add(fan(-1.0, -0.6, blue), (0.5, 0.4, -0.6))                                              # a BvhNode of triangles
    add(b.translate((2.0, 0.1, -2.2), b.rotate_y(37.0, ball_row(-1.0, 0.0, 5, green))), (2.0, 0.4, -2.2))  # the wrapped BVH member
    add(b.translate((4.4, 0.0, -0.6), b.rotate_y(-52.0, fan(-1.2, 0.0, checker))), (4.4, 0.4, -0.6))
    prism = lambda mat: b.rect_prism((-0.3, 0.0, -0.5), (0.3, 0.7, 0.5), mat)
    add(b.rotate_y(0.0, b.rect_prism((-5.6, 0.0, -0.4), (-5.0, 0.7, 0.6), noise)), (-5.3, 0.35, 0.1))           # chains of 1 ...
    add(b.translate((-3.6, 0.0, -2.8), prism(image)), (-3.6, 0.35, -2.8))
    add(b.translate((-2.4, 0.0, -2.8), b.rotate_y(90.0, prism(red))), (-2.4, 0.35, -2.8))                      # ... 2 ...
    add(b.rotate_y(180.0, b.translate((1.2, 0.0, 2.8), prism(metal))), (-1.2, 0.35, -2.8))
    add(b.translate((0.2, 0.0, -2.0), b.rotate_y(180.0, b.translate((0.0, 0.5, 1.0), b.sphere((0.0, 0.0, 0.0), 0.45, glass)))),  # ... 3 ...
        (0.2, 0.5, -3.0))
    add(b.translate((5.4, 0.0, -2.6), b.rotate_y(33.0, b.translate((0.1, 0.0, 0.0), b.rotate_y(-17.0, prism(checker))))),  # ... and 4
        (5.5, 0.35, -2.6))
    add(b.translate((-5.2, 0.0, 1.9), b.rotate_y(90.0, b.xy_rect(-0.5, 0.5, 0.1, 0.9, 0.0, green))), (-5.2, 0.5, 1.9))
    add(b.sphere((0.0, 4.2, 0.0), 0.7, light), (0.0, 4.2, 0.0))                                 # an emissive member: a sampled light
    # coincident faces, as in tie_scene: a bare prism and a BvhNode holding a prism (and a ball), in both orders.  Both spellings
    # of the flat scene let the later member win every tie.  The reference does not where the BvhNode's OWN box ends in the tied
    # face (Aabb::hit, aabb.rs:23-61, rejects t_max <= t_min), so these members are judged between the spellings and against
    # O1 ray by ray (t, p and the normal are those of either prism), not by O1's frame
    def tie_bvh(x0, mat):
        return b.bvh_from_list(b.hittable_list([b.rect_prism((x0, 0.0, -4.4), (x0 + 1.0, 0.8, -3.6), mat),
                                                b.sphere((x0 + 0.5, 1.3, -4.0), 0.2, mat)]), 0.0, 1.0)
    add(b.rect_prism((-5.0, 0.0, -4.4), (-4.0, 0.8, -3.6), red), (-4.6, 0.8, -4.0))
    add(tie_bvh(-4.5, blue), (-4.2, 0.8, -4.0))
    add(tie_bvh(3.5, blue), (3.8, 0.8, -4.0))
    add(b.rect_prism((4.0, 0.0, -4.4), (5.0, 0.8, -3.6), red), (4.2, 0.8, -4.0))
    return m, aim


def member_zoo(rtsr, spelling, layout="middle", with_aim=False, plain=False):
    """Both spellings of a small world (28 member objects at most) whose members cover every kind emit_solid_entry accepts.
    layout: where the tree(s) stand in the world list (ZOO_LAYOUTS).  The hoisted twin has the same objects at the
    same positions.  with_aim: also a list of points on or in the members, for rays to be aimed at.  plain: see _zoo_members
    (the "pair" layout keeps its medium, which draws through logf: it is tier B either way)."""
    assert spelling in ("hoisted", "instanced") and layout in ZOO_LAYOUTS
    b = rtsr.Builder(13)
    zoo, aim = _zoo_members(b, plain)
    grey, glass = b.lambertian((0.5, 0.5, 0.5)), b.dielectric(1.5)
    ground = b.sphere((0.0, -500.0, 0.0), 500.0, b.lambertian((0.45, 0.5, 0.4)))
    s1 = b.sphere((0.0, 0.5, 2.6), 0.5, grey)
    plain_bvh = b.bvh_from_list(b.hittable_list([b.sphere((5.5 + 0.1 * k, 0.3 + 0.7 * k, 2.0), 0.3, grey) for k in range(3)]), 0.0, 1.0)
    aim = aim + [(0.0, 0.5, 2.6), (5.6, 1.0, 2.0), (2.0, 0.0, 0.0)]
    tree = (lambda ms: [b.instance_bvh(b.hittable_list(ms))]) if spelling == "instanced" else (lambda ms: list(ms))
    if layout == "middle":
        slots = [ground] + tree(zoo) + [s1]
    elif layout == "first":
        slots = tree(zoo) + [ground, s1]
    elif layout == "after_bvh":
        slots = [plain_bvh] + tree(zoo) + [ground]
    elif layout == "last":
        slots = [ground, s1] + tree(zoo)
    elif layout == "alone":
        slots = None
    elif layout == "two":
        slots = tree(zoo[:11]) + [ground, s1] + tree(zoo[11:]) + [plain_bvh]
    elif layout == "pair":  # Book-2's ball: a glass sphere, then a medium bounded by the very same sphere
        ball = b.sphere((2.4, 0.6, 2.4), 0.6, glass)
        aim = aim + [(2.4, 0.6, 2.4)] * 3
        slots = [ground] + tree(zoo + [ball]) + [b.constant_medium((0.2, 0.4, 0.9), 0.8, ball), s1]
    else:  # "one" / "empty": no tree record at all, beside other slots (the other members stay plain slots in both spellings)
        slots = [ground] + tree([zoo[12]] if layout == "one" else []) + [s1, plain_bvh] + zoo[:12]
    if slots is None:
        world = b.instance_bvh(b.hittable_list(zoo)) if spelling == "instanced" else b.hittable_list(zoo)
    else:
        world = b.hittable_list(slots)
    return (b, world, aim) if with_aim else (b, world)


def zoo_cam_cfg(rtsr, width=48, spp=8, depth=12):
    cam = rtsr.Camera.new((0.8, 4.5, 10.5), (0.0, 0.6, -1.0), (0.0, 1.0, 0.0), 44.0, 1.5, 0.0, 10.0, 0.0, 1.0)
    cfg = rtsr.Config.new(1.5, width, spp, depth, 4, seed=17, background=(0.35, 0.4, 0.55))
    return cam, cfg, rtsr.image_height(cfg)


def offset_scene(rtsr, spelling, offset):
    """Four members carried `offset` away along x and z (0, 12345.678, 1e6): where the boxes' slack has to grow with the
    magnitude.  -> (builder, world, aim points)."""
    b = rtsr.Builder(5)
    grey, red = b.lambertian((0.5, 0.5, 0.5)), b.metal((0.8, 0.3, 0.3), 0.1)
    balls = b.bvh_from_list(b.hittable_list([b.sphere((0.6 * k, 0.3, 0.0), 0.3, red) for k in range(4)]), 0.0, 1.0)
    ms = [b.translate((offset, 0.0, offset), b.rotate_y(31.0, b.rect_prism((-0.5, 0.0, -0.5), (0.5, 1.0, 0.5), grey))),
          b.translate((offset + 2.0, 0.0, offset), b.rotate_y(-70.0, balls)),
          b.sphere((offset - 2.0, 0.5, offset), 0.5, grey), b.sphere((offset - 2.0, 0.5, offset), -0.4, grey),
          b.translate((offset, 0.0, offset + 2.0), b.xz_rect(-0.5, 0.5, -0.5, 0.5, 0.25, red))]
    aim = [(offset, 0.5, offset), (offset + 2.5, 0.3, offset - 0.5), (offset - 2.0, 0.5, offset), (offset, 0.25, offset + 2.0)]
    world = b.hittable_list([b.instance_bvh(b.hittable_list(ms))] if spelling == "instanced" else ms)
    return b, world, aim


# The f32 fast mode on the zoo (tests/test_gpu_instance_tree.py), by the tier rule of tests/test_gpu_f32_parity.py.  Tier A,
# bit for bit against O2f: the plain zoo in every layout but "pair".  Tier B: the zoo with its noise and image textures in
# every layout, and the plain "pair" (its medium); the cap on unequal pixels comes from the two CPU builds of O2f alone
# (glibc's float functions against the same five computed in double), measured at the frame of zoo_cam_cfg by
# tests/test_instance_tree.py::test_zoo_reference_alone_flip_rate: 0 unequal pixels of 1536 in every case, so every cap is
# the floor of test_gpu_f32_parity.cap_pixels, max(4 x unequal, 5) = 5 pixels.
ZOO_F32_EXACT = [("plain", l) for l in ZOO_LAYOUTS if l != "pair"]
ZOO_F32_CAPPED = [("textured", l) for l in ZOO_LAYOUTS] + [("plain", "pair")]
ZOO_REFERENCE_ALONE_UNEQUAL = {case: 0 for case in ZOO_F32_CAPPED}

# Where the zoo's image-textured members lie (lo, hi; their surfaces are the only ones inside): the YzRect at x = -1.2 and the
# translated prism at (-3.6, 0, -2.8).  The core computes u and v for such members only (and stores 0 elsewhere), so a test
# that compares u and v with O1 picks the hits to compare by WHERE O1 says the ray hit.
ZOO_IMAGE_REGIONS = [((-1.2001, 0.2, 0.0), (-1.1999, 1.2, 1.0)), ((-3.9001, -0.0001, -3.3001), (-3.2999, 0.7001, -2.2999))]
