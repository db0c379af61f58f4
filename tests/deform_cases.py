"""Deforming scenes for tests/test_set_triangles_host.py and tests/test_gpu_set_triangles.py (a helper module, not a test file).

Every case is built twice by the same function: at rest, and from scratch with every deformable vertex displaced -- the FRESH
scene, the judge of every test.  A case records its deformable parts: the handle whose triangles rtx_flat_triangle_ids lists
and the triangles' vertices in that order, at rest and displaced, so update_of() turns a rest scene into the ids and vertices
handed to set_triangles.  All seeded, all small; everything here runs on the CPU.

Coordinates stay away from 0: a box plane that is +0 in one union order and -0 in another is the same plane to every walker
but not the same bytes, and the tests compare bytes.
"""
import numpy as np

import update_cases
from set_transforms_cases import NODE, NODE32, MOTION32, narrow, leaf_boxes, tree_roots  # noqa: F401  (re-exported)
from update_cases import INSTANCED_POSE, Case, cam_cfg  # noqa: F401  (re-exported)

TRIANGLE = np.dtype([("v", np.float64, (3, 3)), ("normal", np.float64, (3,)), ("mat", np.int32), ("pad", np.int32)])
NODE4 = np.dtype([("lo", np.float32, (3, 4)), ("hi", np.float32, (3, 4)), ("child", np.int32, (4,)), ("pad", np.int32, (4,))])
assert (TRIANGLE.itemsize, NODE4.itemsize) == (104, 128)
FLAT_ARRAYS = ("triangles", "triangle_id", "nodes", "nodes32", "motion32", "entries", "top_level", "member_local_box", "top_box32")
DEVICE_ARRAYS = ("triangles", "nodes", "nodes32", "motion32", "entries", "world_desc", "top_box32")


def displace(v, cell):
    """The displacement of every case: a sine field of one cell size, plus a shear."""
    v = np.asarray(v, dtype=np.float64)
    out = v.copy()
    out[..., 1] += cell * np.sin(2.1 * v[..., 0] + 0.3) * np.cos(1.7 * v[..., 2] + 0.5)
    out[..., 0] += 0.11 * (v[..., 1] - 0.5) + 0.05 * cell * np.sin(3.3 * v[..., 2])
    out[..., 2] += 0.07 * cell * np.cos(2.9 * v[..., 0])
    return out


def sheet_mesh(n_tris, origin=(0.3, 1.0, 0.4), extent=4.0, seed=0):
    """n_tris triangles of a grid over [origin, origin + extent] in x and z, height a gentle seeded bump: (vertices, faces,
    cell).  The grid is the smallest near-square one that holds n_tris; an odd count drops the last triangle."""
    cells = (n_tris + 1) // 2
    nx = max(int(np.ceil(np.sqrt(cells))), 1)
    ny = (cells + nx - 1) // nx
    cell = extent / max(nx, ny)
    rng = np.random.default_rng(100 + seed)
    gx, gz = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    v = np.stack([origin[0] + cell * gx, origin[1] + 0.2 * cell * rng.uniform(0.1, 1.0, gx.shape), origin[2] + cell * gz], axis=-1).reshape(-1, 3)
    idx = lambda i, j: i * (ny + 1) + j
    faces = []
    for i in range(nx):
        for j in range(ny):
            faces.append((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)))
            faces.append((idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))
    return v, np.array(faces[:n_tris], dtype=np.int64), cell


class _Maker(update_cases.Maker):
    """Deformable triangles: (handle, rest triangles, moved triangles) per part.  Meshes are given to the builder triangle by
    triangle (no shared vertex records), so that one triangle can move alone; the displacement is a function of position, so
    shared corners still move together."""

    def _pick(self, rest, mv):
        on = np.array([self.on(self.k + i) for i in range(len(rest))])
        self.k += len(rest)
        return np.where(on[:, None, None], mv, rest)

    def mesh(self, v, faces, cell, mat):
        """-> the list handle rtx_triangle_mesh returns."""
        rest = np.asarray(v, dtype=np.float64)[faces]
        mv = displace(rest, cell)
        use = self._pick(rest, mv)
        h = self.b.triangle_mesh(use.reshape(-1, 3), np.arange(3 * len(use), dtype=np.int64).reshape(-1, 3), mat)
        self.parts.append((h, rest, mv))
        return h

    def triangle(self, tri, cell, mat):
        rest = np.asarray(tri, dtype=np.float64)[None]
        mv = displace(rest, cell)
        use = self._pick(rest, mv)[0]
        h = self.b.triangle(tuple(use[0]), tuple(use[1]), tuple(use[2]), mat)
        self.parts.append((h, rest, mv))
        return h


def sheet(rtsr, moved, n_tris, max_leaf=0, gpu_builder=False):
    m = _Maker(rtsr, 5, moved)
    b = m.b
    v, f, cell = sheet_mesh(n_tris)
    mesh = m.mesh(v, f, cell, b.lambertian((0.7, 0.4, 0.3)))
    world = b.hittable_list([b.sphere((2.3, -500.0, 2.4), 500.0, b.lambertian((0.5, 0.5, 0.5))), b.bvh_from_list(mesh, 0.0, 1.0)])
    return Case(b, world, m.parts, {"max_leaf": max_leaf, "gpu_builder": gpu_builder})


def line(rtsr, moved, n=40):
    """n triangles at geometric spacing: a deep, skewed tree."""
    m = _Maker(rtsr, 6, moved)
    b = m.b
    v, faces = [], []
    for k in range(n):
        x = 0.3 + 0.002 * 1.3 ** k
        s = 0.0005 * 1.3 ** k
        v += [(x, 1.0, 1.0), (x + s, 1.0 + 0.3 * s, 1.0 + s), (x, 1.0 + s, 1.0 + 2 * s)]
        faces.append((3 * k, 3 * k + 1, 3 * k + 2))
    mesh = m.mesh(np.array(v), np.array(faces, dtype=np.int64), 0.2, b.lambertian((0.3, 0.6, 0.8)))
    world = b.hittable_list([b.sphere((30.0, -500.0, 2.4), 500.0, b.lambertian((0.5, 0.5, 0.5))), b.bvh_from_list(mesh, 0.0, 1.0)])
    return Case(b, world, m.parts, {"max_leaf": 1}, look=((30.0, 30.0, 120.0), (30.0, 8.0, 30.0)))


def _mixed_members(m, n_tris=24):
    """A mesh, static spheres (one of negative radius) and rectangles, for ONE BvhNode."""
    b = m.b
    red, glass, grey = b.lambertian((0.8, 0.3, 0.3)), b.dielectric(1.5), b.metal((0.7, 0.7, 0.8), 0.1)
    v, f, cell = sheet_mesh(n_tris, origin=(0.5, 0.6, 0.6), extent=3.0, seed=1)
    mesh = m.mesh(v, f, cell, red)
    # (the sphere of negative radius sits inside an opaque one: its reference box is inverted, hit.rs:239-244, so whether the
    # literal oracle's BvhNode ever reaches it depends on its random tree -- no ray may be able to tell)
    others = [b.sphere((1.0, 1.6, 1.2), 0.45, red), b.sphere((1.0, 1.6, 1.2), -0.4, glass), b.sphere((3.2, 1.5, 2.8), 0.5, grey),
              b.sphere((2.1, 2.4, 0.9), 0.3, red), b.xz_rect(0.4, 1.6, 2.6, 3.8, 1.9, grey), b.xy_rect(2.6, 3.9, 0.5, 1.8, 0.45, red),
              b.yz_rect(0.7, 1.9, 1.1, 2.3, 4.1, grey)]
    return mesh, others


def mixed(rtsr, moved):
    m = _Maker(rtsr, 7, moved)
    b = m.b
    mesh, others = _mixed_members(m)
    world = b.hittable_list([b.sphere((2.3, -500.0, 2.4), 500.0, b.lambertian((0.5, 0.5, 0.5))), b.bvh_from_list(b.hittable_list([mesh] + others), 0.0, 1.0)])
    return Case(b, world, m.parts)


def beside_movers(rtsr, moved):
    """A sheet's BVH beside a BVH of moving spheres: the scene has time-aware boxes, the sheet's nodes carry their static copy."""
    m = _Maker(rtsr, 8, moved)
    b = m.b
    v, f, cell = sheet_mesh(30, seed=2)
    mesh = m.mesh(v, f, cell, b.lambertian((0.7, 0.4, 0.3)))
    grey = b.lambertian((0.5, 0.5, 0.5))
    movers = b.bvh_from_list(b.hittable_list([b.moving_sphere((0.8 + k, 2.5, 1.0), (0.8 + k, 2.5 + 0.2 * k, 1.0), 0.0, 1.0, 0.3, grey) for k in range(4)]), 0.0, 1.0)
    world = b.hittable_list([b.sphere((2.3, -500.0, 2.4), 500.0, grey), b.bvh_from_list(mesh, 0.0, 1.0), movers])
    return Case(b, world, m.parts)


def shared(rtsr, moved):
    """One triangle handle in a BVH AND as a plain top-level slot (two flat copies, one id), a second plain triangle, and a
    handle listed twice in the BVH."""
    m = _Maker(rtsr, 9, moved)
    b = m.b
    red, blue = b.lambertian((0.8, 0.3, 0.3)), b.lambertian((0.2, 0.3, 0.8))
    v, f, cell = sheet_mesh(10, seed=3)
    mesh = m.mesh(v, f, cell, red)
    both = m.triangle([(1.0, 2.0, 1.0), (2.5, 2.2, 1.3), (1.4, 3.1, 2.2)], 0.5, blue)
    alone = m.triangle([(3.0, 1.8, 2.0), (4.1, 2.0, 2.4), (3.3, 2.9, 3.3)], 0.5, blue)
    twice = m.triangle([(0.6, 2.4, 3.0), (1.5, 2.5, 3.4), (0.9, 3.2, 3.9)], 0.5, red)
    pair = b.hittable_list([twice, twice])
    members = b.hittable_list([mesh, both, pair])
    bvh = b.bvh_from_list(members, 0.0, 1.0)
    world = b.hittable_list([b.sphere((2.3, -500.0, 2.4), 500.0, b.lambertian((0.5, 0.5, 0.5))), both, bvh, alone])
    case = Case(b, world, m.parts)
    case.handles = {"pair": pair, "members": members, "bvh": bvh, "both": both, "twice": twice, "alone": alone}
    return case


def instanced(rtsr, moved, hoisted=False, pose=INSTANCED_POSE):
    """An instance tree of two Translate(RotateY(BvhNode(sheet))) and a Translate(list of 3 triangles), beside a ground sphere.
    hoisted: the members written into the world list themselves -- the spelling the literal oracle renders.  pose: the three
    members' (offset, angle in degrees; None: the member has no RotateY)."""
    m = _Maker(rtsr, 10, moved)
    b = m.b
    red, blue, grey = b.lambertian((0.8, 0.3, 0.3)), b.metal((0.6, 0.7, 0.9), 0.2), b.lambertian((0.5, 0.5, 0.5))
    members = []
    for k, (off, ang) in enumerate(pose[:2]):
        v, f, cell = sheet_mesh(18 + 6 * k, origin=(0.2, 0.8, 0.3), extent=2.0, seed=4 + k)
        members.append(b.translate(off, b.rotate_y(ang, b.bvh_from_list(m.mesh(v, f, cell, red if k else blue), 0.0, 1.0))))
    tris = [m.triangle([(0.2 + 0.7 * k, 0.5, 0.3), (0.8 + 0.7 * k, 0.6, 0.5), (0.4 + 0.7 * k, 1.4, 0.9)], 0.4, red) for k in range(3)]
    members.append(b.translate(pose[2][0], b.hittable_list(tris)))
    ground = b.sphere((2.3, -500.0, 2.4), 500.0, grey)
    world = b.hittable_list([ground] + members) if hoisted else b.hittable_list([ground, b.instance_bvh(b.hittable_list(members))])
    return Case(b, world, m.parts, look=((2.8, 5.5, 10.5), (2.8, 1.0, 2.4)))


def fog(rtsr, moved):
    """A ConstantMedium whose boundary is a closed triangle mesh (an octahedron, each face split in four) in a BVH."""
    m = _Maker(rtsr, 11, moved)
    b = m.b
    c, r = np.array((2.3, 2.0, 2.4)), 1.3
    corners = [c + r * np.array(d, dtype=np.float64) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    v, faces = list(corners), []
    mid = {}

    def midpoint(i, j):
        key = (min(i, j), max(i, j))
        if key not in mid:
            p = 0.5 * (v[i] + v[j])
            v.append(c + r * (p - c) / np.linalg.norm(p - c))
            mid[key] = len(v) - 1
        return mid[key]

    for x in (0, 1):
        for y in (2, 3):
            for z in (4, 5):
                ab, bc, ca = midpoint(x, y), midpoint(y, z), midpoint(z, x)
                faces += [(x, ab, ca), (y, bc, ab), (z, ca, bc), (ab, bc, ca)]
    mesh = m.mesh(np.array(v), np.array(faces, dtype=np.int64), 0.3, b.lambertian((0.5, 0.5, 0.5)))
    smoke = b.constant_medium((0.9, 0.9, 1.0), 0.8, b.bvh_from_list(mesh, 0.0, 1.0))
    world = b.hittable_list([b.sphere((2.3, -500.0, 2.4), 500.0, b.lambertian((0.4, 0.6, 0.4))), smoke, b.sphere((4.0, 1.0, 3.5), 0.6, b.metal((0.8, 0.8, 0.8), 0.0))])
    return Case(b, world, m.parts)


def movers(rtsr, moved=False):
    """A BVH of triangles and one MovingSphere: the refusal."""
    m = _Maker(rtsr, 12, moved)
    b = m.b
    v, f, cell = sheet_mesh(12, seed=6)
    mesh = m.mesh(v, f, cell, b.lambertian((0.7, 0.4, 0.3)))
    grey = b.lambertian((0.5, 0.5, 0.5))
    bvh = b.bvh_from_list(b.hittable_list([mesh, b.moving_sphere((1.0, 2.5, 1.0), (1.0, 3.0, 1.0), 0.0, 1.0, 0.3, grey)]), 0.0, 1.0)
    return Case(b, b.hittable_list([b.sphere((2.3, -500.0, 2.4), 500.0, grey), bvh]), m.parts)


CASES = {
    "mixed": mixed, "beside_movers": beside_movers, "shared": shared, "instanced": instanced, "fog": fog, "line40": line,
    "sheet257_leaf1": lambda r, mv: sheet(r, mv, 257, max_leaf=1),
}
SHEET_LEAVES = (2, 3, 4, 5, 64, 65, 257, 1024)


def count_leaves(flat):
    """Leaves of all BVHs of a flat scene (instance trees aside: the cases that use this have none)."""
    nodes = flat.array("nodes").view(NODE)
    return int((nodes["child"] < 0).sum())


_sheet_sizes = {}


def sheet_tris_for_leaves(rtsr, leaves, max_leaf):
    """The triangle count at which sheet(...) flattens to exactly `leaves` leaves: `leaves` itself at max_leaf 1; at the
    default (2 a leaf) the largest count up to 2 * leaves whose tree has that many."""
    if max_leaf == 1:
        return leaves
    key = (leaves, max_leaf)
    if key not in _sheet_sizes:
        for n in range(2 * leaves, leaves - 1, -1):
            if n >= 2 and count_leaves(sheet(rtsr, False, n, max_leaf).flatten()) == leaves:
                _sheet_sizes[key] = n
                break
        else:
            raise AssertionError("no sheet of %d leaves at max_leaf %d" % (leaves, max_leaf))
    return _sheet_sizes[key]


def update_of(case, flat, moved=True, every=1, only=None):
    """(ids, vertices[n, 9]) that move the deformable triangles of `flat` (flattened from `case`, the REST build) to their
    displaced (or, moved=False, their rest) vertices.  every: each every-th id; only: that one position of the full list."""
    ids, verts = [], []
    for h, rest, mv in case.parts:
        got = flat.triangle_ids(case.builder, h)
        assert len(got) == len(rest)
        ids.append(got)
        verts.append((mv if moved else rest).reshape(-1, 9))
    ids, verts = np.concatenate(ids), np.concatenate(verts)
    # a handle listed twice yields its id twice: keep the first
    _, first = np.unique(ids, return_index=True)
    keep = np.sort(first)
    ids, verts = ids[keep], verts[keep]
    if only is not None:
        return ids[only:only + 1].copy(), verts[only:only + 1].copy()
    return ids[::every].copy(), verts[::every].copy()


# One resident scene through all three update entries, on `instanced`: every triangle displaced; the members moved (the first
# set_transforms after a mesh update reads the members' local boxes back); the tree rebuilt; every third triangle back to rest;
# the members moved again.  Poses keep every coordinate away from 0, like the cases.
SEQUENCE_POSES = ((((1.0, 0.5, 0.2), 50.0), ((2.5, 0.1, 3.0), -10.0), ((0.3, 0.6, 3.2), None)),
                  (((0.6, 0.2, 0.1), 33.0), ((3.4, 0.4, 1.9), -60.0), ((1.5, 0.3, 4.4), None)))
SEQUENCE_END = {"moved": lambda k: k % 3 != 0, "pose": SEQUENCE_POSES[1]}  # instanced(rtsr, **SEQUENCE_END): the end state from scratch


def update_sequence(case, flat):
    """[(name, apply)]: apply(target) makes the step's call on a Flat or a Scene.  flat: flattened from `case` = instanced at
    rest (it only names the ids and the slots, so it may itself be a target)."""
    first = flat.instance_tree(0)["first_slot"]

    def ops(pose):
        return {first + k: [("translate", off)] + ([("rotate_y", ang)] if ang is not None else []) for k, (off, ang) in enumerate(pose)}

    return [("set_triangles", lambda s: s.set_triangles(*update_of(case, flat))),
            ("set_transforms", lambda s: s.set_transforms(ops(SEQUENCE_POSES[0]))),
            ("rebuild_instance_trees", lambda s: s.rebuild_instance_trees()),
            ("set_triangles again", lambda s: s.set_triangles(*update_of(case, flat, moved=False, every=3))),
            ("set_transforms again", lambda s: s.set_transforms(ops(SEQUENCE_POSES[1])))]


def triangles_by_id(flat):
    """{id: the 104 bytes of its record}; every flat copy of an id must hold the same bytes."""
    tri = flat.array("triangles").view(TRIANGLE)
    ids = flat.array("triangle_id").view(np.int32)
    assert len(tri) == len(ids)
    out = {}
    for t, i in zip(tri, ids):
        b = t.tobytes()
        assert out.setdefault(int(i), b) == b, "two copies of id %d differ" % i
    return out


def seeded_rays(n, seed, lo=(-0.5, 0.3, -0.5), hi=(5.5, 4.0, 5.5)):
    return update_cases.seeded_rays(n, seed, lo, hi, (0.5, 2.5))


def refusals(n_ids):
    """(name, ids or None, n or None, vertices or None, word of the message, host entries only)."""
    good = np.arange(18, dtype=np.float64).reshape(2, 9) + 1.0
    nan, inf = good.copy(), good.copy()
    nan[1, 4], inf[0, 8] = float("nan"), float("inf")
    return [
        ("null ids", None, 2, good, "ids is NULL", False),
        ("null vertices", [0, 1], None, None, "vertices is NULL", False),
        ("negative n", [0, 1], -1, good, "n < 0", False),
        ("id negative", [0, -1], None, good, "ids[1] is out of range", False),
        ("id past the end", [n_ids, 1], None, good, "ids[0] is out of range", False),
        ("id named twice", [1, 1], None, good, "twice", False),
        ("NaN vertex", [0, 1], None, nan, "vertices[1][4] is not finite", True),
        ("infinite vertex", [0, 1], None, inf, "vertices[0][8] is not finite", True),
    ]
