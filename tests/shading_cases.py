"""Worlds whose LOOK is edited, for tests/test_set_shading_host.py, tests/test_set_shading_abi.py and
tests/test_gpu_set_shading.py (a helper module, not a test file).

A case is a function of a dict of values that builds its world through the Builder.  REST[name] holds the values at rest,
VARIANTS[name] the edits tried: each a dict of the values that change.  The FRESH scene of a variant is the case built from
scratch with REST | variant -- the judge of every test; the EDITED scene is the case built at rest and then edited with
edits_for().  A world notes, per value name, what an edit of it names: ("solid_color", tex), ("noise_scale", tex), ("metal",
mat), ("dielectric", mat), ("medium_density", slot), or ("fog_color", slot) -- the colour texture rtx_constant_medium made
inside, reached through Flat.medium(slot) -> Flat.material -> tex as a caller has to.

All small, all seeded; coordinates are random doubles away from 0 so that no two primitives tie.  Everything here runs on
the CPU.
"""
import numpy as np

ASPECT = 16.0 / 9.0
MATERIAL = np.dtype([("kind", np.int32), ("tex", np.int32), ("albedo", np.float64, (3,)), ("param", np.float64), ("needs_uv", np.int32), ("pad", np.int32)])
TEXTURE = np.dtype([("kind", np.int32), ("a", np.int32), ("b", np.int32), ("pad", np.int32), ("color", np.float64, (3,)), ("scale", np.float64)])
MATERIAL32 = np.dtype([("kind", np.int32), ("tex", np.int32), ("albedo", np.float32, (3,)), ("param", np.float32), ("needs_uv", np.int32), ("pad", np.int32)])
TEXTURE32 = np.dtype([("kind", np.int32), ("a", np.int32), ("b", np.int32), ("pad", np.int32), ("color", np.float32, (3,)), ("scale", np.float32)])
LIGHT = np.dtype([("kind", np.int32), ("slot", np.int32), ("prim", np.int32), ("mat", np.int32), ("area", np.float64), ("cdf", np.float64), ("pmf", np.float64)])
assert (MATERIAL.itemsize, TEXTURE.itemsize, MATERIAL32.itemsize, TEXTURE32.itemsize, LIGHT.itemsize) == (48, 48, 32, 32, 40)
# every array rtx_flat_array serves
FLAT_ARRAYS = ("entries", "nodes", "nodes32", "motion32", "top_level", "member_local_box", "triangles", "top_box32", "triangle_id", "spheres",
               "lights", "materials", "textures")
# what an edit may write on a resident scene, and every other array rtx_device_scene_array serves
DEVICE_WRITTEN = ("materials", "textures", "entries", "world_desc", "lights")
DEVICE_KEPT = ("nodes", "nodes32", "motion32", "nodes4", "triangles", "top_box32", "spheres")
KERNEL_OF = {"simple": "k_trace_simple", "vote": "k_trace_vote", "world": "k_trace_world", "wavefront": "k_wf_trace"}


class World:
    """A world under construction: the builder, the values it is built with, and what an edit of each value names."""

    def __init__(self, rtsr, vals, seed=1):
        self.b, self.v, self.targets, self.slots = rtsr.Builder(seed), vals, {}, []

    def solid(self, name):
        tex = self.b.solid_color(self.v[name])
        self.targets[name] = ("solid_color", tex)
        return tex

    def noise(self, name):
        tex = self.b.noise(self.v[name])
        self.targets[name] = ("noise_scale", tex)
        return tex

    def lambertian(self, name):
        return self.b.lambertian(self.solid(name))

    def light(self, name):
        return self.b.diffuse_light(self.solid(name))

    def metal(self, name):
        rgb, fuzz = self.v[name]
        mat = self.b.metal(rgb, fuzz)
        self.targets[name] = ("metal", mat)
        return mat

    def glass(self, name):
        mat = self.b.dielectric(self.v[name])
        self.targets[name] = ("dielectric", mat)
        return mat

    def add(self, obj):
        """obj becomes the next slot of the world list."""
        self.slots.append(obj)
        return len(self.slots) - 1

    def fog(self, density, colour, boundary):
        slot = self.add(self.b.constant_medium(self.v[colour], self.v[density], boundary))
        self.targets[density] = ("medium_density", slot)
        self.targets[colour] = ("fog_color", slot)
        return slot


class Case:
    def __init__(self, w, look, bg=(0.7, 0.8, 1.0), world=None, vote=False, lds=False, vfov=35.0):
        self.builder, self.targets, self.look, self.bg, self.vfov = w.b, w.targets, look, bg, vfov
        self.world = world if world is not None else w.b.hittable_list(w.slots)
        self.vote, self.lds = vote, lds  # the world is ONE BVH beside plain primitives, in a preset k_trace_vote has; k_trace_lds by default

    def flatten(self):
        return self.builder.flatten(self.world)


def cam_cfg(rtsr, case, width=48, spp=4, depth=8, seed=31):
    cam = rtsr.Camera.new(case.look[0], case.look[1], (0.0, 1.0, 0.0), case.vfov, ASPECT, 0.0, 10.0, 0.0, 1.0)
    cfg = rtsr.Config.new(ASPECT, width, spp, depth, 4, seed=seed, background=case.bg)
    return cam, cfg, rtsr.image_height(cfg)


def _spheres(w, n, seed, mats, lo=(0.5, 0.45, 0.5), hi=(5.5, 1.7, 5.5), r=(0.12, 0.4)):
    rng = np.random.default_rng(seed)
    lo, hi = np.array(lo), np.array(hi)
    return [w.b.sphere(tuple(lo + (hi - lo) * rng.uniform(0.0, 1.0, 3)), float(rng.uniform(*r)), mats(k) if callable(mats) else mats[k % len(mats)])
            for k in range(n)]


def _ground(w, mat):
    return w.b.sphere((2.9, -1000.0, 2.9), 1000.0, mat)


FIELD_LOOK = ((3.0, 5.0, 11.0), (3.0, 0.8, 3.0))


# ---- the cases
def cornell_light(rtsr, v):
    """Five walls, one rectangle light, two spheres; no checker, noise or image: every kernel compiled for this world reads
    FlatMaterial::albedo only."""
    w = World(rtsr, v)
    b = w.b
    white, green = b.lambertian((0.73, 0.73, 0.73)), b.lambertian((0.12, 0.45, 0.15))
    w.add(b.yz_rect(0.0, 5.55, 0.0, 5.55, 5.55, green))
    w.add(b.yz_rect(0.0, 5.55, 0.0, 5.55, 0.0, w.lambertian("wall")))
    w.add(b.xz_rect(2.13, 3.43, 2.27, 3.32, 5.54, w.light("light")))
    w.add(b.xz_rect(0.0, 5.55, 0.0, 5.55, 0.0, white))
    w.add(b.xz_rect(0.0, 5.55, 0.0, 5.55, 5.55, white))
    w.add(b.xy_rect(0.0, 5.55, 0.0, 5.55, 5.55, white))
    w.add(b.sphere((1.9, 0.9, 1.9), 0.9, b.dielectric(1.5)))
    w.add(b.sphere((3.7, 1.2, 3.5), 1.2, white))
    return Case(w, ((2.78, 2.78, -8.0), (2.78, 2.78, 0.0)), bg=(0.0, 0.0, 0.0), vfov=40.0)


def shared_texture(rtsr, v):
    """ONE SolidColor named by a Lambertian, a DiffuseLight and an Isotropic, and a child of a checker on a fourth object: three
    albedo copies, one texture record, and the checker holds none.  (rtx_constant_medium makes its phase material's texture
    itself, so the Isotropic that shares a caller's texture is one from rtx_isotropic, worn by a sphere; the world holds a
    medium as well, whose own Isotropic must NOT follow the edit.)"""
    w = World(rtsr, v)
    b = w.b
    tex = w.solid("shared")
    w.add(_ground(w, b.lambertian(b.checker(tex, b.solid_color((0.9, 0.9, 0.9))))))
    w.add(b.sphere((1.3, 0.8, 2.9), 0.8, b.lambertian(tex)))
    w.add(b.xz_rect(2.2, 3.6, 2.1, 3.5, 3.4, b.diffuse_light(tex)))
    w.add(b.sphere((3.1, 0.7, 3.3), 0.7, b.isotropic(tex)))
    w.fog("density", "fog", b.sphere((4.7, 0.9, 2.2), 0.9, b.dielectric(1.5)))
    return Case(w, FIELD_LOOK)


def checker_children(rtsr, v):
    """Both children of the ground's checker, in a world of one sphere BVH whose kernels fetch textures (k_trace_lds's checker
    instantiation by default)."""
    w = World(rtsr, v)
    b = w.b
    ground = _ground(w, b.lambertian(b.checker(w.solid("even"), w.solid("odd"))))
    mats = [b.lambertian((0.8, 0.3, 0.3)), b.metal((0.7, 0.7, 0.8), 0.1), b.dielectric(1.5)]
    world = b.bvh_from_list(b.hittable_list([ground] + _spheres(w, 5, 311, mats)), 0.0, 1.0)
    return Case(w, FIELD_LOOK, world=world, vote=True, lds=True)


def two_lamps(rtsr, v):
    """A rectangle light and a sphere light of unequal colour over a floor."""
    w = World(rtsr, v)
    b = w.b
    w.add(b.xz_rect(-1.0, 7.0, -1.0, 7.0, 0.0, b.lambertian((0.6, 0.6, 0.6))))
    w.add(b.xz_rect(1.2, 2.6, 2.1, 3.3, 3.2, w.light("rect")))
    w.add(b.sphere((4.3, 2.4, 2.7), 0.45, w.light("ball")))
    w.add(b.sphere((2.9, 0.8, 3.1), 0.8, b.lambertian((0.7, 0.4, 0.3))))
    return Case(w, FIELD_LOOK, bg=(0.02, 0.02, 0.03))


def noise_lamp(rtsr, v):
    """A rectangle light whose emission is a Noise, beside a sphere light of a plain colour: the pick weight goes through
    texture_value."""
    w = World(rtsr, v)
    b = w.b
    w.add(b.xz_rect(-1.0, 7.0, -1.0, 7.0, 0.0, b.lambertian((0.6, 0.6, 0.6))))
    w.add(b.xz_rect(1.2, 2.6, 2.1, 3.3, 3.2, b.diffuse_light(w.noise("scale"))))
    w.add(b.sphere((4.3, 2.4, 2.7), 0.45, b.diffuse_light((2.0, 2.0, 2.0))))
    w.add(b.sphere((2.9, 0.8, 3.1), 0.8, b.lambertian(w.noise("marble"))))
    return Case(w, FIELD_LOOK, bg=(0.02, 0.02, 0.03))


def metal_fuzz(rtsr, v):
    w = World(rtsr, v)
    b = w.b
    mats = [w.metal("m0"), w.metal("m1"), b.lambertian((0.3, 0.5, 0.8))]
    world = b.bvh_from_list(b.hittable_list([_ground(w, b.lambertian((0.5, 0.5, 0.5)))] + _spheres(w, 6, 312, mats, r=(0.3, 0.6))), 0.0, 1.0)
    return Case(w, FIELD_LOOK, world=world, vote=True, lds=True)


def glass(rtsr, v):
    """Glass balls in a BVH under a top-level rectangle light: the mesh preset of k_trace_vote."""
    w = World(rtsr, v)
    b = w.b
    mats = [w.glass("g0"), b.lambertian((0.8, 0.3, 0.3)), w.glass("g1")]
    bvh = b.bvh_from_list(b.hittable_list([_ground(w, b.lambertian((0.5, 0.5, 0.5)))] + _spheres(w, 6, 313, mats, r=(0.3, 0.6))), 0.0, 1.0)
    w.add(bvh)
    w.add(b.xz_rect(1.5, 4.5, 1.5, 4.5, 4.0, b.diffuse_light((3.0, 3.0, 3.0))))
    return Case(w, FIELD_LOOK, vote=True)


def fog(rtsr, v):
    """Four media: bounded by a sphere that is also the glass ball in the slot before it (the slot record's WD_PAIR), by a
    rect_prism, by a rect_prism under Translate(RotateY(..)), and one whose density goes to 0."""
    w = World(rtsr, v)
    b = w.b
    w.add(_ground(w, b.lambertian((0.4, 0.6, 0.4))))
    w.add(b.sphere((1.71, 1.32, 2.93), 1.1, b.dielectric(1.5)))
    w.fog("d_pair", "c_pair", b.sphere((1.71, 1.32, 2.93), 1.1, b.dielectric(1.5)))
    w.fog("d_box", "c_box", b.rect_prism((3.1, 0.2, 3.6), (4.4, 1.5, 4.9), b.lambertian((1.0, 1.0, 1.0))))
    w.fog("d_turn", "c_turn", b.translate((4.2, 0.3, 0.9), b.rotate_y(25.0, b.rect_prism((0.0, 0.0, 0.0), (1.2, 1.6, 1.1), b.lambertian((1.0, 1.0, 1.0))))))
    w.fog("d_zero", "c_zero", b.sphere((0.9, 0.7, 5.0), 0.7, b.dielectric(1.5)))
    w.add(b.xz_rect(1.5, 4.5, 1.5, 4.5, 5.0, b.diffuse_light((3.0, 3.0, 3.0))))
    case = Case(w, FIELD_LOOK)
    case.pair_slot = 1
    return case


def tables(rtsr, v, n):
    """n materials and n textures: a top-level rectangle light and a BVH of n - 1 Lambertian spheres, each of its own colour.
    The LAST texture (and with it the last material) is what VARIANTS edit."""
    w = World(rtsr, v)
    b = w.b
    light = w.light("light")
    names = ["c%d" % k for k in range(n - 2)] + ["last"]
    mats = [w.lambertian(name) for name in names]
    bvh = b.bvh_from_list(b.hittable_list([_ground(w, mats[-1])] + _spheres(w, n - 2, 314 + n, mats[:-1], r=(0.2, 0.45))), 0.0, 1.0)  # the ground wears the last
    w.add(bvh)
    w.add(b.xz_rect(1.5, 4.5, 1.5, 4.5, 4.0, light))
    case = Case(w, FIELD_LOOK, vote=True)
    case.n = n
    return case


def _tables_rest(n):
    rng = np.random.default_rng(700 + n)
    v = {"c%d" % k: tuple(rng.uniform(0.2, 0.9, 3)) for k in range(n - 2)}
    v.update({"last": (0.9, 0.2, 0.2), "light": (3.0, 3.0, 3.0)})
    return v


MANY = 128  # Lambertian spheres of `many`: a colour edit of each is 2 write records, and one Metal edit makes 257


def many(rtsr, v):
    w = World(rtsr, v)
    b = w.b
    mats = [w.lambertian("c%d" % k) for k in range(MANY)]
    spheres = _spheres(w, MANY, 315, mats, lo=(0.3, 0.3, 0.3), hi=(5.7, 2.4, 5.7), r=(0.1, 0.25))
    world = b.bvh_from_list(b.hittable_list([_ground(w, w.metal("ground"))] + spheres), 0.0, 1.0)
    return Case(w, FIELD_LOOK, world=world, vote=True, lds=True)


def _many_rest():
    rng = np.random.default_rng(800)
    v = {"c%d" % k: tuple(rng.uniform(0.2, 0.9, 3)) for k in range(MANY)}
    v["ground"] = ((0.6, 0.6, 0.6), 0.2)
    return v


def _many_all():
    rng = np.random.default_rng(801)
    v = {"c%d" % k: tuple(rng.uniform(0.1, 0.95, 3)) for k in range(MANY)}
    v["ground"] = ((0.8, 0.7, 0.5), 0.05)
    return v


CASES = {
    "cornell_light": cornell_light, "shared_texture": shared_texture, "checker_children": checker_children, "two_lamps": two_lamps,
    "noise_lamp": noise_lamp, "metal_fuzz": metal_fuzz, "glass": glass, "fog": fog, "many": many,
    "tables_16": lambda r, v: tables(r, v, 16), "tables_17": lambda r, v: tables(r, v, 17),
    "tables_64": lambda r, v: tables(r, v, 64), "tables_65": lambda r, v: tables(r, v, 65),
}
REST = {
    "cornell_light": {"light": (15.0, 15.0, 15.0), "wall": (0.65, 0.05, 0.05)},
    "shared_texture": {"shared": (1.6, 1.3, 0.9), "fog": (0.2, 0.4, 0.9), "density": 0.8},
    "checker_children": {"even": (0.2, 0.3, 0.1), "odd": (0.9, 0.9, 0.9)},
    "two_lamps": {"rect": (4.0, 4.0, 4.0), "ball": (6.0, 5.0, 3.0)},
    "noise_lamp": {"scale": 4.0, "marble": 2.5},
    "metal_fuzz": {"m0": ((0.8, 0.8, 0.9), 0.1), "m1": ((0.9, 0.6, 0.3), 0.4)},
    "glass": {"g0": 1.5, "g1": 1.5},
    "fog": {"d_pair": 0.8, "c_pair": (0.2, 0.4, 0.9), "d_box": 0.6, "c_box": (0.9, 0.9, 1.0), "d_turn": 1.1, "c_turn": (0.1, 0.1, 0.1),
            "d_zero": 0.5, "c_zero": (0.8, 0.3, 0.3)},
    "many": _many_rest(),
    "tables_16": _tables_rest(16), "tables_17": _tables_rest(17), "tables_64": _tables_rest(64), "tables_65": _tables_rest(65),
}
VARIANTS = {
    "cornell_light": [{"light": (4.0, 9.0, 15.0), "wall": (0.1, 0.2, 0.7)}, {"light": (2.5, 2.5, 2.5)}],
    "shared_texture": [{"shared": (0.3, 2.1, 0.6)}],
    "checker_children": [{"even": (0.7, 0.1, 0.4), "odd": (0.05, 0.15, 0.6)}],
    "two_lamps": [{"rect": (0.0, 0.0, 0.0)}, {"rect": (0.0, 0.0, 0.0), "ball": (0.0, 0.0, 0.0)}, {"ball": (600.0, 500.0, 300.0)}],
    "noise_lamp": [{"scale": 0.7}, {"scale": 9.0, "marble": 0.4}],
    # fuzz 0, 0.3, exactly 1, 1.5 (stored as 1) and -0.25 (passes as the builder passes it)
    "metal_fuzz": [{"m0": ((0.3, 0.9, 0.4), f)} for f in (0.0, 0.3, 1.0, 1.5, -0.25)] + [{"m0": ((0.5, 0.5, 0.9), 0.0), "m1": ((0.9, 0.9, 0.2), 1.5)}],
    "glass": [{"g0": 1.0}, {"g0": 2.4, "g1": 1.33}, {"g0": 0.5}],
    "fog": [{"d_pair": 0.15, "c_pair": (0.9, 0.5, 0.1), "d_box": 2.5, "d_turn": 0.2, "c_turn": (0.7, 0.7, 0.9)}, {"d_zero": 0.0, "c_zero": (0.1, 0.9, 0.2)}],
    "many": [_many_all(), {"c77": (0.05, 0.9, 0.9)}],
    "tables_16": [{"last": (0.1, 0.9, 0.3)}], "tables_17": [{"last": (0.1, 0.9, 0.3)}],
    "tables_64": [{"last": (0.1, 0.9, 0.3)}], "tables_65": [{"last": (0.1, 0.9, 0.3)}],
}
assert sorted(CASES) == sorted(REST) == sorted(VARIANTS)
# a variant whose edit is refresh-free: no texture is edited, so a resident scene's light table is not recomputed
METAL_ONLY = ("metal_fuzz", 0)


def build(rtsr, name, variant=None):
    """The case at rest, or built from scratch with the values of `variant` (a dict, or an index into VARIANTS[name])."""
    vals = dict(REST[name])
    if variant is not None:
        vals.update(VARIANTS[name][variant] if isinstance(variant, int) else variant)
    return CASES[name](rtsr, vals)


def edits_for(case, flat, new_vals):
    """The edits that give `flat` (flattened from `case`) the values of new_vals: what Flat.set_shading / Scene.set_shading take."""
    out = []
    for name, val in new_vals.items():
        kind, index = case.targets[name]
        if kind == "fog_color":  # the colour rtx_constant_medium wrapped: slot -> phase material -> its texture
            mat = flat.medium(index)["material"]
            info = flat.material(mat)
            assert info["kind"] == "isotropic"
            kind, index = "solid_color", info["tex"]
        out.append((kind, index, val[0], val[1]) if kind == "metal" else (kind, index, val))
    return out


def sequence(rtsr):
    """ONE world for every kind of update of a resident scene in turn: a lamp sphere (set_spheres moves it, set_shading recolours
    it), a rectangle light, and a fog in a box under Translate(RotateY(..)) (set_transforms moves it, set_shading thins it).
    -> the case, with .lamp (the sphere's handle) and .fog_slot."""
    w = World(rtsr, {"ball": (6.0, 5.0, 3.0), "rect": (4.0, 4.0, 4.0), "d": 0.9, "c": (0.8, 0.8, 0.9)})
    b = w.b
    w.add(b.xz_rect(-1.0, 7.0, -1.0, 7.0, 0.0, b.lambertian((0.6, 0.6, 0.6))))
    w.add(b.xz_rect(1.2, 2.6, 2.1, 3.3, 3.2, w.light("rect")))
    lamp = b.sphere((4.3, 2.4, 2.7), 0.45, w.light("ball"))
    w.add(lamp)
    box = b.rect_prism((0.0, 0.0, 0.0), (1.4, 1.6, 1.2), b.lambertian((1.0, 1.0, 1.0)))
    fog_slot = w.fog("d", "c", b.translate((2.2, 0.2, 2.8), b.rotate_y(20.0, box)))
    w.add(b.sphere((0.9, 0.7, 4.4), 0.7, b.metal((0.8, 0.8, 0.8), 0.1)))
    case = Case(w, FIELD_LOOK, bg=(0.02, 0.02, 0.03))
    case.lamp, case.fog_slot = lamp, fog_slot
    return case


def pairs():
    """Every (case, variant index)."""
    return [(name, k) for name in sorted(CASES) for k in range(len(VARIANTS[name]))]


def book1(rtsr):
    """Catalogue scene 100 -> (builder, world, cam, background).  No builder spelling of new values exists for a catalogue scene:
    its judge is the host-edited flat scene (proven on the hand-built cases), uploaded fresh and rendered by the oracle."""
    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(rtsr.SCENE_BOOK1_CANONICAL)
    return b, world, cam, bg


def book1_edits(flat):
    """Every material of the flat scene edited by its kind: a Lambertian through its texture."""
    rng = np.random.default_rng(900)
    out, seen = [], set()
    for m in range(flat.info()["n_materials"]):
        info = flat.material(m)
        if info["kind"] == "metal":
            out.append(("metal", m, tuple(rng.uniform(0.3, 1.0, 3)), float(rng.uniform(0.0, 0.6))))
        elif info["kind"] == "dielectric":
            out.append(("dielectric", m, float(rng.uniform(1.2, 2.2))))
        elif flat.texture(info["tex"])["kind"] == "solid_color" and info["tex"] not in seen:
            seen.add(info["tex"])
            out.append(("solid_color", info["tex"], tuple(rng.uniform(0.05, 0.95, 3))))
    return out


# ---- raw calls and the refusals (tests/test_set_shading_abi.py on the flat scene, tests/test_gpu_set_shading.py on a resident one)
def raw_edit(rtsr, what, index, *v):
    e = rtsr.RtxShadingEdit()
    e.what, e.index = what, index
    for a, x in enumerate(v):
        e.v[a] = x
    return e


def call_set_shading(rtsr, fn, handle, edits, n=None, *rest):
    """One raw call of rtx_flat_set_shading / rtx_scene_set_shading.  edits: None for a NULL pointer; n: None for len(edits)."""
    arr = (rtsr.RtxShadingEdit * max(len(edits), 1))(*edits) if edits is not None else None
    return fn(handle, arr, len(edits) if n is None else n, *rest)


def refusals(rtsr, case, flat):
    """(edits or None, n or None, words of the message), in the order of the ladder."""
    t = case.targets
    shared, fog_slot = t["shared"][1], t["density"][1]
    info = flat.info()
    lam = [m for m in range(info["n_materials"]) if flat.material(m) == {"kind": "lambertian", "tex": shared, "albedo": flat.texture(shared)["color"], "param": 0.0}][0]
    checker = [x for x in range(info["n_textures"]) if flat.texture(x)["kind"] == "checker"][0]
    glass = [m for m in range(info["n_materials"]) if flat.material(m)["kind"] == "dielectric"][0]
    S, N, M, D, F = rtsr.RTX_SHADE_SOLID_COLOR, rtsr.RTX_SHADE_NOISE_SCALE, rtsr.RTX_SHADE_METAL, rtsr.RTX_SHADE_DIELECTRIC, rtsr.RTX_SHADE_MEDIUM_DENSITY
    good = raw_edit(rtsr, S, shared, 0.1, 0.2, 0.3)
    nan, inf = float("nan"), float("inf")
    return [
        (None, 2, ["edits is NULL"]),
        ([good], -1, ["n < 0"]),
        ([good, raw_edit(rtsr, 5, 0, 0.1)], None, ["edits[1].what"]),
        ([raw_edit(rtsr, -1, 0, 0.1)], None, ["edits[0].what"]),
        ([raw_edit(rtsr, S, info["n_textures"], 0.1, 0.2, 0.3)], None, ["edits[0].index", "out of range", "%d textures" % info["n_textures"]]),
        ([raw_edit(rtsr, S, -1, 0.1, 0.2, 0.3)], None, ["edits[0].index", "out of range"]),
        ([good, raw_edit(rtsr, M, info["n_materials"], 0.1, 0.2, 0.3, 0.0)], None, ["edits[1].index", "%d materials" % info["n_materials"]]),
        ([raw_edit(rtsr, F, info["n_top_level"], 1.0)], None, ["edits[0].index", "%d top-level slots" % info["n_top_level"]]),
        ([raw_edit(rtsr, M, lam, 0.1, 0.2, 0.3, 0.0)], None, ["edits[0].index", "not a Metal", "Lambertian", "edit its texture `tex` (%d" % shared]),
        ([raw_edit(rtsr, S, checker, 0.1, 0.2, 0.3)], None, ["edits[0].index", "not a SolidColor", "Checker", "children"]),
        ([raw_edit(rtsr, N, shared, 2.0)], None, ["edits[0].index", "not a Noise", "RTX_SHADE_SOLID_COLOR"]),
        ([raw_edit(rtsr, M, glass, 0.1, 0.2, 0.3, 0.0)], None, ["edits[0].index", "not a Metal", "RTX_SHADE_DIELECTRIC"]),
        ([raw_edit(rtsr, D, lam, 1.5)], None, ["edits[0].index", "not a Dielectric", "edit its texture"]),
        ([raw_edit(rtsr, F, 0, 1.0)], None, ["edits[0].index", "not a ConstantMedium"]),
        ([good, raw_edit(rtsr, F, fog_slot, nan)], None, ["edits[1].v[0] is not finite"]),
        ([raw_edit(rtsr, S, shared, 0.1, inf, 0.3)], None, ["edits[0].v[1] is not finite"]),
        ([raw_edit(rtsr, D, glass, -inf)], None, ["edits[0].v[0] is not finite"]),
        ([raw_edit(rtsr, S, shared, 0.1, 0.2, 0.3, 0.5)], None, ["edits[0].v[3]", "must be 0"]),
        ([raw_edit(rtsr, F, fog_slot, 1.0, 0.0, nan)], None, ["edits[0].v[2]", "must be 0"]),
        ([good, raw_edit(rtsr, F, fog_slot, 1.0), good], None, ["texture %d twice" % shared]),
        ([raw_edit(rtsr, F, fog_slot, 1.0), raw_edit(rtsr, F, fog_slot, 2.0)], None, ["slot %d twice" % fog_slot]),
    ]
