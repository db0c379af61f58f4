"""The host checker, the scenes and the analytic model of tests/test_features_cases.py, tests/test_gpu_features.py and the two
analytic tests of tests/test_gpu_denoise.py (a helper module, not a test file): everything here runs on the CPU.

The judge is tests/features_host_check.cpp built with oracle/Makefile's CXXFLAGS: once as it is (f64) and once with
o2_flat_f32.cpp's four defines (the float judge, linked to liboracle.so for oracle_f32_images).  It returns, per pixel, the
averaged albedo and normal (float32) and `hits`, the number of the pixel's feature samples that hit anything.

A case is a small frame (at most 1920 pixels) of one scene with its own feature_spp; between them the cases use 1, 3, 4 and 64
samples and reach every texture kind, a lens, a shutter, every primitive kind, a BVH, sphere and box media of ordinary density,
every material kind, an instance tree (P_INST) and GravitySpheres (P_ALL).  The conditions every case must meet (enough pixels
whose samples disagree, all hit and all miss; both colours of a medium; several texture values) are checked from `hits` and
the checker's albedo by tests/test_features_cases.py, on the CPU alone.

Two kinds of case cannot have a pixel whose samples disagree about hitting: a closed room and Book-2 inside its fog sphere,
where every ray hits something (mesh_open puts a triangle BVH in the open for that reason).  Such a case says so (`closed`) and takes ONE sample per pixel, the count at which the
condition on disagreeing samples does not apply; the conditions on misses are waived for it, with that reason."""
import ctypes as C
import os
import subprocess

import numpy as np

from instance_scenes import member_zoo, zoo_cam_cfg, zoo_image
from trace_rays_cases import CXXFLAGS, ORACLE_BUILD, gravity_time_limit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "features_host_check.cpp")

_D = C.POINTER(C.c_double)
_F = C.POINTER(C.c_float)
_ARGS = [C.c_void_p, _D, _D, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, _F, _F, C.POINTER(C.c_int32)]
_checkers = {}


def checkers(tmp_path_factory):
    """{False: the f64 judge's entry, True: the float judge's}, built once per session (needs liboracle.so: the orc fixture)."""
    if not _checkers:
        d = tmp_path_factory.mktemp("features_host")
        out64, out32 = str(d / "features_host_check.so"), str(d / "features_host_check_f32.so")
        subprocess.run(["g++"] + CXXFLAGS + ["-shared", SRC, "-o", out64], check=True)
        subprocess.run(["g++"] + CXXFLAGS + ["-DFEATURES_HOST_F32", "-shared", SRC, os.path.join(ORACLE_BUILD, "liboracle.so"),
                        "-Wl,-rpath," + ORACLE_BUILD, "-o", out32], check=True)
        for f32, path, name in ((False, out64, "features_host"), (True, out32, "features_host_f32")):
            fn = getattr(C.CDLL(path), name)
            fn.restype, fn.argtypes = C.c_int, _ARGS
            _checkers[f32] = fn
    return _checkers


def host_features(chk, flat, cam, cfg, height, feature_spp, f32=False):
    """The judge's (albedo, normal, hits) of a frame: float32 (h, w, 3) twice and int32 (h, w); row 0 is the bottom row."""
    w = cfg.image_width
    camera = np.frombuffer(bytes(cam), dtype=np.float64).copy()
    assert camera.size == 24
    bg = np.array(cfg.background[:], dtype=np.float64)
    albedo = np.zeros((height, w, 3), dtype=np.float32)
    normal = np.zeros_like(albedo)
    hits = np.zeros((height, w), dtype=np.int32)
    rc = chk[f32](flat.arrays_ptr(), camera.ctypes.data_as(_D), bg.ctypes.data_as(_D), w, height, feature_spp, cfg.max_depth,
                  cfg.seed, albedo.ctypes.data_as(_F), normal.ctypes.data_as(_F), hits.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, rc
    return albedo, normal, hits


def same_bits(a, b):
    """float32 arrays equal bit for bit."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def first_difference(got, ref):
    """"n of N pixels differ; first (j, i): got ..., checker ..." for two (h, w, 3) float32 planes."""
    bad = np.argwhere((got.view(np.uint32) != ref.view(np.uint32)).any(axis=2))
    if len(bad) == 0:
        return "equal"
    j, i = int(bad[0][0]), int(bad[0][1])
    return "%d of %d pixels differ; first (j, i) = (%d, %d): got %r, checker %r" % (len(bad), got.shape[0] * got.shape[1], j, i,
                                                                                     got[j, i].tolist(), ref[j, i].tolist())


# ---- the sample streams and primary rays, restated in numpy (core/rng.hpp, core/integrator.hpp: path_begin) ----
def oracle_stream(orc):
    """(seed, pixel, sample, n) -> the stream's first n uniforms, from the CPU oracle (rtsr.device_stream's CPU twin)."""
    def stream(seed, pixel, sample, n):
        out = np.empty(n, dtype=np.float64)
        orc.load().oracle_sample_stream(seed, pixel, sample, n, out.ctypes.data_as(_D))
        return out
    return stream


def primary_ray(stream, cam, cfg, height, i, j, s):
    """Path sample s of pixel (i, j) -> (origin, direction, time), f64.  The stream's k-th uniform is (x_k >> 11) 2^-53 of
    the k-th 64-bit output x_k; gen_range(lo..hi) takes its mantissa from x_k >> 12 = floor(uniform 2^52): the jitter (two
    uniforms), the lens sample (pairs in [-1, 1) until one lies in the unit disk) and the shutter time (camera.rs:59-71)."""
    w = cfg.image_width
    u = stream(cfg.seed, j * w + i, s, 64)
    o = np.array(cam.origin[:])
    llc, hor, ver = np.array(cam.lower_left_corner[:]), np.array(cam.horizontal[:]), np.array(cam.vertical[:])
    mant = np.floor(u * 2.0 ** 52)  # x_k >> 12, exact
    k = 2
    while True:
        x, y = (2.0 + mant[k] * 2.0 ** -51) + -3.0, (2.0 + mant[k + 1] * 2.0 ** -51) + -3.0
        k += 2
        if x * x + y * y + 0.0 < 1.0:
            break
    rd = cam.lens_radius * np.array([x, y, 0.0])
    offset = np.array(cam.u[:]) * rd[0] + np.array(cam.v[:]) * rd[1]
    d = llc + ((i + u[0]) / (w - 1)) * hor + ((j + u[1]) / (height - 1)) * ver - o - offset
    scale = cam.time2 - cam.time1
    time = (1.0 + mant[k] * 2.0 ** -52) * scale + (cam.time1 - scale)
    return o + offset, d, time


def analytic_features(rtsr, cam, cfg, center, radius, feature_spp, stream=None):
    """Per pixel: how many of the feature samples hit the sphere, and the average of the hit normals (numpy, f64).  For a
    camera without a lens.  stream: rtsr.device_stream (the default) or oracle_stream(orc), its CPU twin."""
    stream = stream or rtsr.device_stream
    w, h = cfg.image_width, rtsr.image_height(cfg)
    o = np.array(cam.origin[:])
    llc, hor, ver = np.array(cam.lower_left_corner[:]), np.array(cam.horizontal[:]), np.array(cam.vertical[:])
    hits = np.zeros((h, w), dtype=np.int32)
    nsum = np.zeros((h, w, 3))
    for j in range(h):
        for i in range(w):
            for s in range(feature_spp):
                ru, rv = stream(cfg.seed, j * w + i, s, 2)
                d = llc + ((i + ru) / (w - 1)) * hor + ((j + rv) / (h - 1)) * ver - o
                oc = o - center
                a, half_b, c = d @ d, oc @ d, oc @ oc - radius * radius
                disc = half_b * half_b - a * c
                if disc < 0:
                    continue
                t = (-half_b - np.sqrt(disc)) / a
                if t < 1e-3:
                    continue
                hits[j, i] += 1
                nsum[j, i] += (o + t * d - center) / radius
    return hits, nsum / feature_spp


# ---- the cases ----
class Case:
    """One frame.  closed: why no ray can miss (None: an open scene).  media: [(window, medium colour, colour behind it)] with
    window = (j0, j1, i0, i1), a pixel rectangle inside the medium's outline: among the first samples of its pixels some must
    end in the medium and some on what lies behind.  textured: the albedo must take >= 3 values beside the background.
    f32_exact: no sample reaches a platform function (tests/test_gpu_f32_parity.py: EXACT_CASES draws that line), and the
    scene has neither a lens nor a RotateY, which are left to the f64 comparison.  ray_query: the frame's normals are recomputed through the oracle's
    world_hit -- not for media, whose free path is drawn from the path's own stream, which that probe does not continue."""

    def __init__(self, name, builder, world, cam, cfg, height, spp, closed=None, media=(), textured=False, f32_exact=False,
                 ray_query=True, sphere=None):
        self.name, self.builder, self.world, self.cam, self.cfg, self.height, self.spp = name, builder, world, cam, cfg, height, spp
        self.closed, self.media, self.textured, self.f32_exact, self.ray_query = closed, media, textured, f32_exact, ray_query
        self.sphere = sphere  # (centre, radius, colour) of the one-sphere scene, where the analytic model applies
        self.flat = builder.flatten(world)
        assert closed is None or spp == 1


BACKGROUND = (0.7, 0.8, 1.0)


def _cfg(rtsr, aspect, width, seed, background=BACKGROUND):
    cfg = rtsr.Config.new(aspect, width, 8, 50, 4, seed=seed, background=background)
    return cfg, rtsr.image_height(cfg)


def one_sphere(rtsr):
    """The scene of test_gpu_denoise.py's analytic tests: one Lambertian sphere in front of the sky."""
    b = rtsr.Builder(1)
    colour, center, radius = (0.3, 0.6, 0.9), np.array([0.0, 0.0, -3.0]), 1.2
    world = b.hittable_list([b.sphere(tuple(center), radius, b.lambertian(colour))])
    cam = rtsr.Camera.new((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 60.0, 1.5, 0.0, 1.0, 0.0, 1.0)
    cfg, h = _cfg(rtsr, 1.5, 36, 5)
    return Case("one_sphere", b, world, cam, cfg, h, 4, f32_exact=True, sphere=(center, radius, np.float32(colour)))


def _textures(rtsr):
    """A checker, a Perlin and an image texture under a Lambertian, on three spheres before the sky; the odd frame 33 x 17."""
    b = rtsr.Builder(2)
    mats = [b.lambertian(b.checker_from_colors((0.1, 0.3, 0.1), (0.9, 0.9, 0.9))), b.lambertian(b.noise(4.0)),
            b.lambertian(b.image_from_texels(zoo_image()))]
    world = b.hittable_list([b.sphere((x, 0.0, -5.0), 1.0, m) for x, m in zip((-2.3, 0.0, 2.3), mats)])
    cam = rtsr.Camera.new((0.0, 0.5, 0.0), (0.0, 0.0, -5.0), (0.0, 1.0, 0.0), 40.0, 33.0 / 17.0, 0.0, 1.0, 0.0, 1.0)
    cfg, h = _cfg(rtsr, 33.0 / 17.0, 33, 21)
    assert h == 17
    return Case("textures", b, world, cam, cfg, h, 3, textured=True)


def _moving_defocus(rtsr):
    """The catalogue's moving-sphere test with its own camera: aperture 0.1, shutter 2 .. 2.5, a BVH, a checker ground."""
    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(rtsr.SCENE_MOVING_TEST)
    assert cam.lens_radius > 0.0 and cam.time1 < cam.time2
    cfg, h = _cfg(rtsr, 16.0 / 9.0, 48, 22, bg)
    return Case("moving_defocus", b, world, cam, cfg, h, 4, textured=True)


def _cornell(rtsr, sid, name, spp, seed, **kw):
    """A Cornell room seen through its open side from the catalogue's viewpoint, with a field of view of 50 degrees in place of
    40 and a slight roll, so that the room's outline crosses the pixel rows: the walls' inner faces (face-forwarded normals),
    the boxes, and the background around the room."""
    b = rtsr.Builder(1)
    world, _, bg = b.get_world_cam(sid)
    cam = rtsr.Camera.new((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), (0.08, 1.0, 0.0), 50.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    cfg, h = _cfg(rtsr, 1.0, 40, seed, (0.05, 0.1, 0.2))
    return Case(name, b, world, cam, cfg, h, spp, **kw)


def _mesh_room(rtsr):
    """The catalogue's mesh room: 2000 triangles behind a BVH between rectangles seen from inside.  The rectangles close the
    room (walls and ceiling reach 100 units beyond the corners), so no ray misses."""
    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(rtsr.SCENE_STANFORD_DRAGON, mesh_triangles=2000)
    cfg, h = _cfg(rtsr, 16.0 / 9.0, 48, 24, bg)
    return Case("mesh_room", b, world, cam, cfg, h, 1, closed="the room's rectangles enclose the camera", f32_exact=True)


def _mesh_open(rtsr):
    """A torus of 2048 triangles behind a BVH, lying over a metal floor rectangle before a Lambertian panel, in the open: the
    triangle BVH at three samples per pixel, with outlines against the sky.  (No vertex ring lies in an axis plane.)"""
    b = rtsr.Builder(1)
    n = 32
    u, v = np.meshgrid(0.1 + 2.0 * np.pi * np.arange(n) / n, 0.07 + 2.0 * np.pi * np.arange(n) / n, indexing="ij")
    ring = 1.0 + 0.4 * np.cos(v)
    vertices = np.stack([ring * np.cos(u), 0.55 + 0.4 * np.sin(v), ring * np.sin(u) - 4.0], axis=-1).reshape(-1, 3)
    idx = lambda a, c: (a % n) * n + (c % n)
    faces = [f for a in range(n) for c in range(n)
             for f in ((idx(a, c), idx(a + 1, c), idx(a + 1, c + 1)), (idx(a, c), idx(a + 1, c + 1), idx(a, c + 1)))]
    mesh = b.bvh_from_list(b.triangle_mesh(vertices, faces, b.lambertian((0.7, 0.5, 0.2))), 0.0, 1.0)
    world = b.hittable_list([mesh, b.xz_rect(-1.8, 1.8, -5.5, -2.5, 0.1, b.metal((0.6, 0.6, 0.7), 0.1)),
                             b.xy_rect(-0.9, 1.6, 0.1, 1.9, -5.6, b.lambertian((0.2, 0.3, 0.8)))])
    cam = rtsr.Camera.new((0.3, 2.2, 0.0), (0.0, 0.5, -4.0), (0.0, 1.0, 0.0), 50.0, 1.5, 0.0, 1.0, 0.0, 1.0)
    cfg, h = _cfg(rtsr, 1.5, 48, 30)
    return Case("mesh_open", b, world, cam, cfg, h, 3, f32_exact=True)


def _book2(rtsr):
    """Book-2's final scene, reduced: the fog (density 1e-4) spans the scene inside a glass sphere of radius 5000, so every ray
    ends in the fog, on an object or on that sphere.  Also a moving sphere, image and Perlin textures, Translate o RotateY."""
    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(rtsr.SCENE_BOOK2_FINAL, book2_boxes_per_side=4, book2_spheres=50)
    cfg, h = _cfg(rtsr, 1.0, 40, 25, bg)
    # the fog before the cluster of white spheres (0.73) in the upper middle of the frame.  (The blue smoke ball lies inside a
    # glass sphere of its own: the first hit there is the glass.)
    return Case("book2", b, world, cam, cfg, h, 1, closed="the fog's glass sphere encloses the scene", ray_query=False,
                media=[((19, 28, 19, 30), np.float32((1.0, 1.0, 1.0)), np.float32((0.73, 0.73, 0.73)))], textured=True)


SMOKE, BEHIND, SOLID = (0.2, 0.4, 0.9), (0.8, 0.2, 0.1), (0.2, 0.7, 0.3)


def _sphere_media(rtsr):
    """Media over spheres at the catalogue's densities: a smoke ball (0.01, Cornell's, over a sphere of radius 80: an optical
    depth of at most 1.6, so a good share of its rays cross it) before a red wall, inside a fog (1e-4, Book-2's) that spans the
    scene in a sphere of radius 5000 -- without Book-2's glass shell, so that a ray the fog lets through can miss."""
    b = rtsr.Builder(4)
    grey = b.lambertian((0.5, 0.5, 0.5))
    world = b.hittable_list([
        b.sphere((-110.0, 0.0, 0.0), 60.0, b.lambertian(SOLID)),
        b.constant_medium(SMOKE, 0.01, b.sphere((90.0, 0.0, 0.0), 80.0, grey)),
        b.xy_rect(0.0, 200.0, -110.0, 110.0, 300.0, b.lambertian(BEHIND)),
        b.constant_medium((1.0, 1.0, 1.0), 0.0001, b.sphere((0.0, 0.0, 0.0), 5000.0, grey))])
    cam = rtsr.Camera.new((0.0, 0.0, -600.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.5, 0.0, 10.0, 0.0, 1.0)
    cfg, h = _cfg(rtsr, 1.5, 48, 26, (0.05, 0.1, 0.2))
    # windows inside the smoke ball's outline (before the wall) and inside the solid sphere's (before which lies only fog)
    return Case("sphere_media", b, world, cam, cfg, h, 3, ray_query=False,
                media=[((12, 19, 14, 21), np.float32(SMOKE), np.float32(BEHIND)),
                       ((12, 19, 29, 35), np.float32((1.0, 1.0, 1.0)), np.float32(SOLID))])


def _materials(rtsr):
    """Metal, Dielectric, DiffuseLight and Lambertian spheres in a row across a frame of 64 x 4: one filter block's pixels."""
    b = rtsr.Builder(1)
    mats = [b.metal((0.8, 0.5, 0.25), 0.3), b.dielectric(1.5), b.diffuse_light((4.0, 3.0, 2.0)), b.lambertian((0.25, 0.75, 0.5)),
            b.metal((0.3, 0.4, 0.9), 0.0), b.dielectric(1.3), b.diffuse_light((0.5, 0.5, 0.5))]
    world = b.hittable_list([b.sphere((-2.1 + 0.7 * k, 0.0, -4.0), 0.22, m) for k, m in enumerate(mats)])
    cam = rtsr.Camera.new((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 3.6, 16.0, 0.0, 1.0, 0.0, 1.0)
    cfg, h = _cfg(rtsr, 16.0, 64, 7, (0.1, 0.2, 0.3))
    assert h == 4
    return Case("materials", b, world, cam, cfg, h, 4, f32_exact=True)


def _zoo(rtsr):
    """The member zoo as one instance tree (tests/instance_scenes.py): preset P_INST."""
    b, world = member_zoo(rtsr, "instanced", "middle")
    cam, cfg, h = zoo_cam_cfg(rtsr, width=48)
    c = Case("zoo", b, world, cam, cfg, h, 3, textured=True)
    assert c.flat.instances()["n_trees"] == 1
    return c


def _gravity(rtsr):
    """The GravitySphere scene (preset P_ALL) with the catalogue's lens and a shutter that ends at the stored time limit."""
    b = rtsr.Builder(1)
    world, cam0, bg = b.get_world_cam(rtsr.SCENE_RANDOM_MOVING)
    cam = rtsr.Camera.new((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, 16.0 / 9.0, 0.1, 10.0, 0.0, gravity_time_limit())
    assert cam.lens_radius == cam0.lens_radius
    cfg, h = _cfg(rtsr, 16.0 / 9.0, 48, 27, bg)
    return Case("gravity", b, world, cam, cfg, h, 4)


def _book1(rtsr):
    """Book 1's final scene (a BVH of Lambertian, Metal and Dielectric spheres) through a pinhole."""
    b = rtsr.Builder(1)
    world, _, bg = b.get_world_cam(rtsr.SCENE_BOOK1_CANONICAL)
    cam = rtsr.Camera.new((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, 1.5, 0.0, 10.0, 0.0, 1.0)
    cfg, h = _cfg(rtsr, 1.5, 48, 28, bg)
    return Case("book1", b, world, cam, cfg, h, 4, f32_exact=True)


CASES = {
    "one_sphere": one_sphere,
    "textures": _textures,
    "moving_defocus": _moving_defocus,
    # rectangles and boxes (Translate o RotateY over a prism), 64 samples
    "cornell_box": lambda r: _cornell(r, r.SCENE_CORNELL_BOX, "cornell_box", 64, 23),
    # media over boxes at Cornell's density 0.01: black smoke over the tall box, white over the short one, each before the
    # white back wall (0.73); the windows lie inside the boxes' outlines
    "box_media": lambda r: _cornell(r, r.SCENE_CORNELL_SMOKE, "box_media", 4, 29, ray_query=False,
                                    media=[((10, 21, 14, 19), np.float32((0, 0, 0)), np.float32((0.73, 0.73, 0.73))),
                                           ((8, 14, 21, 27), np.float32((1, 1, 1)), np.float32((0.73, 0.73, 0.73)))]),
    "mesh_room": _mesh_room,
    "mesh_open": _mesh_open,
    "book2": _book2,
    "sphere_media": _sphere_media,
    "materials": _materials,
    "zoo": _zoo,
    "gravity": _gravity,
    "book1": _book1,
}
# no noise or image texture, no medium, no lens, no RotateY: spheres, a sphere BVH, and rectangles and triangles behind a BVH
F32_EXACT = ("one_sphere", "materials", "book1", "mesh_room", "mesh_open")
_built, _refs = {}, {}


def case(rtsr, name):
    """The named case, built once per session; no device is touched."""
    if name not in _built:
        _built[name] = CASES[name](rtsr)
        assert _built[name].f32_exact == (name in F32_EXACT)
    return _built[name]


def reference(chk, rtsr, name, spp=None, f32=False):
    """The checker's (albedo, normal, hits) of a case at spp samples (its own by default): computed once, never written to."""
    c = case(rtsr, name)
    key = (name, spp or c.spp, f32)
    if key not in _refs:
        _refs[key] = host_features(chk, c.flat, c.cam, c.cfg, c.height, key[1], f32=f32)
        for a in _refs[key]:
            a.setflags(write=False)
    return _refs[key]


# ---- the large frame: the second trip of k_features' grid-stride loop ----
FEATURE_GRID_WAVES = 8 * 256  # features_impl: at most n_cu * 8 blocks of 256 lanes


def large_case(rtsr, n_cu):
    """Three spheres before the sky, one sample per pixel, on the smallest frame 1024 pixels wide that holds more than
    n_cu * 8 * 256 pixels: the pixels beyond that count are the ones a lane reaches on its second trip."""
    b = rtsr.Builder(1)
    world = b.hittable_list([b.sphere((0.0, -100.5, -1.0), 100.0, b.lambertian((0.8, 0.8, 0.0))),
                             b.sphere((-0.6, 0.0, -1.2), 0.5, b.metal((0.8, 0.6, 0.2), 0.0)),
                             b.sphere((0.6, 0.0, -1.0), 0.5, b.lambertian((0.1, 0.2, 0.5)))])
    w = 1024
    h = n_cu * FEATURE_GRID_WAVES // w + 1
    aspect = w / (h + 0.5)  # image_height truncates w / aspect
    cam = rtsr.Camera.new((0.0, 0.3, 1.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 60.0, aspect, 0.0, 1.0, 0.0, 1.0)
    cfg, height = _cfg(rtsr, aspect, w, 31)
    assert height == h and w * h > n_cu * FEATURE_GRID_WAVES
    return Case("large", b, world, cam, cfg, h, 1)
