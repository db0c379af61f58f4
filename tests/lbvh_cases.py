"""Inputs that stress the GPU BVH builder (csrc/hip/lbvh.hip): equal Morton codes in bulk, axes without centroid extent, a short
last leaf, coincident primitives of different materials, inverted boxes, moving spheres, and trees that are chains.

Every constructor returns (builder, world, cam, cfg, probes): a world of ONE bvh_from_list of at least 1024 primitives (the GPU
builder's threshold, flatten.cpp) and a light -- a rectangle beside the BVH in the world list, so the world is k_trace_vote's;
`movers` is lit by its background alone and stays a sphere world, k_trace_lds's.  probes: (n, 3) centres of the primitives,
for rays aimed at what the camera does not see.  tests/test_lbvh_cases.py proves the scenes on the CPU (O1 == O2 through the
host builder); tests/test_gpu_lbvh_edges.py runs the GPU builder on them.  Frames: at most 96 px wide, at most 4 spp."""
import numpy as np

SKY = (0.55, 0.65, 0.85)


def _cfg(rtsr, width=64, aspect=1.0, spp=2, depth=12, seed=11, background=SKY):
    return rtsr.Config.new(aspect, width, spp, depth, 4, seed=seed, background=background)


def _cam(rtsr, lookfrom, lookat, vfov=40.0, aspect=1.0, t0=0.0, t1=1.0):
    return rtsr.Camera.new(lookfrom, lookat, (0.0, 1.0, 0.0), vfov, aspect, 0.0, 10.0, t0, t1)


def _world(b, objs, light_y, half=4.0, centre=(0.0, 0.0), t0=0.0, t1=1.0, as_list=False):
    """[BvhNode::from_list(objs, t0, t1), a light of 2 * half square at height light_y]; as_list: [objs ..., the light]"""
    light = b.xz_rect(centre[0] - half, centre[0] + half, centre[1] - half, centre[1] + half, light_y, b.diffuse_light((5.0, 5.0, 5.0)))
    if as_list:
        return b.hittable_list(list(objs) + [light])
    return b.hittable_list([b.bvh_from_list(b.hittable_list(objs), t0, t1), light])


def _mats(b):
    return [b.lambertian((0.7, 0.3, 0.3)), b.metal((0.8, 0.8, 0.7), 0.1), b.dielectric(1.5), b.lambertian((0.3, 0.6, 0.8))]


def same_centroid(rtsr):
    """1500 concentric spheres, radii 0.1 .. 3, glass and lambertian in turn: ONE Morton code, the tree is the index tie-break's."""
    b = rtsr.Builder(1)
    glass, grey = b.dielectric(1.5), b.lambertian((0.6, 0.6, 0.5))
    radii = np.linspace(0.1, 3.0, 1500)
    objs = [b.sphere((0.0, 0.0, 0.0), float(r), glass if k % 2 == 0 else grey) for k, r in enumerate(radii)]
    world = _world(b, objs, 8.0)
    return b, world, _cam(rtsr, (0.0, 1.0, 9.0), (0.0, 0.0, 0.0)), _cfg(rtsr), np.zeros((1500, 3))


def threshold(rtsr, n):
    """n spheres on a jittered grid in the plane y = 0.3: 1023 stays with the host builder, 1024 and 1025 go to the device."""
    b = rtsr.Builder(2)
    mats = _mats(b)
    rng = np.random.default_rng(7)
    centres = []
    for k in range(n):
        i, j = divmod(k, 33)
        centres.append((0.5 * i - 8.0 + 0.15 * rng.random(), 0.3 + 0.2 * rng.random(), 0.5 * j - 8.0 + 0.15 * rng.random()))
    objs = [b.sphere(c, 0.17, mats[k % 4]) for k, c in enumerate(centres)]
    world = _world(b, objs, 6.0, half=6.0)
    return b, world, _cam(rtsr, (0.0, 9.0, 16.0), (0.0, 0.0, 0.0)), _cfg(rtsr), np.array(centres)


def odd_cluster(rtsr):
    """1031 (a prime) tilted triangles in a slab: n is no multiple of any cluster size."""
    b = rtsr.Builder(3)
    mats = _mats(b)
    rng = np.random.default_rng(8)
    objs, centres = [], []
    for k in range(1031):
        c = np.array([8.0 * rng.random() - 4.0, 2.0 * rng.random(), 8.0 * rng.random() - 4.0])
        v = [c + 0.35 * (rng.random(3) - 0.5) for _ in range(3)]
        objs.append(b.triangle(tuple(v[0]), tuple(v[1]), tuple(v[2]), mats[k % 4]))
        centres.append((v[0] + v[1] + v[2]) / 3.0)
    world = _world(b, objs, 6.0)
    return b, world, _cam(rtsr, (0.0, 5.0, 9.0), (0.0, 1.0, 0.0)), _cfg(rtsr), np.array(centres)


def coplanar(rtsr):
    """40 x 40 xz_rect tiles at one k: no centroid extent on y."""
    b = rtsr.Builder(4)
    mats = _mats(b)
    objs, centres = [], []
    for i in range(40):
        for j in range(40):
            x, z = 0.5 * i - 10.0, 0.5 * j - 10.0
            objs.append(b.xz_rect(x, x + 0.5, z, z + 0.5, 0.25, mats[(i + 2 * j) % 4]))
            centres.append((x + 0.25, 0.25, z + 0.25))
    world = _world(b, objs, 5.0)
    return b, world, _cam(rtsr, (0.3, 6.1, 14.2), (0.0, 0.0, 0.0)), _cfg(rtsr), np.array(centres)


def collinear(rtsr):
    """1300 spheres on a line parallel to x: no centroid extent on y and z."""
    b = rtsr.Builder(5)
    mats = _mats(b)
    centres = [(0.05 * k - 32.5, 0.5, 0.0) for k in range(1300)]
    objs = [b.sphere(c, 0.02 + 0.001 * (k % 7), mats[k % 4]) for k, c in enumerate(centres)]
    world = _world(b, objs, 4.0)
    return b, world, _cam(rtsr, (0.0, 1.5, 4.0), (0.0, 0.5, 0.0)), _cfg(rtsr, width=96, aspect=2.0), np.array(centres)


def outlier(rtsr):
    """1200 spheres in the unit cube and one at (1e9, 1e9, 1e9): every centroid but one quantises to Morton cell 0."""
    b = rtsr.Builder(6)
    mats = _mats(b)
    rng = np.random.default_rng(9)
    centres = [tuple(rng.random(3)) for _ in range(1200)] + [(1e9, 1e9, 1e9)]
    objs = [b.sphere(c, 0.02 if k < 1200 else 1.0e6, mats[k % 4]) for k, c in enumerate(centres)]
    world = _world(b, objs, 3.0, centre=(0.5, 0.5))
    return b, world, _cam(rtsr, (0.5, 1.2, 3.0), (0.5, 0.5, 0.5)), _cfg(rtsr), np.array(centres)


def coincident_tris(rtsr, as_list=False):
    """400 distinct triangles, each listed three times as three objects of three colours, in shuffled list order; plus 100
    triangles whose SAME handle is listed twice (the flattener then keeps a private leaf-ordered copy of the BVH's triangles).
    Every ray that meets one of the 400 ties three ways: which colour it sees is the tie rule's to say, not the builder's.
    as_list: the same objects as a plain HittableList (and the light), where hit.rs:676-680 lets the later object win."""
    b = rtsr.Builder(7)
    colours = [b.lambertian((0.9, 0.1, 0.1)), b.lambertian((0.1, 0.9, 0.1)), b.lambertian((0.1, 0.1, 0.9))]
    grey = b.lambertian((0.5, 0.5, 0.5))
    rng = np.random.default_rng(10)
    objs, centres = [], []
    for k in range(500):
        c = np.array([6.0 * rng.random() - 3.0, 2.0 * rng.random(), 6.0 * rng.random() - 3.0])
        v = [tuple(c + 0.6 * (rng.random(3) - 0.5)) for _ in range(3)]
        if k < 400:
            objs += [b.triangle(v[0], v[1], v[2], m) for m in colours]
        else:
            t = b.triangle(v[0], v[1], v[2], grey)
            objs += [t, t]
        centres.append(np.mean(np.array(v), axis=0))
    objs = [objs[k] for k in rng.permutation(len(objs))]
    world = _world(b, objs, 6.0, as_list=as_list)
    return b, world, _cam(rtsr, (0.0, 4.0, 8.0), (0.0, 1.0, 0.0)), _cfg(rtsr), np.array(centres)


def hollow_shells(rtsr, as_list=False):
    """Book-1's hollow glass (radius r and -0.9 r at one centre: the second's reference box is inverted) 300 times among 500
    plain spheres: 1100 spheres.  as_list: the same objects as a plain HittableList (and the light): no boxes at all."""
    b = rtsr.Builder(8)
    mats = _mats(b)
    glass = mats[2]
    rng = np.random.default_rng(11)
    objs, centres = [], []
    for k in range(800):
        c = (8.0 * rng.random() - 4.0, 0.2 + 1.6 * rng.random(), 8.0 * rng.random() - 4.0)
        r = 0.1 + 0.12 * rng.random()
        if k < 300:
            objs += [b.sphere(c, r, glass), b.sphere(c, -0.9 * r, glass)]
            centres += [c, c]
        else:
            objs.append(b.sphere(c, r, mats[k % 4]))
            centres.append(c)
    world = _world(b, objs, 6.0, as_list=as_list)
    return b, world, _cam(rtsr, (0.0, 4.0, 9.0), (0.0, 0.8, 0.0)), _cfg(rtsr), np.array(centres)


def movers(rtsr):
    """1200 spheres, three quarters of them moving along all three axes over the BVH's interval (0, 1); the shutter (0.2, 0.7)
    lies inside it.  A sphere world of one BVH, lit by the background."""
    b = rtsr.Builder(9)
    mats = _mats(b)
    objs, centres = [], []
    for k in range(1200):
        c0 = (10.0 * b.random() - 5.0, 0.2 + 2.0 * b.random(), 10.0 * b.random() - 5.0)
        r = 0.06 + 0.08 * b.random()
        if k % 4 == 0:
            objs.append(b.sphere(c0, r, mats[k % 3]))
        else:
            c1 = (c0[0] + 1.5 * b.random() - 0.75, c0[1] + 1.0 * b.random() - 0.25, c0[2] + 1.5 * b.random() - 0.75)
            objs.append(b.moving_sphere(c0, c1, 0.0, 1.0, r, mats[k % 4]))
        centres.append(c0)
    world = b.hittable_list([b.bvh_from_list(b.hittable_list(objs), 0.0, 1.0)])
    cam = _cam(rtsr, (6.0, 4.0, 9.0), (0.0, 0.8, 0.0), aspect=1.5, t0=0.2, t1=0.7)
    return b, world, cam, _cfg(rtsr, width=96, aspect=1.5, spp=4), np.array(centres)


def chain(rtsr, K):
    """For k < K and each axis a one sphere centred at 2^k + 0.5 on a (radius 2^k / 4), one sphere at 2097151 on all three,
    the rest of 1100 concentric at the origin.  The centroid bounds are 0 .. 2097151, so a centroid's 21-bit cell is its
    coordinate: every code but two has a single bit set and Karras' tree over them is a chain, about 4 levels per k."""
    b = rtsr.Builder(10)
    mats = _mats(b)
    centres = []
    radii = []
    for k in range(K):
        for a in range(3):
            c = [0.0, 0.0, 0.0]
            c[a] = 2.0 ** k + 0.5
            centres.append(tuple(c))
            radii.append(0.25 * 2.0 ** k)
    centres.append((2097151.0, 2097151.0, 2097151.0))
    radii.append(1.0)
    n_origin = 1100 - len(centres)
    centres += [(0.0, 0.0, 0.0)] * n_origin
    radii += list(np.linspace(0.05, 0.45, n_origin))
    objs = [b.sphere(c, float(r), mats[k % 4]) for k, (c, r) in enumerate(zip(centres, radii))]
    world = _world(b, objs, 40.0, half=10.0)
    return b, world, _cam(rtsr, (14.0, 10.0, 22.0), (2.0, 2.0, 2.0)), _cfg(rtsr), np.array(centres)


# id -> (constructor, its arguments, the max_leaf values the GPU tests build with); tall trees last
CASES = {
    "same_centroid": (same_centroid, (), (1,)),
    "threshold_1023": (threshold, (1023,), (1, 8)),
    "threshold_1024": (threshold, (1024,), (1, 8)),
    "threshold_1025": (threshold, (1025,), (1, 8)),
    "odd_cluster": (odd_cluster, (), (2, 3, 8)),
    "coplanar": (coplanar, (), (1,)),
    "collinear": (collinear, (), (1,)),
    "outlier": (outlier, (), (1,)),
    "coincident_tris": (coincident_tris, (), (2,)),
    "hollow_shells": (hollow_shells, (), (1, 4)),
    "movers": (movers, (), (1, 4)),
    "chain_12": (chain, (12,), (1,)),
    "chain_16": (chain, (16,), (1,)),
    "chain_18": (chain, (18,), (1,)),
}


def build(rtsr, case_id):
    fn, args, _ = CASES[case_id]
    return fn(rtsr, *args)
