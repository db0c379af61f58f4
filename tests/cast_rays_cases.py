"""Scenes and ray sets of tests/test_gpu_cast_rays.py (a helper module, not a test file): everything here runs on the CPU.

A case is a flattened scene plus R rays from a fixed numpy seed: origins on a sphere around an aim box, directed at uniform
points of that box, then 100 more rays whose t_max is cut to a random fraction of their free hit distance (the oracle's).  The
aim box and the radius are chosen per scene so that the oracle's own answers hold at least 25 % hits and 10 % misses
(check_mix; a closed room or a ground sphere of radius 1000 would otherwise be hit by every ray): the box is the region of
interest a little enlarged, not the scene's tight box.
"""
import numpy as np

from instance_scenes import member_zoo

T_MIN = 0.001
CUT_RAYS = 100


def sphere_rays(n, seed, lo, hi, radius_factor):
    """n rays: origins uniform on the sphere of radius radius_factor x the half diagonal of [lo, hi] around its centre, aimed
    at uniform points of the box (directions not normalised).  float64 (n, 3) arrays."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    centre, radius = 0.5 * (lo + hi), radius_factor * 0.5 * np.linalg.norm(hi - lo)
    v = rng.normal(size=(n, 3))
    o = centre + radius * v / np.linalg.norm(v, axis=1, keepdims=True)
    target = lo + rng.uniform(size=(n, 3)) * (hi - lo)
    return np.ascontiguousarray(o), np.ascontiguousarray(target - o)


class Case:
    """name, builder, flat, rays (o, d, time, t_max) and -- after oracle() -- the oracle's records as an (n, 11) array."""

    def __init__(self, name, builder, world, lo, hi, radius_factor, n=1900, seed=1, times=None, f32=False, max_leaf=0, reach=np.inf):
        self.name, self.builder, self.world, self.f32 = name, builder, world, f32
        self.flat = builder.flatten(world, max_leaf=max_leaf)
        self.box = (lo, hi, radius_factor)
        self.n_free, self.seed = n, seed
        self.time_range = times
        self.reach = reach  # t_max of the free rays (inf: unbounded)
        self.o = self.d = self.time = self.t_max = None

    def build_rays(self, orc):
        """The free rays, then CUT_RAYS copies of hitting free rays with t_max = fraction x their free t."""
        rng = np.random.default_rng(self.seed + 1000)
        o, d = sphere_rays(self.n_free, self.seed, *self.box)
        time = np.zeros(self.n_free) if self.time_range is None else rng.uniform(self.time_range[0], self.time_range[1], self.n_free)
        free = records(orc, self, o, d, time, np.full(self.n_free, self.reach), seed=1, stream_step=0)
        hitting = np.flatnonzero((free[:, 0] == 1.0) & np.isfinite(free[:, 1]))
        pick = hitting[rng.integers(len(hitting), size=CUT_RAYS)]
        cut = free[pick, 1] * rng.uniform(0.05, 0.95, CUT_RAYS)
        self.o = np.ascontiguousarray(np.concatenate([o, o[pick]]))
        self.d = np.ascontiguousarray(np.concatenate([d, d[pick]]))
        self.time = np.ascontiguousarray(np.concatenate([time, time[pick]]))
        self.t_max = np.ascontiguousarray(np.concatenate([np.full(self.n_free, self.reach), cut]))
        return self

    @property
    def n(self):
        return len(self.o)


def records(orc, case, o, d, time, t_max, seed, stream_step):
    """The oracle's answer to every ray, one call each: (n, 11) = hit, t, p, normal, u, v, front_face (zeros on a miss)."""
    probe = orc.core32_world_hit if case.f32 else orc.core_world_hit
    ptr = case.flat.arrays_ptr()
    out = np.zeros((len(o), 11))
    for r in range(len(o)):
        rec = probe(ptr, tuple(o[r]), tuple(d[r]), float(time[r]), T_MIN, float(t_max[r]), rng_seed=seed + r * stream_step)
        if rec is not None:
            out[r] = [1.0, rec["t"], *rec["p"], *rec["normal"], rec["u"], rec["v"], float(rec["front_face"])]
    return out


def check_mix(name, rec):
    """The input condition, from the oracle's answers alone: at least 25 % hits and at least 10 % misses."""
    hits = int(rec[:, 0].sum())
    print("%s: %d rays, %d hits, %d misses" % (name, len(rec), hits, len(rec) - hits))
    assert 4 * hits >= len(rec), (name, hits, len(rec))
    assert 10 * (len(rec) - hits) >= len(rec), (name, hits, len(rec))


def hits_as_records(h):
    """A RayHits with every column (numpy) in the layout of records(): +inf t of a miss becomes 0, as the oracle's row."""
    hit = h.ids[:, 0] == 1
    out = np.zeros((h.n, 11))
    out[:, 0] = hit
    out[:, 1] = np.where(hit, h.t, 0.0)
    out[:, 2:5], out[:, 5:8], out[:, 8:10] = h.p, h.normal, h.uv
    out[:, 10] = h.ids[:, 3]
    return out


def same_bits(a, b):
    """Bit for bit up to the payload of a NaN (tests/test_instance_tree.py: _same_bits): equal values with NaN == NaN, and
    equal signs wherever the value is not a NaN (which tells -0.0 from 0.0).  -> a boolean per row."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    eq = ((a == b) | (na & nb)) & ((np.signbit(a) & ~na) == (np.signbit(b) & ~nb))
    return eq.reshape(len(a), -1).all(axis=1)


# ---- the scenes.  (lo, hi, radius factor) were fitted on the CPU with the oracle alone; check_mix holds them to it. ----
def _catalogue(rtsr, name, scene_id, lo, hi, rf, times=None, seed=1, f32=False, reach=np.inf, **kw):
    b = rtsr.Builder(1)
    world, cam, _ = b.get_world_cam(scene_id, **kw)
    if times == "shutter":
        times = (cam.time1, cam.time2)
    return Case(name, b, world, lo, hi, rf, times=times, seed=seed, f32=f32, reach=reach)


def _zoo(rtsr, layout, f32=False, plain=False):
    b, world = member_zoo(rtsr, "instanced", layout, plain=plain)
    return Case("zoo_%s%s" % (layout, "_f32" if f32 else ""), b, world, (-8.0, -0.5, -6.5), (8.0, 6.0, 5.5), 1.0,
                seed=40 + len(layout), f32=f32)


F64_CASES = {
    # media draws
    "cornell_smoke": lambda r: _catalogue(r, "cornell_smoke", r.SCENE_CORNELL_SMOKE, (-250.0, -250.0, -250.0), (805.0, 805.0, 805.0), 0.9, seed=2),
    # BVH of boxes, Translate o RotateY, a medium, a moving sphere: times drawn in the shutter.  The fog's sphere of radius
    # 5000 holds the whole scene and every unbounded ray ends in it, so the free rays of this scene reach to t = 2 (about
    # twice the way to the aimed point: a range-limited sensor); beyond it a ray is a miss
    "book2": lambda r: _catalogue(r, "book2", r.SCENE_BOOK2_FINAL, (-50.0, 50.0, -50.0), (600.0, 600.0, 600.0), 0.8, times="shutter", seed=3,
                                  reach=2.0, book2_boxes_per_side=4, book2_spheres=50),
    "moving_test": lambda r: _catalogue(r, "moving_test", r.SCENE_MOVING_TEST, (-8.0, -1.0, -8.0), (8.0, 8.0, 8.0), 1.0, times="shutter", seed=4),
    # GravitySpheres, at two times (P_ALL)
    "gravity_t0.37": lambda r: _catalogue(r, "gravity_t0.37", r.SCENE_RANDOM_MOVING, (-12.0, -1.0, -12.0), (12.0, 14.0, 12.0), 1.0, times=(0.37, 0.37), seed=5),
    "gravity_t6.2": lambda r: _catalogue(r, "gravity_t6.2", r.SCENE_RANDOM_MOVING, (-12.0, -1.0, -12.0), (12.0, 14.0, 12.0), 1.0, times=(6.2, 6.2), seed=6),
    # triangles under a BVH beside plain rectangles (P_ANY)
    "mesh_room": lambda r: _catalogue(r, "mesh_room", r.SCENE_STANFORD_DRAGON, (-160.0, -60.0, -160.0), (160.0, 120.0, 160.0), 0.9, seed=7, mesh_triangles=8000),
    # instance trees (P_INST), two layouts of the member zoo
    "zoo_middle": lambda r: _zoo(r, "middle"),
    "zoo_two": lambda r: _zoo(r, "two"),
}
MEDIUM_CASES = ("cornell_smoke", "book2")

# f32 scenes, bit for bit against core32_world_hit: no platform function (sinf, logf, ...) is reached by these two.  The
# medium scenes do reach logf (the medium's distance draw) and are NOT in this set: they are not compared bit for bit.
F32_CASES = {
    "book1_f32": lambda r: _catalogue(r, "book1_f32", r.SCENE_BOOK1_CANONICAL, (-12.0, -1.0, -12.0), (12.0, 14.0, 12.0), 1.0, seed=8, f32=True),
    "zoo_plain_f32": lambda r: _zoo(r, "middle", f32=True, plain=True),
}
