"""What the cases and the tests of set_triangles and set_spheres share (a helper module, not a test file): the plumbing of a case
(deform_cases.py and sphere_update_cases.py keep the scenes, `refusals`, `update_of` and the dtypes of their kind), one raw call
of a set_* entry, and the helpers of the host and the GPU tests.  Everything but upload() and below runs on the CPU."""
import ctypes as C
import os

import numpy as np

from set_transforms_cases import NODE, NODE32

SWITCHES = ("RTX_TRACE_KERNEL", "RTX_WIDE")
KERNEL_OF = {"simple": "k_trace_simple", "vote": "k_trace_vote", "world": "k_trace_world", "wavefront": "k_wf_trace"}
INSTANCED_POSE = (((0.4, 0.2, 0.3), 20.0), ((3.1, 0.3, 2.2), -35.0), ((1.2, 0.4, 4.0), None))


class Case:
    def __init__(self, builder, world, parts, flatten=None, look=((2.3, 5.0, 8.5), (2.3, 1.0, 2.4))):
        self.builder, self.world, self.parts, self.flatten_opt, self.look = builder, world, parts, dict(flatten or {}), look

    def flatten(self):
        return self.builder.flatten(self.world, **self.flatten_opt)


class Maker:
    """Adds updatable primitives to a builder and notes (handle, rest values, moved values) per part.  moved: False (at rest),
    True (every primitive moved) or a predicate on the primitive's position in update_of's full list -- the fresh scene of a
    partial update.  A kind's module adds the methods that make its primitives."""

    def __init__(self, rtsr, seed, moved):
        self.b, self.moved, self.parts, self.k = rtsr.Builder(seed), moved, [], 0

    def on(self, k):
        return self.moved(k) if callable(self.moved) else bool(self.moved)


def cam_cfg(rtsr, case, width=48, spp=4, depth=8, seed=31):
    cam = rtsr.Camera.new(case.look[0], case.look[1], (0.0, 1.0, 0.0), 35.0, 1.5, 0.0, 10.0, 0.0, 1.0)
    cfg = rtsr.Config.new(1.5, width, spp, depth, 4, seed=seed)
    return cam, cfg, rtsr.image_height(cfg)


def seeded_rays(n, seed, lo, hi, target_y):
    """Origins on a box [lo, hi] around the scene, aimed at points inside it at a height in target_y."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(lo), np.array(hi)
    o = lo + (hi - lo) * rng.uniform(0.0, 1.0, (n, 3))
    o[:, 1] = hi[1] + rng.uniform(0.5, 3.0, n)
    side = rng.integers(0, 3, n)
    o[side == 1, 0] = lo[0] - 2.0
    o[side == 2, 2] = hi[2] + 2.0
    target = lo + (hi - lo) * rng.uniform(0.15, 0.85, (n, 3))
    target[:, 1] = rng.uniform(target_y[0], target_y[1], n)
    return o, target - o


def call_set_prims(rtsr, fn, handle, ids, n, values, *rest):
    """One raw call of an rtx_*_set_triangles / _set_spheres entry.  ids, values: None for a NULL pointer; n: None for len(ids)."""
    ia = np.ascontiguousarray(ids, dtype=np.int32) if ids is not None else None
    va = np.ascontiguousarray(values, dtype=np.float64) if values is not None else None
    return fn(handle, ia.ctypes.data_as(C.POINTER(C.c_int32)) if ia is not None else None, len(ia) if n is None else n,
              va.ctypes.data_as(C.POINTER(C.c_double)) if va is not None else None, *rest)


# ---- the host tests
def flat_arrays(flat, names, oracle_names):
    """Every array an update may or may not touch, as bytes; oracle_names: those no hook of the library's reads -- the oracle's view
    of the same FlatScene does.  (Tests that call this take the `orc` fixture, which builds the oracle.)"""
    import oracle_py
    out = {name: flat.array(name) for name in names}
    for name in oracle_names:
        out[name] = oracle_py.flat_array(flat.arrays_ptr(), name)[0]
    return out


def hit_records(orc, flat, o, d):
    out = np.zeros((len(o), 11))
    for r in range(len(o)):
        rec = orc.core_world_hit(flat.arrays_ptr(), tuple(o[r]), tuple(d[r]), 0.25, 0.001, float("inf"), rng_seed=1 + r)
        if rec is not None:
            out[r] = [1.0, rec["t"], *rec["p"], *rec["normal"], rec["u"], rec["v"], float(rec["front_face"])]
    return out


def assert_same_topology(now, first, untouched):
    n, n0 = now["nodes"].view(NODE), first["nodes"].view(NODE)
    m, m0 = now["nodes32"].view(NODE32), first["nodes32"].view(NODE32)
    assert np.array_equal(n["child"], n0["child"]) and np.array_equal(n["pad"], n0["pad"])
    assert np.array_equal(m["child"], m0["child"]) and np.array_equal(m["axis"], m0["axis"]) and np.array_equal(m["pad"], m0["pad"])
    for k in untouched:
        assert np.array_equal(now[k], first[k]), k


# ---- the GPU tests
def upload(flat, env=None):
    """flat.upload() under the given RTX_* switches (read once per upload)."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env or {})
    try:
        return flat.upload()
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def device_arrays(scene, names):
    """{name: the resident array as bytes}; "plans" stands for the launch plans an update must keep (which = 8, 9)."""
    return {k: np.array([scene.wide_levels(), scene.max_stack()], dtype=np.int32).view(np.uint8) if k == "plans" else scene.array(k) for k in names}


def assert_arrays_equal(scene, want, what):
    now = device_arrays(scene, want)
    for k in want:
        assert now[k].size == want[k].size and np.array_equal(now[k], want[k]), "%s: %s differs from the host-updated scene uploaded fresh in %d bytes" % (
            what, k, int((now[k] != want[k]).sum()) if now[k].size == want[k].size else -1)


def same_screen(a, b, what):
    bad = int((a.accum != b.accum).any(axis=2).sum())
    assert bad == 0 and np.array_equal(a.rgb8, b.rgb8), "%s: %d pixels differ from the fresh upload" % (what, bad)


def updated_pair(cache, rtsr, cases, update_of, setter, name, env=()):
    """(updated scene, fresh scene, host-updated flat, fresh flat, case): uploaded at rest and updated on the device through the
    method `setter` ("set_triangles" / "set_spheres"), and the same world built from scratch with the moved values.  Built once
    per case for the default switches (a scene under a forced kernel keeps that kernel's workspace: not kept beyond its one
    frame)."""
    if name in cache and not env:
        return cache[name]
    case, moved = cases[name](rtsr, False), cases[name](rtsr, True)
    flat, fresh_flat = case.flatten(), moved.flatten()
    scene = upload(flat, dict(env))
    ids, values = update_of(case, flat)
    getattr(scene, setter)(ids, values)
    getattr(flat, setter)(ids, values)
    pair = (scene, upload(fresh_flat, dict(env)), flat, fresh_flat, case)
    if not env:
        cache[name] = pair
    return pair
