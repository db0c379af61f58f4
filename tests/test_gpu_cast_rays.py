"""Ray queries on the device (Scene.cast_rays, rtx_scene_cast_rays*): the device answers the ray the CPU core answers.

Every comparison is by bit pattern with NaN equal to NaN (cast_rays_cases.same_bits): the oracle is called once per ray
(orc.core_world_hit / core32_world_hit), its answers are computed once per scene and shared by the tests of this file.
Scenes and rays: tests/cast_rays_cases.py (at most 2000 rays per scene)."""
import ctypes as C

import numpy as np
import pytest

import cast_rays_cases as cc
from instance_scenes import member_zoo

pytestmark = pytest.mark.gpu
SEED = 1
_CASES = {}


def _case(rtsr, orc, name):
    """The case with its rays, its resident scene and the oracle's records under stream_step 0 (built once)."""
    if name not in _CASES:
        case = (cc.F64_CASES.get(name) or cc.F32_CASES[name])(rtsr).build_rays(orc)
        case.scene = case.flat.upload(f32=case.f32)
        case.ref = {0: cc.records(orc, case, case.o, case.d, case.time, case.t_max, SEED, 0)}
        _CASES[name] = case
    return _CASES[name]


def _cast(case, stream_step=0, **kw):
    return case.scene.cast_rays(case.o, case.d, case.time, case.t_max, t_min=cc.T_MIN, seed=SEED, stream_step=stream_step, **kw)


def _assert_equal_records(name, got, ref):
    bad = np.flatnonzero(~cc.same_bits(got, ref))
    print("%s: %d rays, %d hit, %d differ from the oracle" % (name, len(ref), int(ref[:, 0].sum()), len(bad)))
    assert len(bad) == 0, "%s: ray %d: device %r, oracle %r" % (name, bad[0], got[bad[0]].tolist(), ref[bad[0]].tolist())


# ---- 1. bit-exact against the CPU core, f64
@pytest.mark.parametrize("name", list(cc.F64_CASES))
def test_f64_rays_equal_the_cpu_core(rtsr, orc, name):
    """Hit or miss, t, p, normal, u, v and front_face of every ray equal core_world_hit's, bit for bit (stream_step 0: every
    ray on the oracle's stream).  The input condition comes from the oracle alone: >= 25 % hits, >= 10 % misses."""
    case = _case(rtsr, orc, name)
    cc.check_mix(name, case.ref[0])
    h = _cast(case)
    _assert_equal_records(name, cc.hits_as_records(h), case.ref[0])
    miss = h.ids[:, 0] == 0
    assert np.all(np.isposinf(h.t[miss])) and np.all(h.ids[miss] == [0, -1, -1, 0])
    assert not h.p[miss].any() and not h.normal[miss].any() and not h.uv[miss].any()
    hit = ~miss
    info = case.flat.info()
    assert np.all((h.ids[hit, 1] >= 0) & (h.ids[hit, 1] < info["n_materials"]))
    assert np.all((h.ids[hit, 2] >= 0) & (h.ids[hit, 2] < info["n_top_level"]))


def test_gravity_rays_at_and_past_the_time_limit(rtsr, orc):
    """Scene 8 again.  A ray whose time lies past the stored trajectory by more than 10 s is not cast (get_center's fallback
    loop is unbounded there) and reports a miss; a ray exactly AT the limit is cast and equals the oracle.  The limit is
    table_len * 0.001 + 10 with the table of GravitySphere::new (time0 = 0 for every sphere of this scene), rebuilt here."""
    case = _case(rtsr, orc, "gravity_t0.37")
    t, table_len = 0.0, 1
    while t < 100.0:
        t += 0.001
        table_len += 1
    limit = table_len * 0.001 + 10.0
    pick = np.flatnonzero(case.ref[0][:, 0] == 1.0)[:4]
    o = np.ascontiguousarray(np.concatenate([case.o[pick], case.o[pick]]))
    d = np.ascontiguousarray(np.concatenate([case.d[pick], case.d[pick]]))
    time = np.concatenate([np.full(4, limit), np.full(4, np.nextafter(limit, np.inf))])
    h = case.scene.cast_rays(o, d, time, t_min=cc.T_MIN, seed=SEED)
    ref = cc.records(orc, case, o[:4], d[:4], time[:4], np.full(4, np.inf), SEED, 0)
    print("gravity at the limit %.17g: %d of 4 rays hit" % (limit, int(ref[:, 0].sum())))
    assert ref[:, 0].sum() >= 1
    inside = cc.hits_as_records(h)[:4]
    _assert_equal_records("gravity at the limit", inside, ref)
    assert np.all(h.ids[4:] == [0, -1, -1, 0]) and np.all(np.isposinf(h.t[4:]))
    assert not h.p[4:].any() and not h.normal[4:].any() and not h.uv[4:].any()


# ---- 2. per-ray streams
@pytest.mark.parametrize("name", cc.MEDIUM_CASES)
def test_per_ray_streams(rtsr, orc, name):
    """stream_step 1: ray r draws from rng_for_sample(seed + r, 0, 0), as the oracle called with rng_seed = seed + r; and the
    rule reaches the medium's draw: some ray answers differently under the two rules."""
    case = _case(rtsr, orc, name)
    if 1 not in case.ref:
        case.ref[1] = cc.records(orc, case, case.o, case.d, case.time, case.t_max, SEED, 1)
    got = cc.hits_as_records(_cast(case, stream_step=1))
    _assert_equal_records(name + " (stream per ray)", got, case.ref[1])
    differ = int((~cc.same_bits(case.ref[0], case.ref[1])).sum())
    print("%s: %d rays answer differently under stream_step 0 and 1" % (name, differ))
    assert differ >= 1
    assert int((~cc.same_bits(got, cc.hits_as_records(_cast(case)))).sum()) == differ


# ---- 3. directed rays on the device
def _directed_rays(orc, flat):
    """The directed set of tests/test_instance_tree.py on the zoo's own coordinates (rebuilt here): zero direction components,
    rays in a rectangle's plane, along a prism's face, edge and top, from inside a member and from its surface, the
    negative-radius sphere from inside, between the shells and outside, t_max exactly on a member, exact ties between the
    coincident members, and rays over the rotated members' footprints.  The fixed coordinates of the axis-parallel rays stand
    off every plane (+ 0.0137 ...) except where a plane is the point of the ray."""
    inf = float("inf")
    rays = []
    add = lambda o, d, t_min=0.001, t_max=inf: rays.append((o, d, t_min, t_max))
    for x, z in ((-4.0, 1.0), (1.0, 1.2), (3.4, 0.9), (2.0, -2.2), (-2.4, -2.8), (5.5, -2.6), (-4.2, -4.0), (4.2, -4.0)):
        add((x + 0.0137, 6.0, z + 0.0071), (0.0, -1.0, 0.0))
        add((x + 0.0137, 6.0, z - 1.5), (0.0, -1.0, 0.25))
        add((x - 2.0, 0.3137, z + 0.0071), (1.0, 0.0, 0.0))
    add((-4.0, 0.6137, -0.5), (1.0, 0.013, 0.0))      # in the plane of the XyRect at z = -0.5 (t = NaN) ...
    add((-2.5, 0.2137, -0.5), (0.0, 1.0, 0.0))
    add((-2.0137, 0.4, 0.2), (0.003, 0.0, 1.0))       # ... of the XzRect at y = 0.4 ...
    add((-1.2, 3.0, 0.5137), (0.0, -1.0, 0.01))       # ... of the YzRect at x = -1.2
    add((3.0, 2.0, 0.9137), (0.0, -1.0, 0.0))         # along a face of the bare prism, along its edge, along its top
    add((3.0, 2.0, 0.5), (0.0, -1.0, 0.0))
    add((2.0, 0.9, 0.9137), (1.0, 0.0, 0.0))
    add((3.8, 0.9, -2.0), (0.0, 0.0, 1.0))
    add((-4.0, 0.6, 1.0), (0.3, 0.2, 1.0))            # from inside a member, from its surface (outward and inward)
    add((-4.0, 1.2, 1.0), (0.01, 1.0, 0.02))
    add((-4.0, 1.2, 1.0), (0.01, -1.0, 0.02))
    add((3.4, 0.45, 0.9), (1.0, 0.3, 0.2))
    add((2.0, 0.4, -2.2), (0.2, 0.1, 1.0))
    for o, d in (((1.0, 0.7, 1.2), (0.3, 1.0, 0.2)), ((1.0, 1.35, 1.2), (0.01, -1.0, 0.0)), ((1.0, 1.35, 1.2), (1.0, 0.02, 0.0)),
                 ((1.0137, 5.0, 1.2071), (0.0, -1.0, 0.0)), ((-3.0, 0.7137, 1.2071), (1.0, 0.0, 0.0)), ((1.0, 0.7, 6.0), (0.05, 0.02, -1.0)),
                 ((1.55, 3.0, 1.2071), (0.0, -1.0, 0.0)), ((1.0, 0.7, 1.2), (-1.0, -0.2, 0.4))):
        add(o, d)                                     # the negative-radius sphere
    for x in (-4.3137, -4.2071, -4.1037, 4.1137, 4.2071, 4.3037):
        add((x, 5.0, -4.0071), (0.0, -1.0, 0.0))      # exact ties: the coincident top faces (y = 0.8) of the tied members
        add((x, 5.0, -4.3), (0.001, -1.0, 0.05))
    for o, d in (((-4.0137, 6.0, 1.0071), (0.0, -1.0, 0.0)), ((2.3, 5.0, 1.2), (0.01, -1.0, 0.02)), ((3.4137, 4.0, 0.9071), (0.0, -1.0, 0.0)),
                 ((2.0, 3.0, 2.0), (0.0, -0.6, -1.0))):
        free = orc.core_world_hit(flat.arrays_ptr(), o, d)
        assert free is not None and free["t"] == free["t"]
        add(o, d, 0.001, free["t"])                   # t_max exactly on a member (the reference accepts t == t_max)
    for cx, cz in ((-2.4, -2.8), (-1.2, -2.8), (5.5, -2.6), (2.0, -2.2), (4.4, -0.6), (-5.2, 1.9)):
        for i in range(9):
            for j in range(9):
                x, z = cx - 1.0 + 0.25 * i + 0.0037, cz - 1.0 + 0.25 * j + 0.0013
                add((x, 3.0, z), (0.0, -1.0, 0.0) if (i + j) % 2 else (0.02, -1.0, -0.01))
    return rays


def test_directed_rays_instanced_equals_hoisted_equals_oracle(rtsr, orc):
    """The instanced and the hoisted spelling of the zoo ("middle") give the same bits on the device, both equal the oracle's
    answer for their own flat scene, and the slot the instanced spelling reports is the hoisted spelling's (a member's slot
    is its position in the world list either way).  t = NaN occurs (rays in a rectangle's plane)."""
    (bh, wh), (bi, wi) = member_zoo(rtsr, "hoisted"), member_zoo(rtsr, "instanced")
    fh, fi = bh.flatten(wh), bi.flatten(wi)
    rays = _directed_rays(orc, fh)
    o = np.array([r[0] for r in rays], dtype=np.float64)
    d = np.array([r[1] for r in rays], dtype=np.float64)
    t_max = np.array([r[3] for r in rays], dtype=np.float64)
    got = {}
    for key, flat in (("hoisted", fh), ("instanced", fi)):
        h = flat.upload().cast_rays(o, d, None, t_max, t_min=0.001, seed=SEED)
        ref = np.zeros((len(rays), 11))
        for r, (ro, rd, t_min, tm) in enumerate(rays):
            rec = orc.core_world_hit(flat.arrays_ptr(), ro, rd, t_min=t_min, t_max=tm, rng_seed=SEED)
            if rec is not None:
                ref[r] = [1.0, rec["t"], *rec["p"], *rec["normal"], rec["u"], rec["v"], float(rec["front_face"])]
        _assert_equal_records("directed, " + key, cc.hits_as_records(h), ref)
        got[key] = h
    hits = int((got["hoisted"].ids[:, 0] == 1).sum())
    print("directed: %d rays, %d hit, %d with NaN t" % (len(rays), hits, int(np.isnan(got["hoisted"].t).sum())))
    assert 4 * hits >= len(rays) and np.isnan(got["hoisted"].t).any()
    assert cc.same_bits(cc.hits_as_records(got["instanced"]), cc.hits_as_records(got["hoisted"])).all()
    assert np.array_equal(got["instanced"].ids, got["hoisted"].ids)  # hit flag, material, SLOT and front_face
    # the eight vertical rays of the first loop stand over eight different members (none under the lamp) and the footprint rays
    # reach the ground: at least nine slots answer
    assert len(set(got["hoisted"].ids[got["hoisted"].ids[:, 0] == 1, 2].tolist())) >= 9


# ---- 4. slots and materials
def _slot_world(rtsr):
    b = rtsr.Builder(1)
    shared = b.lambertian((0.5, 0.5, 0.5))
    mats = [shared, b.lambertian((0.1, 0.2, 0.3)), shared, b.metal((0.8, 0.8, 0.8), 0.1), b.dielectric(1.5),
            b.lambertian((0.3, 0.2, 0.1)), b.metal((0.7, 0.6, 0.5), 0.0), b.lambertian((0.9, 0.9, 0.9))]
    centres = [(3.0 * k, 0.0, 0.0) for k in range(8)]
    objs = [b.sphere(c, 1.0, m) for c, m in zip(centres, mats)]
    objs[3] = b.translate((0.0, 0.0, 0.0), objs[3])
    pair_mats = [b.lambertian((0.2, 0.9, 0.2)), b.lambertian((0.9, 0.2, 0.2))]
    pair = [(24.0, 0.0, 0.0), (27.0, 0.0, 0.0)]
    objs.append(b.bvh_from_list(b.hittable_list([b.sphere(c, 1.0, m) for c, m in zip(pair, pair_mats)]), 0.0, 1.0))
    return b, b.hittable_list(objs), centres + pair


def test_slots_and_materials(rtsr):
    b, world, centres = _slot_world(rtsr)
    flat = b.flatten(world)
    kinds = flat.top_level_kinds()
    assert len(kinds) == 9 and kinds[3] == 3 and kinds[8] == 2 and all(k == 0 for i, k in enumerate(kinds) if i not in (3, 8))
    c = np.array(centres, dtype=np.float64)
    o = np.ascontiguousarray(np.concatenate([c + [0.0137, 5.0, 0.0071], [[100.0, 5.0, 0.0]]]))  # the last ray passes everything
    d = np.ascontiguousarray(np.tile([0.0, -1.0, 0.0], (len(o), 1)))
    h = flat.upload().cast_rays(o, d)
    ids = h.ids
    assert ids[:10, 0].tolist() == [1] * 10 and ids[:10, 3].tolist() == [1] * 10
    assert ids[:10, 2].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 8]  # each object's index in the list; both spheres of the BvhNode
    m = ids[:10, 1].tolist()
    assert all(0 <= x < flat.info()["n_materials"] for x in m)
    same = {(i, j) for i in range(10) for j in range(i + 1, 10) if m[i] == m[j]}
    assert same == {(0, 2)}, m  # equal material indices exactly where the handle is shared
    assert ids[10].tolist() == [0, -1, -1, 0] and np.isposinf(h.t[10])
    assert not h.p[10].any() and not h.normal[10].any() and not h.uv[10].any()
    assert np.all(np.abs(h.t[:10] - (5.0 - np.sqrt(1.0 - 0.0137 ** 2 - 0.0071 ** 2))) < 1e-12)


# ---- 5. batch shapes
def _big_batch(rtsr):
    """A cheap scene and one full pass of the grid plus one ray: the launcher's grid is 8 blocks of 256 threads per CU, so ray
    8 * 256 * CUs is the first one a thread takes in its second trip; the host entry's slices of 262144 rays are crossed too."""
    import torch
    b, world, centres = _slot_world(rtsr)
    n = 8 * 256 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    assert n > 262144
    o, d = cc.sphere_rays(n, 11, (-2.0, -2.0, -2.0), (29.0, 2.0, 2.0), 0.8)
    return b.flatten(world).upload(), o, d, n


def _columns(h):
    return [getattr(h, c) for c in h.columns]


def _equal_hits(a, b):
    return a.columns == b.columns and all(x.tobytes() == y.tobytes() for x, y in zip(_columns(a), _columns(b)))


def test_batch_sizes_and_columns(rtsr):
    scene, o, d, n = _big_batch(rtsr)
    big = scene.cast_rays(o, d)
    assert 4 * int(big.hit.sum()) >= n and 10 * int((~big.hit).sum()) >= n
    assert _equal_hits(big, scene.cast_rays(o, d))  # two calls give the same bits
    for k in (1, 63, 64, 65, 257):
        part = scene.cast_rays(np.ascontiguousarray(o[:k]), np.ascontiguousarray(d[:k]))
        assert all(x.tobytes() == y[:k].tobytes() for x, y in zip(_columns(part), _columns(big))), k
    for want in (("t",), ("ids",), ("uv", "p")):
        some = scene.cast_rays(o, d, want=want)
        assert some.columns == want and all(getattr(some, c).tobytes() == getattr(big, c).tobytes() for c in want)
        assert all(getattr(some, c) is None for c in rtsr.RAY_COLUMNS if c not in want)
    # n = 0: RTX_OK through both entries, nothing launched, empty columns
    empty = scene.cast_rays(np.zeros((0, 3)), np.zeros((0, 3)))
    assert empty.n == 0 and empty.t.shape == (0,) and empty.ids.shape == (0, 4)
    # an all-NULL RtxRayHits is a legal timing run
    batch = rtsr.RtxRayBatch()
    rtsr.lib.rtx_ray_batch_defaults(C.byref(batch))
    batch.n, batch.origin, batch.direction = 1000, o.ctypes.data, d.ctypes.data
    assert rtsr.lib.rtx_scene_cast_rays(scene.ptr, C.byref(batch), C.byref(rtsr.RtxRayHits())) == rtsr.RTX_OK


@pytest.mark.parametrize("stream_step", [0, 1])
def test_a_split_batch_equals_the_whole(rtsr, orc, stream_step):
    """Three calls whose seed is advanced by first_ray * stream_step equal one call, on a scene whose medium draws."""
    case = _case(rtsr, orc, "cornell_smoke")
    whole = _cast(case, stream_step=stream_step)
    cuts = [0, 517, 1300, case.n]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        cut = lambda a: np.ascontiguousarray(a[lo:hi])
        part = case.scene.cast_rays(cut(case.o), cut(case.d), cut(case.time), cut(case.t_max), t_min=cc.T_MIN,
                                    seed=SEED + lo * stream_step, stream_step=stream_step)
        assert all(x.tobytes() == y[lo:hi].tobytes() for x, y in zip(_columns(part), _columns(whole))), (lo, hi)


# ---- 6. device pointers
def test_torch_tensors_on_a_side_stream(rtsr, orc):
    import torch
    case = _case(rtsr, orc, "cornell_smoke")
    ref = _cast(case, stream_step=1)
    dev = torch.device("cuda", 0)
    host = (case.o, case.d, case.time, case.t_max)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        tens = [torch.from_numpy(a).to(dev) for a in host]
        keep = [t.clone() for t in tens]
        h = case.scene.cast_rays(*tens, t_min=cc.T_MIN, seed=SEED, stream_step=1)
        few = case.scene.cast_rays(tens[0], tens[1], want=("ids",))
    side.synchronize()
    assert all(getattr(h, c).is_cuda and getattr(h, c).device == dev for c in h.columns)
    assert h.t.dtype == torch.float64 and h.ids.dtype == torch.int32 and tuple(h.ids.shape) == (case.n, 4)
    assert all(getattr(h, c).cpu().numpy().tobytes() == getattr(ref, c).tobytes() for c in rtsr.RAY_COLUMNS)
    assert all(torch.equal(a, b) for a, b in zip(tens, keep))  # the inputs are unchanged
    assert few.columns == ("ids",) and few.t is None and tuple(few.ids.shape) == (case.n, 4)
    # the single-column cast on the device route: time 0, unbounded, every ray on the stream of SEED
    few_ref = case.scene.cast_rays(case.o, case.d, want=("ids",))
    assert few.ids.cpu().numpy().tobytes() == few_ref.ids.tobytes()
    for name, kw in (("origins", dict(origins=tens[0].float(), directions=tens[1])),
                     ("directions", dict(origins=tens[0], directions=tens[1].t().contiguous().t())),
                     ("times", dict(origins=tens[0], directions=tens[1], times=tens[2][:-1])),
                     ("t_max", dict(origins=tens[0], directions=tens[1], t_max=tens[3].cpu()))):
        with pytest.raises(ValueError) as e:
            case.scene.cast_rays(**kw)
        assert str(e.value).startswith(name + ":"), str(e.value)


# ---- 7. f32 scenes
@pytest.mark.parametrize("name", list(cc.F32_CASES))
def test_f32_rays_equal_the_float_core(rtsr, orc, name):
    """An f32 scene narrows the ray and widens the record: equal to core32_world_hit bit for bit.  Book-1 canonical and the
    zoo's tier-A spelling (solid colours, no medium) reach no platform function.  The medium scenes do reach logf in their
    distance draw: they are not in this set, and nothing here compares them more loosely."""
    case = _case(rtsr, orc, name)
    assert case.scene.is_f32
    cc.check_mix(name, case.ref[0])
    _assert_equal_records(name, cc.hits_as_records(_cast(case)), case.ref[0])
