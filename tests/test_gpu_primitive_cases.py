"""Closest-hit records of the static primitives and the Translate / RotateY chain on the device (Scene.cast_rays, f64 and
upload(f32=True)) against the independent judge of tests/primitive_cases.py, and bit for bit (NaN for NaN) against the CPU core.
The premises of the cases (lattice exactness, undecided caps, stored sines and cosines) are asserted by
tests/test_primitive_cases.py from the judge alone; here the device answers the same rays.  Every batch is at most 4096 rays.
Three 36 x 24 frames of pure-colour lights then go through every walker that can reach them, their pixel sums decoded into hit
counts per primitive and held to the judge's first hits (test_frames_through_every_walker).

Worst observed-to-bound ratios are printed per case and build (pytest -s; profiles/primitives/README.md keeps them)."""
import numpy as np
import pytest

import cast_rays_cases as cc
import primitive_cases as pc

FAMILIES = pc.FAMILIES

pytestmark = pytest.mark.gpu
_GENERAL = {}


def _general(rtsr, mode):
    if mode not in _GENERAL:
        _GENERAL[mode] = [c for c in pc.general_cases(mode) if mode in c.modes]
        for c in _GENERAL[mode]:
            c.build(rtsr)
    return _GENERAL[mode]


def _cast(case, mode, **kw):
    return case.world.scene(mode).cast_rays(case.o, case.d, None, case.t_max, t_min=case.t_min, **kw)


def _device_against_judge_and_core(orc, case, mode):
    """The CPU core answers first (a case the core cannot answer never reaches the device), then the device: its records equal
    the core's bit for bit and meet the judge.  -> the worst observed-to-bound ratio.

    A ray of the f32 face-touch class (Case.judge: the record changes when the primitives the culling ray rules out are left
    out; core/cull32.hpp, "what the replacement gives up") has two stated records.  world_hit skips a primitive only when no
    lane of the WAVE may hit it (RT_WAVE_ANY), so on the device such a ray is culled or not depending on the rays beside it in
    the batch, while the CPU core, one ray per thread, always culls a bare slot.  The device must give one of the two; which
    one each ray got is printed, and a device record that differs from the CPU core's is only admitted for this class."""
    w = case.world
    core = pc.core_records(orc, w.flat, case.o, case.d, case.t_min, case.t_max, mode)
    h = _cast(case, mode)
    rows = pc.device_records(h)
    verdicts = case.judge(mode)
    touch = np.array([bool(v.get("face_touch")) for v in verdicts])
    assert mode == "f32" or not touch.any()
    differ = ~cc.same_bits(rows, core)
    bad = np.flatnonzero(differ & ~touch)
    assert len(bad) == 0, "%s (%s): ray %d: device %r, CPU core %r" % (case.name, mode, bad[0], rows[bad[0]].tolist(), core[bad[0]].tolist())
    miss = h.ids[:, 0] == 0
    assert np.all(np.isposinf(h.t[miss])) and np.all(h.ids[miss] == [0, -1, -1, 0])
    worst = 0.0
    for r in range(case.n):
        prim = None if miss[r] else int(w.prim_of_material[h.ids[r, 1]])
        got = pc.got_of_row(rows[r], prim)
        if touch[r]:
            which = pc.check_touch_record(case, mode + ", device", r, verdicts[r], got, allow_rule=True)
            print("%s (%s), face-touch ray %d: the device gives the %s record%s" % (case.name, mode, r, which, ", the CPU core another" if differ[r] else ""))
            continue
        worst = max(worst, pc.check_record(case, mode + ", device", r, verdicts[r], got))
    return worst


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_lattice_cases_on_the_device(rtsr, orc, family, mode):
    """Every lattice ray: the device equals the exact judge in hit or miss, t, p, normal (NaN for NaN), front_face and the
    primitive, and the CPU core in every bit.  The zero direction and the zero radius are among the sphere cases."""
    rays = 0
    for case in FAMILIES[family](mode):
        if mode not in case.modes:
            continue
        case.build(rtsr)
        _device_against_judge_and_core(orc, case, mode)
        rays += case.n
    print("%s (%s): %d rays on the device equal the exact judge and the CPU core" % (family, mode, rays))
    assert rays > 0


@pytest.mark.parametrize("mode", pc.MODES)
def test_zero_area_triangle_on_the_device(rtsr, orc, mode):
    """A triangle moved onto a line by set_triangles answers t = NaN with a NaN normal when it is reached."""
    case = pc.Case("triangle_zero_area", pc.lst(pc.tri(*pc.T0)), [((0.0, 2.0, 2.0), (0.5, -1.0, -1.0)), ((5.0, -1.0, 4.0), (-1.0, 0.5, -2.0))])
    w = case.build(rtsr)
    line = [(0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (2.0, 0.0, 0.0)]
    w.flat.set_triangles(w.flat.triangle_ids(w.b, w.handle), np.array([line], dtype=np.float64).reshape(1, 9))
    case.desc.children[0].a.update(v0=line[0], v1=line[1], v2=line[2])
    assert all(v["rec"] is not None and np.isnan(v["rec"]["t"]) for v in case.judge(mode))
    _device_against_judge_and_core(orc, case, mode)


@pytest.mark.parametrize("mode", pc.MODES)
def test_general_cases_on_the_device(rtsr, orc, mode):
    """Every decided ray: hit, front_face and primitive equal the judge's; t, p and normal lie within the derived bound; and
    every ray, decided or not, equals the CPU core bit for bit."""
    for case in _general(rtsr, mode):
        worst = _device_against_judge_and_core(orc, case, mode)
        print("%s (%s): worst observed / bound on the device %.3g" % (case.name, mode, worst))


@pytest.mark.parametrize("mode", pc.MODES)
def test_containers_do_not_change_a_bit_on_the_device(rtsr, orc, mode):
    """Top-level entries, a group, a host-built BVH at max_leaf 1 and at the default, a chain (Translate by 0), instance-tree
    members with and without a chain, and a rectangle as a prism's face: identical bits of t, p, normal and front_face (under a
    chain front_face is the wrapper's: primitive_cases.container_columns), each equal to the CPU core's."""
    rays = pc.container_rays()
    ref = None
    for name, (desc, max_leaf) in pc.container_worlds().items():
        case = pc.Case("container_" + name, desc, rays, kind="general", max_leaf=max_leaf)
        w = case.build(rtsr)
        core = pc.core_records(orc, w.flat, case.o, case.d, case.t_min, case.t_max, mode)
        rec = pc.device_records(_cast(case, mode))
        assert cc.same_bits(rec, core).all(), (name, mode)
        if ref is None:
            ref = rec
            assert 4 * int(rec[:, 0].sum()) >= case.n
            continue
        cols = pc.container_columns(name, rec, ref)
        bad = np.flatnonzero(~cc.same_bits(rec[:, :cols], ref[:, :cols]))
        assert len(bad) == 0, "%s (%s): ray %d: %r, top-level %r" % (name, mode, bad[0], rec[bad[0]].tolist(), ref[bad[0]].tolist())
    rays = pc.prism_face_rays()
    got = {}
    for name, desc in pc.PRISM_FACE_WORLDS.items():
        case = pc.Case("face_" + name, desc, rays, kind="general")
        case.build(rtsr)
        got[name] = pc.device_records(_cast(case, mode))
    assert got["rect"][:, 0].all() and cc.same_bits(got["rect"], got["prism"]).all()


def test_a_chain_case_through_torch_tensors(rtsr):
    """The four-op chain case with its rays and its records in torch tensors on the device: the same bytes as through numpy."""
    import torch
    case = [c for c in _general(rtsr, "f64") if c.name == "chain_TRTR"][0]
    ref = _cast(case, "f64")
    dev = torch.device("cuda", 0)
    o, d, t_max = (torch.from_numpy(a).to(dev) for a in (case.o, case.d, case.t_max))
    h = case.world.scene("f64").cast_rays(o, d, None, t_max, t_min=case.t_min)
    torch.cuda.synchronize()
    assert all(getattr(h, c).is_cuda for c in h.columns)
    assert all(getattr(h, c).cpu().numpy().tobytes() == getattr(ref, c).tobytes() for c in rtsr.RAY_COLUMNS)


# ---- frames through every walker ------------------------------------------------------------------------------------------------
# (environment of the upload, the kernel it must take).  k_trace_lds is compiled for Lambertian, Metal and Dielectric spheres
# only (P_SPHERES holds no light), so the sphere BVH of lights is k_trace_vote's by default and k_trace_lds renders its matte
# twin, whose pixels decode into the total hit count (test_primitive_cases.test_frames_on_the_cpu).
FRAME_KERNELS = {
    "sphere_bvh": (({}, "k_trace_vote"), ({"RTX_TRACE_KERNEL": "vote"}, "k_trace_vote"), ({"RTX_TRACE_KERNEL": "wavefront"}, "k_wf_trace"),
                   ({"RTX_TRACE_KERNEL": "world"}, "k_trace_world"), ({"RTX_TRACE_KERNEL": "simple"}, "k_trace_simple")),
    "mesh_and_rects": (({"RTX_WIDE": "0"}, "k_trace_vote"), ({"RTX_WIDE": "1"}, "k_trace_vote"), ({"RTX_TRACE_KERNEL": "wavefront"}, "k_wf_trace"),
                       ({"RTX_TRACE_KERNEL": "world", "RTX_WIDE": "0"}, "k_trace_world"), ({"RTX_TRACE_KERNEL": "world", "RTX_WIDE": "1"}, "k_trace_world"),
                       ({"RTX_TRACE_KERNEL": "simple"}, "k_trace_simple")),
    "list_world": (({}, "k_trace_world"), ({"RTX_TRACE_KERNEL": "simple"}, "k_trace_simple")),
}


def _render_under(rtsr, monkeypatch, flat, mode, env, cam, cfg):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene = flat.upload(f32=(mode == "f32"))
    screen = scene.render(cam, cfg, want_stats=True)
    for k in env:
        monkeypatch.delenv(k)
    return rtsr.trace_kernel_name(screen.stats.trace_kernel), np.asarray(screen.accum, dtype=np.float64)


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("name", list(FRAME_KERNELS))
def test_frames_through_every_walker(rtsr, monkeypatch, name, mode):
    """A 36 x 24 frame at 4 spp of lights of pure colours: the pixel sums of every kernel that can reach the scene decode into
    the judge's hit counts per primitive (a pixel is allowed its number of undecided samples).  The expected counts come from
    features_cases.primary_ray on rtsr.device_stream and the judge's first hit."""
    w = pc.World(rtsr, pc.frame_scenes()[name], emit="light")
    want, und = pc.expected_counts(rtsr, w, mode, rtsr.device_stream)
    assert und.sum() <= pc.FRAME_CAP[mode] * pc.FRAME_W * pc.FRAME_H * pc.FRAME_SPP
    cam, cfg = pc.frame_cam_cfg(rtsr)
    for env, kernel in FRAME_KERNELS[name]:
        got_kernel, accum = _render_under(rtsr, monkeypatch, w.flat, mode, env, cam, cfg)
        assert got_kernel == kernel, (name, mode, env, got_kernel)
        pc.check_frame_counts("%s (%s) %s %r" % (name, mode, kernel, env), pc.decode_counts(accum, w.n_prims), want, und)
    if name == "sphere_bvh":
        matte = pc.World(rtsr, pc.frame_scenes()[name], emit="matte")
        cam, cfg = pc.frame_cam_cfg(rtsr, max_depth=1, background=(1.0, 1.0, 1.0))
        got_kernel, accum = _render_under(rtsr, monkeypatch, matte.flat, mode, {}, cam, cfg)
        assert got_kernel == "k_trace_lds", (mode, got_kernel)
        total = pc.FRAME_SPP - accum
        assert np.array_equal(total[:, :, 0], total[:, :, 1]) and np.array_equal(total[:, :, 0], total[:, :, 2])
        pc.check_frame_counts("sphere_bvh (%s) k_trace_lds" % mode, total[:, :, :1].astype(np.int64), want.sum(axis=2, keepdims=True), und)
