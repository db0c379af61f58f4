"""The device on the cases of tests/material_cases.py (proven on the CPU in tests/test_material_cases.py).

Probes: every probe ray of every case through Scene.trace_rays, bit for bit against the f64 host judge (the first JUDGED
replicas of the batch: the same streams), and the device's own counts over all 2^18 samples per point against the closed forms
(the same bits; the assertion names what broke).
Casts: Scene.cast_rays with stream_step = 1 against core_world_hit records, bit for bit, every t_min / t_max variant.
Frames, 48 x 32 at 8 spp and depth 50, RtxRenderStats.trace_kernel asserted each time: glass_balls through k_trace_lds, vote,
wavefront, world and simple; every list world through k_trace_world and k_trace_simple against O2 and O1; every list world
again beside a gravity sphere (k_trace_world<P_ALL>), a two-member instance tree (<P_INST>) and a 200-sphere BVH on the binary and
the 4-wide tree.  Which k_trace_world instantiation a list world reaches follows from launch_world's rule on the feature word
(render.hip), restated in _preset below and asserted per case:
  P_BOOK2             media_sphere, two_media, every pair, surface_in_front over a ball (sphere media only), and the panes
                      (glass_pane, metal_mirror, metal_fuzz: no triangle, no group, no checker, no general medium)
  P_NO_SPHERE_MEDIA   casts, isotropic_slab and surface_in_front over a slab (a rect_prism is a group; general media only), media_general
                      (general media, a BVH of triangles)
  P_ANY               media_sphere with a slab beside it (slab=True: both kinds of medium)
Mixed waves: the frames of the pair worlds are taken from a camera ON the ball's boundary, so the lanes of one wave split between
rays inside, outside, box-culled and paired; they must equal O1.
light_sampling=True on the media worlds that hold a light: k_trace_nee against its host checker.
The f32 scene: glass and metal reach only + - * / sqrt and are held bit for bit to the float judge; media reach logf and are
held to the closed forms under the same cap, every cast's t to the float judge's within LOGF_T_BOUND.

Cases that cannot reach a kernel: k_trace_lds, k_trace_vote and k_wf_trace take worlds of ONE BVH of spheres, so only
glass_balls is theirs and no medium reaches them; the 4-wide tree exists only beside a BVH; a world with an instance tree
keeps the binary tree."""
import numpy as np
import pytest

import light_cases as lc
import material_cases as mc
import trace_rays_cases as tc

pytestmark = pytest.mark.gpu

JUDGED = 4   # replicas of every point held bit for bit to the host judge (2^14 samples per point)
WORLDS = mc.LIST_WORLDS + [("media_sphere", {"slab": True})]
_scenes = {}
F_TRIANGLE, F_GROUP, F_CHECKER, F_GRAVITY, F_INSTANCE = 1 << 3, 1 << 5, 1 << 14, 1 << 17, 1 << 20
WD_PAIR = 32


@pytest.fixture(scope="module")
def chk(orc, tmp_path_factory):
    return tc.checkers(tmp_path_factory)


def _scene(case, f32=False):
    if (id(case), f32) not in _scenes:
        _scenes[(id(case), f32)] = case.flat.upload(f32=f32)
    return _scenes[(id(case), f32)]


def _preset(orc, case):
    """launch_world's choice (render.hip) from the feature word."""
    f = orc.flat_features(case.flat.arrays_ptr())
    if f & F_INSTANCE:
        return "P_INST"
    if f & F_GRAVITY:
        return "P_ALL"
    if not f & (F_TRIANGLE | F_GROUP | F_CHECKER | mc.F_MEDIUM_GENERAL):
        return "P_BOOK2"
    return "P_NO_SPHERE_MEDIA" if not f & mc.F_MEDIUM_SPHERE else "P_ANY"


def _default_kernel(orc, case):
    """choose_trace_kernel's choice (render.hip) for a world of several slots when no kernel is asked for: k_trace_vote takes a
    world list that is ONE BVH beside plain primitives only (plan_vote: no group, wrapper, medium or instance tree among the
    slots) whose features lie within P_MESH -- spheres, rectangles, triangles, groups below the BVH, Lambertian, Metal,
    Dielectric, lights, no texture but solid colours; every other world is k_trace_world's."""
    f = orc.flat_features(case.flat.arrays_ptr())
    kinds = case.flat.top_level_kinds()
    p_mesh = (1 << 0) | (1 << 2) | (1 << 3) | (1 << 4) | (1 << 5) | (1 << 6) | (1 << 9) | (1 << 10) | (1 << 11) | (1 << 12)
    one_bvh = kinds.count(2) == 1 and all(k in (0, 2) for k in kinds)   # ENTRY_BVH = 2, ENTRY_PRIM = 0
    return "k_trace_vote" if one_bvh and not f & ~p_mesh else "k_trace_world"


def _device_sums(scene, case, replicas, spp):
    o, d, t = case.rays(replicas)
    return scene.trace_rays(o, d, t, spp=spp, max_depth=case.max_depth, background=case.background, seed=mc.SEED).sum


def _kernel(rtsr, screen):
    return rtsr.trace_kernel_name(screen.stats.trace_kernel)


def _render_under(monkeypatch, case, env, **kw):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene = case.flat.upload()
    screen = scene.render(case.cam, case.cfg, want_stats=True, **kw)
    for k in env:
        monkeypatch.delenv(k)
    return scene, screen


def _o2(rtsr, orc, case):
    if not hasattr(case, "o2"):
        case.o2 = orc.o2_render(case.flat.arrays_ptr(), case.cam, case.cfg, rtsr.image_height(case.cfg), threads=16)
    return case.o2


def _diff(a, b):
    return "%d pixels differ" % int((~((a == b) | (np.isnan(a) & np.isnan(b)))).any(axis=2).sum())


# ---- probes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", WORLDS + [("glass_balls", {}), ("metal_mirror", {"edited": True}), ("metal_fuzz", {"edited": True})], ids=mc.case_id)
def test_every_probe_equals_the_host_judge(rtsr, chk, name, variant):
    case = mc.build(rtsr, name, **variant)
    want = mc.host_sums(chk, case, replicas=JUDGED)
    got = _device_sums(_scene(case), case, JUDGED, mc.SPP)
    bad = np.nonzero(~tc.same_bits(got, want))[0]
    assert len(bad) == 0, [(case.points[k % len(case.points)].tag, got[k], want[k]) for k in bad[:5]]


@pytest.mark.parametrize("name,variant", mc.STATISTICAL, ids=mc.case_id)
def test_device_counts_against_the_closed_forms(rtsr, name, variant):
    """tests/test_material_cases.py's conditions on the device's own sums at the full sample count."""
    case = mc.build(rtsr, name, **variant)
    counts, whole = mc.counts_of(case, _device_sums(_scene(case), case, case.replicas, mc.SPP))
    assert whole, "a sum is not an integer count times the unit colour"
    lines, failed = mc.check_counts(case, counts)
    print("\n[material cases, device] " + "\n[material cases, device] ".join(lines or ["%s: all exact counts" % case.name]))
    assert not failed, failed
    assert counts[:, 1].sum() == 0


def test_metal_edit_on_a_resident_scene(rtsr, chk):
    """set_shading's ("metal", ...) edit on the RESIDENT scene: fuzz 1.7 and 1e300 arrive as 1, -0.5 as it is; the sums are those
    of the scene built with the values."""
    plain = mc.build(rtsr, "metal_fuzz")
    b = mc._metal_fuzz(rtsr)   # a fresh copy to edit on the device
    scene = b.flat.upload()
    scene.set_shading([("metal", m, (0.2, 0.2, 0.2), 0.125) for m in b.extra["mats"]])
    assert not np.array_equal(_device_sums(scene, b, 1, 64), _device_sums(_scene(plain), plain, 1, 64))
    scene.set_shading([("metal", m, mc.METAL_ALBEDO, f if np.isfinite(f) else 1e300) for m, (_, f) in zip(b.extra["mats"], mc.FUZZ_POINTS)])
    assert np.array_equal(mc.bits(_device_sums(scene, b, JUDGED, 256)), mc.bits(_device_sums(_scene(plain), plain, JUDGED, 256)))


# ---- casts ---------------------------------------------------------------------------------------------------------------
def _cast(scene, cs):
    o, d = cs.rays()
    h = scene.cast_rays(o, d, None, None, t_min=cs.t_min, t_max_all=cs.t_max, seed=mc.SEED + cs.first, stream_step=1, want=("t", "ids"))
    return h.ids[:, 0] == 1, h.t


def test_casts_equal_the_core_records(rtsr, orc):
    case = mc.build(rtsr, "casts")
    scene = _scene(case)
    records = mc.cast_records(orc, case)
    for cs in case.extra["sets"]:
        hit, t = _cast(scene, cs)
        want_hit, want_t = records[cs.tag]
        assert np.array_equal(hit, want_hit), (cs.tag, int((hit != want_hit).sum()))
        assert np.array_equal(mc.bits(np.where(hit, t, np.inf)), mc.bits(want_t)), cs.tag
        if cs.verdict == "never":
            assert not hit.any(), cs.tag
        if cs.verdict == "at_t1":
            assert hit.all() and (t == 2.0).all(), cs.tag
        if cs.share is not None:
            z = abs(hit.mean() - cs.share) / np.sqrt(cs.share * (1.0 - cs.share) / cs.n)
            assert z <= mc.Z_CAP and mc.rel_se(cs.share, cs.n) <= mc.REL_SE_CAP, (cs.tag, hit.mean(), cs.share, z)


@pytest.mark.parametrize("b_first", [False, True])
def test_two_media_casts(rtsr, orc, b_first):
    """Who scatters first, from ids[:, 1] of 2^18 casts along the axis: the closed shares, and the core's records on the first
    4096 rays bit for bit."""
    case = mc.build(rtsr, "two_media", b_first=b_first)
    q = case.points[0]
    n = mc.N_SAMPLES
    o, d = np.ascontiguousarray(np.tile(q.o, (n, 1))), np.ascontiguousarray(np.tile(q.d, (n, 1)))
    h = _scene(case).cast_rays(o, d, None, None, seed=mc.SEED, stream_step=1, want=("t", "ids"))
    ma, mb = case.flat.medium(case.extra["slot_a"])["material"], case.flat.medium(case.extra["slot_b"])["material"]
    args = (mc.TWO["rho_a"], 4.0, 8.0, mc.TWO["rho_b"], 7.0, 10.0)
    want = mc.later_first_shares(*args) if b_first else mc.two_media_shares(*args)
    got = ((h.ids[:, 1] == ma).mean(), (h.ids[:, 1] == mb).mean(), (h.ids[:, 0] == 0).mean())
    for w, g in zip(want, got):
        assert abs(g - w) / np.sqrt(w * (1.0 - w) / n) <= mc.Z_CAP, (want, got)
    for r in range(4096):
        rec = orc.core_world_hit_mat(case.flat.arrays_ptr(), q.o, q.d, rng_seed=mc.SEED + r)
        assert (rec is None) == (h.ids[r, 0] == 0)
        assert rec is None or (rec["mat"] == h.ids[r, 1] and rec["t"] == h.t[r]), (r, rec, h.t[r])


# ---- frames --------------------------------------------------------------------------------------------------------------
def test_glass_balls_through_every_walker_of_a_sphere_bvh(rtsr, orc, monkeypatch):
    case = mc.build(rtsr, "glass_balls")
    ref, ref8 = _o2(rtsr, orc, case)
    for env, kernel in (({}, "k_trace_lds"), ({"RTX_TRACE_KERNEL": "vote"}, "k_trace_vote"), ({"RTX_TRACE_KERNEL": "wavefront"}, "k_wf_trace"),
                        ({"RTX_TRACE_KERNEL": "world"}, "k_trace_world"), ({"RTX_TRACE_KERNEL": "simple"}, "k_trace_simple")):
        _, got = _render_under(monkeypatch, case, env)
        assert _kernel(rtsr, got) == kernel, (env, _kernel(rtsr, got))
        assert np.array_equal(got.accum, ref), (env, _diff(got.accum, ref))
        assert np.array_equal(got.rgb8, ref8), env


PRESETS = {"media_sphere": "P_BOOK2", "two_media": "P_BOOK2", "pair": "P_BOOK2", "glass_pane": "P_BOOK2", "metal_mirror": "P_BOOK2",
           "metal_fuzz": "P_BOOK2", "casts": "P_NO_SPHERE_MEDIA", "media_general": "P_NO_SPHERE_MEDIA", "isotropic_slab": "P_NO_SPHERE_MEDIA"}


@pytest.mark.parametrize("name,variant", WORLDS, ids=mc.case_id)
def test_list_worlds_through_k_trace_world_and_k_trace_simple(rtsr, orc, monkeypatch, name, variant):
    case = mc.build(rtsr, name, **variant)
    if variant.get("slab"):
        assert _preset(orc, case) == "P_ANY"
    elif name == "surface_in_front":
        assert _preset(orc, case) == ("P_BOOK2" if variant.get("ball", True) else "P_NO_SPHERE_MEDIA")
    else:
        assert _preset(orc, case) == PRESETS[name], (name, _preset(orc, case))
    ref, ref8 = _o2(rtsr, orc, case)
    a1, r1 = orc.o1_render(case.b.graph_ptr(), case.world, case.cam, case.cfg, rtsr.image_height(case.cfg), threads=16)
    assert np.array_equal(a1, ref) and np.array_equal(r1, ref8)
    for env, kernel in (({}, "k_trace_world"), ({"RTX_TRACE_KERNEL": "simple"}, "k_trace_simple")):
        scene, got = _render_under(monkeypatch, case, env)
        assert _kernel(rtsr, got) == kernel, (name, env, _kernel(rtsr, got))
        assert np.array_equal(got.accum, a1), (name, env, _diff(got.accum, a1))
        assert np.array_equal(got.rgb8, r1), (name, env)
    if name == "pair":
        # the device's own record of the pair: slot k is flagged exactly when slot k + 1 is a medium in the very same sphere
        desc = np.frombuffer(scene.array("world_desc"), dtype=np.int32).reshape(-1, 48)
        assert bool((desc[:, 0] & WD_PAIR).any()) == case.extra["pairs"], (variant, desc[:, 0])


@pytest.mark.parametrize("name,variant", WORLDS, ids=mc.case_id)
@pytest.mark.parametrize("extra", ["gravity", "instance", "bvh"])
def test_list_worlds_with_a_neighbour_that_changes_the_walker(rtsr, orc, chk, monkeypatch, name, variant, extra):
    case = mc.build(rtsr, name, extra=extra, **variant)
    info = case.flat.info()
    assert info["n_gravity_spheres"] == (extra == "gravity") and case.flat.instances()["n_trees"] == (extra == "instance")
    assert _preset(orc, case) == {"gravity": "P_ALL", "instance": "P_INST"}.get(extra, _preset(orc, mc.build(rtsr, name, **variant)))
    for text, ok in case.conditions:
        assert ok, (name, extra, text)
    ref, ref8 = _o2(rtsr, orc, case)
    want = mc.host_sums(chk, case, replicas=1, spp=256)
    # (beside a BVH the panes, which hold plain rectangles only, are k_trace_vote's by default -- _default_kernel restates
    # choose_trace_kernel: that frame is held as well, and k_trace_world is asked for by name on either tree)
    forced = ({"RTX_TRACE_KERNEL": "world", "RTX_WIDE": "0"}, {"RTX_TRACE_KERNEL": "world", "RTX_WIDE": "1"}, {})
    for env in forced if extra == "bvh" else ({},):
        scene, got = _render_under(monkeypatch, case, env)
        if extra == "bvh" and not env:
            assert _kernel(rtsr, got) == _default_kernel(orc, case), (name, variant, _kernel(rtsr, got))
            assert (_kernel(rtsr, got) == "k_trace_vote") == (name in ("glass_pane", "metal_mirror", "metal_fuzz")), (name, _kernel(rtsr, got))
        else:
            assert _kernel(rtsr, got) == "k_trace_world", (env, _kernel(rtsr, got))
            assert (scene.wide_levels() > 0) == (env.get("RTX_WIDE") == "1"), (env, scene.wide_levels())
        assert np.array_equal(got.accum, ref, equal_nan=True), (env, _diff(got.accum, ref))
        assert np.array_equal(got.rgb8, ref8), env
        assert np.array_equal(mc.bits(_device_sums(scene, case, 1, 256)), mc.bits(want)), env


# ---- light sampling --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nee_chk(tmp_path_factory):
    return lc.nee_checker(tmp_path_factory)


@pytest.mark.parametrize("name,variant", [("media_sphere", {}), ("media_general", {}), ("pair", {"kind": "same"}), ("pair", {"kind": "second_behind"}),
                                          ("surface_in_front", {"after": True})], ids=mc.case_id)
def test_media_under_light_sampling(rtsr, nee_chk, name, variant):
    import ctypes as C
    case = mc.build(rtsr, name, **variant)
    assert case.flat.lights()["n_lights"] >= 1
    gpu = _scene(case).render(case.cam, case.cfg, light_sampling=True, want_stats=True)
    assert rtsr.trace_kernel_name(gpu.stats.trace_kernel) == "k_trace_nee"
    D = C.POINTER(C.c_double)
    camarr = np.frombuffer(bytes(case.cam), dtype=np.float64).copy()
    bg = np.array(case.cfg.background[:3], dtype=np.float64)
    h = rtsr.image_height(case.cfg)
    host = np.zeros((h, mc.FRAME_WIDTH, 3))
    rc = nee_chk(case.flat.arrays_ptr(), camarr.ctypes.data_as(D), bg.ctypes.data_as(D), mc.FRAME_WIDTH, h, mc.FRAME_SPP, mc.FRAME_DEPTH, case.cfg.seed,
                 host.ctypes.data_as(D))
    assert rc == 0
    assert np.array_equal(gpu.accum, host), (name, _diff(gpu.accum, host))


# ---- the f32 scene -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("glass_pane", {"ir": ir}) for ir in mc.IRS] + [("metal_mirror", {}), ("metal_fuzz", {})], ids=mc.case_id)
def test_f32_glass_and_metal_equal_the_float_judge(rtsr, chk, name, variant):
    """Glass and metal reach only + - * / and sqrt: the float scene equals the float judge bit for bit.  (Its sums are NOT held
    to the closed forms: a float cannot hold 1e-9 rad or a strip of 1e-6.)"""
    case = mc.build(rtsr, name, **variant)
    want = mc.host_sums(chk, case, replicas=JUDGED, spp=256, f32=True)
    o, d, t = case.rays(JUDGED)
    got = _scene(case, f32=True).trace_rays(o, d, t, spp=256, max_depth=case.max_depth, background=case.background, seed=mc.SEED).sum
    assert np.array_equal(mc.bits(got), mc.bits(want)), int((~tc.same_bits(got, want)).sum())


@pytest.mark.parametrize("name", ["media_sphere", "media_general"])
def test_f32_media_counts_against_the_closed_forms(rtsr, name):
    """Media reach logf: the float scene's counts are held to the closed forms under the same cap.  Points whose origin lies in
    the medium are left to the f64 scene: the float mode's t_min grows with |origin| (geometry.hpp: ray_t_min), and with it the
    stretch of medium such a ray is exempt from."""
    case = mc.build(rtsr, name)
    o, d, t = case.rays(case.replicas)
    S = _scene(case, f32=True).trace_rays(o, d, t, spp=mc.SPP, max_depth=case.max_depth, background=case.background, seed=mc.SEED).sum
    counts, whole = mc.counts_of(case, S)
    assert whole
    keep = [k for k, q in enumerate(case.points) if "inside" not in q.tag and "centre" not in q.tag.replace("off centre", "")]
    assert len(keep) >= 8
    sub = type("Sub", (), dict(points=[case.points[k] for k in keep], name=case.name + " f32", replicas=case.replicas))
    lines, failed = mc.check_counts(sub, counts[keep])
    print("\n[material cases, f32] " + "\n[material cases, f32] ".join(lines))
    assert not failed, failed


# The float cast against the float judge.  t = t1 + (neg_inv_density * logf(u)) / |d|.  The device's logf is within
# MATH_ULP["logf"] = 3 float ulps of the correctly rounded value (tests/test_gpu_f32_parity.py) and glibc's within 1: the two
# logarithms part by at most (3 + 0.5 + 1) ulps, 4.5 x 2^-23 relative.  The product and the quotient round once each on either
# side (4 x 2^-24), so the two distances d = t - t1 part by at most 6.5 x 2^-23 |d|; the sum rounds once on either side, half an ulp
# of t each: |t_device - t_judge| <= 6.5 x 2^-23 |t - t1| + 2^-23 |t|.  A verdict may differ only where the judge's distance is
# within that of the far end.
def LOGF_T_BOUND(t, t1):
    return 6.5 * 2.0 ** -23 * np.abs(t - t1) + 2.0 ** -23 * np.abs(t)


def test_f32_casts_within_the_logf_bound(rtsr, orc):
    case = mc.build(rtsr, "casts")
    scene = _scene(case, f32=True)
    n_flip = n = 0
    for cs in case.extra["sets"]:
        if cs.verdict != "restated" or cs.density <= 0 or abs(cs.dx) != 1.0 or cs.x1 - cs.x0 < 1.0 or cs.t_min < 0:
            continue   # (chords of 1e-4 are not a float's to resolve; core32_world_hit reads a negative t_min as "the integrator's own guard")
        m = min(cs.n, 2048)
        o, d = cs.rays()
        h = scene.cast_rays(o[:m], d[:m], None, None, t_min=cs.t_min, t_max_all=cs.t_max, seed=mc.SEED + cs.first, stream_step=1, want=("t", "ids"))
        t1 = np.float32(max((cs.x0 - cs.ox) / cs.dx, cs.t_min, 0.0))
        t2 = np.float32(min((cs.x1 - cs.ox) / cs.dx, cs.t_max))
        for r in range(m):
            rec = orc.core32_world_hit(case.flat.arrays_ptr(), o[r], d[r], 0.0, cs.t_min, cs.t_max, rng_seed=mc.SEED + cs.first + r)
            hit = h.ids[r, 0] == 1
            n += 1
            if hit != (rec is not None):
                t = h.t[r] if hit else rec["t"]
                assert abs(t - t2) <= LOGF_T_BOUND(t2, t1), (cs.tag, r, t, t2)
                n_flip += 1
            elif hit:
                assert abs(h.t[r] - rec["t"]) <= LOGF_T_BOUND(rec["t"], t1), (cs.tag, r, h.t[r], rec["t"])
    print("\n[material cases, f32] %d casts, %d verdicts differ at the far end" % (n, n_flip))
    assert n >= 6000 and n_flip <= n // 1000
