"""The device on the cases of tests/texture_cases.py (proven on the CPU in tests/test_texture_cases.py).

Probes: every probe ray of every case through Scene.trace_rays, bit for bit against the f64 host checker; the f32 scene
against the float judge -- bit for bit where no platform function is reached, else within the device's pinned ulp bounds.
Uv columns: Scene.cast_rays on image_lookup and sphere_uv, the NaN of a sphere's pole included.
Walkers: small frames against O2 through every walker a case can reach, RtxRenderStats.trace_kernel asserted each time.
Every list world also runs beside a gravity sphere (k_trace_world<P_ALL>), a two-member instance tree (<P_INST>) and a BVH of
200 spheres (binary and 4-wide tree), frame and probes each time.
Placement: perlin_tables with 1, 2 and 3 tables and table_limits at 64 / 65 records, under the switches that move
k_trace_world's tables between LDS and HBM, with and without a deep BVH beside them.

Combinations a case cannot reach, and why (the launcher cannot select them for that scene; render.hip: choose_trace_kernel):
  * k_trace_lds, k_trace_vote and k_wf_trace take worlds of one BVH of spheres with Lambertian / metal / dielectric
    materials over solid and checker textures: only the BVH form of checker_depth is theirs.  Every list world -- lights,
    rectangles, noise and image textures -- is k_trace_world's (or k_trace_simple's when forced).
  * The 4-wide tree exists only for a world with a BVH (plan_wide): of the list worlds, the ones with the 200-sphere BVH
    beside them.  A world with an instance tree keeps the binary tree."""
import numpy as np
import pytest

import cast_rays_cases as cc
import texture_cases as tx
import trace_rays_cases as tc
from test_texture_cases import VARIANTS, _id

pytestmark = pytest.mark.gpu

PLACEMENTS = ({}, {"RTX_MAT_LDS": "0"}, {"RTX_PERLIN_LDS": "0"}, {"RTX_MAT_LDS": "0", "RTX_PERLIN_LDS": "0"})
_scenes = {}


@pytest.fixture(scope="module")
def chk(orc, tmp_path_factory):
    return tc.checkers(tmp_path_factory)


def _scene(case, f32=False):
    """The case's resident scene under the default switches (uploaded once)."""
    if (id(case), f32) not in _scenes:
        _scenes[(id(case), f32)] = case.flat.upload(f32=f32)
    return _scenes[(id(case), f32)]


def _trace(scene, case, o, d, t):
    return scene.trace_rays(o, d, t, spp=1, max_depth=case.max_depth, background=case.background, seed=1).sum


def _kernel(rtsr, screen):
    return rtsr.trace_kernel_name(screen.stats.trace_kernel)


def _render_under(monkeypatch, case, env):
    """A fresh upload under the switches of env (they are read per upload) -> (scene, frame)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene = case.flat.upload()
    screen = scene.render(case.cam, case.cfg, want_stats=True)
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
@pytest.mark.parametrize("name,variant", VARIANTS, ids=_id)
def test_every_probe_equals_the_host_judge(rtsr, orc, chk, name, variant):
    case = tx.build(rtsr, orc, name, **variant)
    ps, o, d, t = case.rays()
    _, want = tx.host_values(chk, case)
    got = _trace(_scene(case), case, o, d, t)
    bad = np.nonzero(~tc.same_bits(got, want))[0]
    print("\n[texture cases] %s %s: %d probes, %d differ from the host judge" % (name, variant, len(ps), len(bad)))
    assert len(bad) == 0, [(ps[k].tag, ps[k].o, got[k], want[k]) for k in bad[:5]]
    assert np.array_equal(tx.bits(got), tx.bits(want))  # (no sum is a NaN: the pole's NaN ends in a texel)


# The float mode against the float judge.  Where a probe reaches no platform function -- checker parity (only the sign of sinf),
# an image on a rectangle, a triangle or a moving sphere, solid colours -- the sums are equal bit for bit.  Where it reaches
# sinf (a noise texture): the device's sinf is within MATH_ULP["sinf"] = 3 float ulps of the correctly rounded value
# (tests/test_gpu_f32_parity.py, pinned over |x| <= 1e5) and glibc's within 1, both of a result of magnitude <= 1, whose ulp
# is at most 2^-24: the two sines part by at most (3 + 0.5 + 1) 2^-24.  1 + s rounds once on either side (half an ulp of a
# number below 2, 2^-24 each) and the product with 0.5 is exact: |difference of 0.5 (1 + s)| <= 0.5 (4.5 + 2) 2^-24 < 2^-22.
# The argument of the sine is the same float on both sides (+ - * and floor only).
NOISE_F32_BOUND = 2.0 ** -22
# Where it reaches acosf / atan2f (a sphere's (u, v)): within 2 and 3 ulps of values up to pi, ulp 2^-22, so u = (phi + pi) / 2 pi
# and v = theta / pi part from the judge's by less than 2^-20 after their roundings, and u * 8, v * 4 by less than 2^-17: the
# texel is the judge's unless the judge's own u * 8 or (1 - v) * 4 lies that close to an integer.
UV_F32_BOUND = 2.0 ** -17


@pytest.mark.parametrize("name", tx.CASES)
def test_f32_probes_against_the_float_judge(rtsr, orc, chk, name):
    case = tx.build(rtsr, orc, name)
    ps, o, d, t = case.rays(only_f32=True)
    _, want = tx.host_values(chk, case, f32=True)
    got = _trace(_scene(case, f32=True), case, o, d, t)
    n_exact = n_bound = n_open = 0
    for k, q in enumerate(ps):
        if np.array_equal(tx.bits(got[k]), tx.bits(want[k])):
            n_exact += 1
            continue
        if q.tag.endswith("noise") or name in ("perlin_points", "perlin_tables"):
            n_bound += 1
            assert abs(got[k] - want[k]).max() <= NOISE_F32_BOUND and abs(o[k]).max() < 1.0e3, (q.tag, q.o, got[k], want[k])
            continue
        assert name == "sphere_uv", (q.tag, q.o, got[k], want[k])  # tier A everywhere else: bit for bit
        rec = orc.core32_world_hit(case.flat.arrays_ptr(), q.o, q.d)
        near = lambda x: abs(x - np.round(x)) < UV_F32_BOUND
        assert not np.isnan(rec["v"]) and (near(rec["u"] * 8.0) or near((1.0 - rec["v"]) * 4.0)), (q.tag, q.o, rec, got[k], want[k])
        n_open += 1
    print("\n[texture cases] %s f32: %d probes, %d bit-equal, %d within the sinf bound, %d at a texel border" % (name, len(ps), n_exact, n_bound, n_open))
    assert n_open <= len(ps) // 4


# ---- uv columns ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["image_lookup", "sphere_uv"])
def test_uv_columns_equal_the_core(rtsr, orc, name):
    """(u, v), t and the material of every probe's first hit through Scene.cast_rays, against core_world_hit_mat: by bit
    pattern up to the sign and payload of a NaN (cast_rays_cases.same_bits; 0 / 0 sets the sign bit on x86-64 and clears it on
    gfx950).  The pole's v = NaN must arrive as a NaN: a min / max clamp further on would have turned it into a bound."""
    case = tx.build(rtsr, orc, name)
    ps, o, d, t = case.rays()
    hits = _scene(case).cast_rays(o, d, t)
    n_nan = 0
    for k, q in enumerate(ps):
        rec = orc.core_world_hit_mat(case.flat.arrays_ptr(), q.o, q.d, time=q.time)
        assert rec is not None and hits.ids[k, 0] == 1 and hits.ids[k, 1] == rec["mat"], (q.tag, q.o)
        want = np.array([[rec["u"], rec["v"], rec["t"]]])
        got = np.array([[hits.uv[k, 0], hits.uv[k, 1], hits.t[k]]])
        assert cc.same_bits(got, want)[0], (q.tag, q.o, got, want)
        n_nan += bool(np.isnan(hits.uv[k, 1]))
    assert (n_nan >= 1) == (name == "sphere_uv")


# ---- walkers -------------------------------------------------------------------------------------------------------------
def test_checker_chains_through_every_walker_of_a_sphere_bvh(rtsr, orc, monkeypatch):
    """checker_depth as one BVH of spheres: k_trace_lds by default, its vote and wavefront partners, k_trace_world and
    k_trace_simple when forced -- chains of 16 checkers through every copy of texture_value's loop."""
    case = tx.build(rtsr, orc, "checker_depth", as_bvh=True)
    ref, ref8 = _o2(rtsr, orc, case)
    for env, kernel in (({}, "k_trace_lds"), ({"RTX_TRACE_KERNEL": "vote"}, "k_trace_vote"), ({"RTX_TRACE_KERNEL": "wavefront"}, "k_wf_trace"),
                        ({"RTX_TRACE_KERNEL": "world"}, "k_trace_world"), ({"RTX_TRACE_KERNEL": "simple"}, "k_trace_simple")):
        _, got = _render_under(monkeypatch, case, env)
        assert _kernel(rtsr, got) == kernel, (env, _kernel(rtsr, got))
        assert np.array_equal(got.accum, ref), (env, _diff(got.accum, ref))
        assert np.array_equal(got.rgb8, ref8), env


@pytest.mark.parametrize("name", tx.CASES)
def test_list_worlds_through_k_trace_world_and_k_trace_simple(rtsr, orc, monkeypatch, name):
    case = tx.build(rtsr, orc, name)
    ref, ref8 = _o2(rtsr, orc, case)
    for env, kernel in (({}, "k_trace_world"), ({"RTX_TRACE_KERNEL": "simple"}, "k_trace_simple")):
        _, got = _render_under(monkeypatch, case, env)
        assert _kernel(rtsr, got) == kernel, (name, env, _kernel(rtsr, got))
        assert np.array_equal(got.accum, ref, equal_nan=True), (name, env, _diff(got.accum, ref))
        assert np.array_equal(got.rgb8, ref8), (name, env)


@pytest.mark.parametrize("name", tx.CASES)
@pytest.mark.parametrize("extra", ["gravity", "instance", "bvh"])
def test_list_worlds_with_a_neighbour_that_changes_the_walker(rtsr, orc, chk, monkeypatch, name, extra):
    """Every list world with a gravity sphere beside its patches (k_trace_world<P_ALL>), with a two-member instance tree
    (<P_INST>), and with a BVH of 200 spheres on the binary and on the 4-wide tree: the frame is O2's, and every probe the host
    judge's and its closed form's, each time."""
    case = tx.build(rtsr, orc, name, extra=extra)
    info = case.flat.info()
    assert info["n_gravity_spheres"] == (extra == "gravity") and case.flat.instances()["n_trees"] == (extra == "instance")
    assert (info["n_bvh"] == 1 and info["max_stack"] >= 6) == (extra == "bvh")
    for text, ok in case.conditions:
        assert ok, (name, extra, text)
    ref, ref8 = _o2(rtsr, orc, case)
    ps, o, d, t = case.rays()
    _, want = tx.host_values(chk, case)
    for env in ({"RTX_WIDE": "0"}, {"RTX_WIDE": "1"}) if extra == "bvh" else ({},):
        scene, got = _render_under(monkeypatch, case, env)
        assert _kernel(rtsr, got) == "k_trace_world", (env, _kernel(rtsr, got))
        assert (scene.wide_levels() > 0) == (env.get("RTX_WIDE") == "1"), (env, scene.wide_levels())
        assert np.array_equal(got.accum, ref, equal_nan=True), (env, _diff(got.accum, ref))
        assert np.array_equal(got.rgb8, ref8), env
        sums = _trace(scene, case, o, d, t)
        assert np.array_equal(tx.bits(sums), tx.bits(want)), env
        for k, q in enumerate(ps):
            if q.expected is not None:
                assert np.array_equal(tx.bits(sums[k]), tx.bits(q.expected)), (env, q.tag, q.o, sums[k], q.expected)


# ---- placement -----------------------------------------------------------------------------------------------------------
# The rule below is read off plan_world_stacks (csrc/hip/render.hip): the Perlin tables ride in LDS for 1 or 2 tables, not
# from 3 on; the material and texture tables for 1 .. 64 records of EACH, the texture copy behind the material copy, both
# behind the stacks (max_stack + 1 levels) and the Perlin copy.  RtxRenderStats does not report the placement, so the counts
# the plan reads are asserted and every placement must render the same frame.
PLACED = [("perlin_tables", {"n_tables": 1}), ("perlin_tables", {"n_tables": 2}), ("perlin_tables", {}), ("perlin_tables", {"extra": "bvh"}),
          ("table_limits", {}), ("table_limits", {"n_mat": 65, "n_tex": 64}), ("table_limits", {"n_mat": 64, "n_tex": 65}),
          ("table_limits", {"n_mat": 65, "n_tex": 65}), ("table_limits", {"extra": "bvh"}), ("checker_depth", {})]


@pytest.mark.parametrize("name,variant", PLACED, ids=_id)
def test_table_placement_is_invisible(rtsr, orc, monkeypatch, name, variant):
    case = tx.build(rtsr, orc, name, **variant)
    info = case.flat.info()
    if name == "perlin_tables":
        assert info["n_perlins"] == variant.get("n_tables", 3) and info["n_materials"] <= 64 and info["n_textures"] <= 64
    if name == "table_limits":
        assert (info["n_materials"], info["n_textures"]) == (variant.get("n_mat", 64), variant.get("n_tex", 64)) and info["n_perlins"] == 0
    if name == "checker_depth":
        assert info["n_textures"] > 64 and info["n_materials"] <= 64 and info["n_perlins"] == 1  # the textures alone keep both in HBM
    assert (info["max_stack"] >= 6) == (variant.get("extra") == "bvh")
    # (what the frame shows -- every rectangle's own colour and both children of the last checker, every Perlin table -- is
    # asserted on the CPU: tests/test_texture_cases.py.  Scene.trace_rays runs k_trace_rays, which has no table copies.)
    ref, ref8 = _o2(rtsr, orc, case)
    for env in PLACEMENTS:
        scene, got = _render_under(monkeypatch, case, env)
        assert scene.max_stack() == info["max_stack"]
        assert _kernel(rtsr, got) == "k_trace_world", (env, _kernel(rtsr, got))
        assert np.array_equal(got.accum, ref), (env, _diff(got.accum, ref))
        assert np.array_equal(got.rgb8, ref8), env
