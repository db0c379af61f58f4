"""The cases of tests/texture_cases.py on the CPU, before the device sees them (tests/test_gpu_texture_cases.py): every case's
conditions hold; the host judge (tests/rays_host_check.cpp, what the device is compared with), the O1 and core texture probes,
the closed forms and the numpy restatement of the noise agree bit for bit as each case says; O1 == O2 on a small frame of
every case; the float core agrees with float closed forms where no platform function is reached (checker parity, image
lookup on rectangles) and with the float judge everywhere; and a checker chain of 16 equals O1 while one of 17 is refused."""
import numpy as np
import pytest

import texture_cases as tx
import trace_rays_cases as tc

VARIANTS = [(name, {}) for name in tx.CASES] + [("perlin_tables", {"n_tables": 1}), ("perlin_tables", {"n_tables": 2})] + \
           [("table_limits", {"n_mat": m, "n_tex": t}) for m, t in ((65, 64), (64, 65), (65, 65))] + \
           [("image_lookup", {"extra": "instance"}), ("table_limits", {"extra": "gravity"}), ("perlin_tables", {"extra": "bvh"}),
            ("checker_depth", {"extra": "instance"}), ("checker_edges", {"extra": "bvh"}), ("perlin_points", {"extra": "instance"}),
            ("sphere_uv", {"extra": "gravity"}), ("scatter", {"extra": "bvh"})]
FLAT_MATERIAL = np.dtype([("kind", np.int32), ("tex", np.int32), ("albedo", np.float64, (3,)), ("param", np.float64), ("needs_uv", np.int32), ("pad", np.int32)])
FLAT_IMAGE = np.dtype([("width", np.int32), ("height", np.int32), ("first_texel", np.int64)])


def _id(v):
    return v if isinstance(v, str) else ("-".join("%s=%s" % kv for kv in sorted(v.items())) or "plain")


@pytest.fixture(scope="module")
def chk(orc, tmp_path_factory):
    return tc.checkers(tmp_path_factory)


def _same(a, b):
    return np.array_equal(tx.bits(a), tx.bits(b))


def _hit_bits(rec):
    return tx.bits([rec["t"], rec["u"], rec["v"]] + list(rec["p"]) + list(rec["normal"]))


def _expected_of(case, orc, q):
    """(rgb the closed form or O1 names for probe q, the (u, v, p) of its Texture::value call)."""
    if q.handle is not None:
        # (u, v, p) are the literal restatement's; the core must find the same record, a NaN included
        rec = orc.o1_hit(case.b.graph_ptr(), q.handle, q.o, q.d, time=q.time)
        core = orc.core_world_hit(case.flat.arrays_ptr(), q.o, q.d, time=q.time)
        assert rec is not None and core is not None and np.array_equal(_hit_bits(rec), _hit_bits(core)), (case.name, q.tag)
        texels = case.extra["texels"][2] if case.name == "image_lookup" else case.extra["texels"]
        return tx.image_value(texels, rec["u"], rec["v"]), (rec["u"], rec["v"], rec["p"])
    return q.expected, (q.u, q.v, q.p if q.p is not None else (0.0, 0.0, 0.0))


@pytest.mark.parametrize("name,variant", VARIANTS, ids=_id)
def test_conditions_hold_and_every_judge_agrees(rtsr, orc, chk, name, variant):
    case = tx.build(rtsr, orc, name, **variant)
    for text, ok in case.conditions:
        assert ok, (name, text)
    assert case.conditions and 0 < len(case.probes) <= 400
    ps, S = tx.host_values(chk, case)
    n_closed = 0
    for q, s in zip(ps, S):
        expected, (u, v, p) = _expected_of(case, orc, q)
        if expected is not None:
            n_closed += 1
            assert _same(s, expected), (name, q.tag, q.o, s, expected)
        a = orc.o1_texture_value(case.b.graph_ptr(), q.tex, u, v, p)
        b = orc.core_texture_value(case.flat.arrays_ptr(), q.tex, u, v, p)
        assert _same(a, s) and _same(b, s), (name, q.tag, q.o, a, b, s)
    print("\n[texture cases] %s %s: %d probes, %d held by a closed form, all by O1, the core and the host judge" % (name, variant, len(ps), n_closed))
    if "closed" in case.judges and name != "perlin_points":
        assert 2 * n_closed >= len(ps)


def test_checker_depth_flags_and_needs_uv(rtsr, orc):
    case = tx.build(rtsr, orc, "checker_depth")
    f = orc.flat_features(case.flat.arrays_ptr())
    assert f & orc.F_CHECKER and f & orc.F_NOISE and f & orc.F_IMAGE
    mats = orc.flat_array(case.flat.arrays_ptr(), "materials")[0].view(FLAT_MATERIAL)
    by_tex = {int(m["tex"]): int(m["needs_uv"]) for m in mats}
    assert by_tex[case.extra["mixed"]] == 1
    # needs_uv through nesting: 1 exactly for the nine chains over the image and for the mixed tree
    assert sum(by_tex.values()) == case.extra["n_chains"] // 2 + 1 and len(by_tex) == case.extra["n_chains"] + 1
    tags = {q.tag for q in case.probes}
    assert {"image/both/16", "image/odd/16", "image/even/16", "solid/both/16", "solid/odd/1", "solid/even/2"} <= tags


def test_perlin_closed_forms_and_the_restatement(rtsr, orc, chk):
    """Lattice points, the period of 256, the indices beyond i32, and every noise probe of every case against the numpy
    restatement (bit for bit: float64 in the reference's order, the final sine the project's rt_sin)."""
    case = tx.build(rtsr, orc, "perlin_points")
    tabs = tx.perlin_tables(orc, case.flat)
    assert len(tabs) == 3
    ps, S = tx.host_values(chk, case)
    scale_of = dict(zip(case.extra["tex"], case.extra["scales"]))
    table_of = {t: k for k, t in enumerate(case.extra["tex"][:3])}
    by_tag = {}
    for q, s in zip(ps, S):
        by_tag.setdefault(q.tag, []).append((q, s))
        assert s[0] == s[1] == s[2] and 0.0 <= s[0] <= 1.0
        assert _same(s[0], tx.perlin_restated(orc, tabs[table_of[q.tex]], scale_of[q.tex], q.p)), (q.tag, q.p)
    for q, s in by_tag["lattice"]:
        assert q.p[2] == 7.0 and all(c == np.floor(c) for c in q.p)
        assert _same(s[0], 0.5 * (1.0 + orc.rt_math("sin", [4.0 * 7.0])[0])), q.p
    period = by_tag["period"]
    assert len(period) % 4 == 0 and len(period) >= 24
    for g in range(0, len(period), 4):
        for q, s in period[g + 1:g + 4]:
            assert q.tex == period[g][0].tex and q.p != period[g][0].p
            assert _same(s, period[g][1]), (period[g][0].p, q.p)
    assert len({s[0] for _, s in period[::4]}) >= 10  # ... and the points themselves differ
    # beyond i32 the cast saturates, u = 0, and i + 1 wraps: indices 255 then 0 (from below: 0 then 1)
    for q, s in by_tag["past i32"]:
        trace = []
        tx.perlin_restated(orc, tabs[table_of[q.tex]], scale_of[q.tex], q.p, trace)
        axis = 0 if abs(q.p[0]) >= 2.0 ** 31 else 1
        for octave in trace:
            assert octave[axis] == ([255, 0] if q.p[axis] > 0 else [0, 1]) and octave[3][axis] == 0.0, (q.p, octave)
    for q, s in by_tag["octave past i32"]:
        trace = []
        tx.perlin_restated(orc, tabs[table_of[q.tex]], scale_of[q.tex], q.p, trace)
        assert trace[0][0] not in ([255, 0], [0, 1]) or abs(q.p[0]) < 2.0 ** 31
        assert trace[6][0] == ([255, 0] if q.p[0] > 0 else [0, 1]), (q.p, trace[6])
    assert all(q.p[0] < 0 and q.p[1] < 0 and q.p[0] != np.floor(q.p[0]) for q, _ in by_tag["negative"])
    assert len(by_tag["general"]) == 24 and len({s[0] for _, s in by_tag["general"]}) == 24
    # the noise children of the mixed trees
    for name in ("checker_depth", "scatter"):
        other = tx.build(rtsr, orc, name)
        tab = tx.perlin_tables(orc, other.flat)
        assert len(tab) == 1
        qs, T = tx.host_values(chk, other)
        noise = [(q, s) for q, s in zip(qs, T) if q.tag.endswith("/noise")]
        assert noise
        for q, s in noise:
            assert _same(s[0], tx.perlin_restated(orc, tab[0], 4.0 if name == "checker_depth" else -2.0, q.p)), (name, q.p)


@pytest.mark.parametrize("n_tables", [1, 2, 3])
def test_perlin_tables_differ_and_so_do_their_values(rtsr, orc, chk, n_tables):
    case = tx.build(rtsr, orc, "perlin_tables", **({} if n_tables == 3 else {"n_tables": n_tables}))
    tabs = tx.perlin_tables(orc, case.flat)
    assert len(tabs) == n_tables == case.flat.info()["n_perlins"]
    for a in range(n_tables):
        for b in range(a + 1, n_tables):
            assert not np.array_equal(tabs[a]["ranvec"], tabs[b]["ranvec"]) and not np.array_equal(tabs[a]["perm_x"], tabs[b]["perm_x"])
    ps, S = tx.host_values(chk, case)
    n = len(tx.LOCAL_POINTS)
    for k, q in enumerate(ps):
        assert _same(S[k][0], tx.perlin_restated(orc, tabs[k // n], 4.0, q.p)), q.p
    for j in range(n):
        values = {float(S[t * n + j][0]) for t in range(n_tables)}
        assert len(values) == n_tables, (j, values)
        # one table read for all of them would give one value: the rectangles are a period apart
        assert len({tx.perlin_restated(orc, tabs[0], 4.0, ps[t * n + j].p) for t in range(n_tables)}) == 1


@pytest.mark.parametrize("n_mat,n_tex", [(64, 64), (65, 64), (64, 65), (65, 65)])
def test_table_limits_have_the_counts_they_claim(rtsr, orc, n_mat, n_tex):
    case = tx.build(rtsr, orc, "table_limits", **({} if (n_mat, n_tex) == (64, 64) else {"n_mat": n_mat, "n_tex": n_tex}))
    info = case.flat.info()
    assert (info["n_materials"], info["n_textures"], info["n_rects"]) == (n_mat, n_tex, n_mat)
    tex = orc.flat_array(case.flat.arrays_ptr(), "textures")[0].view(np.int32).reshape(n_tex, -1)
    assert tuple(tex[-1][:3]) == (1, n_tex - 3, n_tex - 2)  # the last record: a checker over the two records before it
    # The frame the placement runs of tests/test_gpu_texture_cases.py compare with O2 shows EVERY rectangle's own colour and
    # both children of the last checker, sample by sample: a table copy that lost or mis-indexed any one record changes it.
    h = rtsr.image_height(case.cfg)
    seen = set()
    for j in range(h):
        for i in range(case.cfg.image_width):
            for k in range(case.cfg.samples_per_pixel):
                seen.add(tuple(orc.o2_sample(case.flat.arrays_ptr(), case.cam, case.cfg, h, i, j, k)))
    want = {tuple(q.expected) for q in case.probes}
    assert len(want) == n_tex - 1 and want <= seen, sorted(want - seen)


def test_the_perlin_tables_frame_shows_every_table(rtsr, orc):
    """The camera looks down -z at x in 320 -+ 323: the three rectangles (x in [0, 128], [256, 384], [512, 640], y in [0, 128]) fall
    into the pixel columns 1 .. 5, 14 .. 18 and 27 .. 30 of the 32, and each must be lit there in the frame the placement runs
    compare (the noise is 0.5 (1 + sin) > 0 almost everywhere)."""
    for n_tables in (1, 2, 3):
        case = tx.build(rtsr, orc, "perlin_tables", **({} if n_tables == 3 else {"n_tables": n_tables}))
        a2, _ = orc.o2_render(case.flat.arrays_ptr(), case.cam, case.cfg, rtsr.image_height(case.cfg), threads=4)
        lit = a2.any(axis=2).sum(axis=0)  # per column
        for k, (lo, hi) in enumerate(((1, 6), (14, 19), (27, 31))):
            assert (lit[lo:hi].min() >= 4) == (k < n_tables), (n_tables, k, lit)


def test_second_image_starts_behind_the_first(rtsr, orc):
    case = tx.build(rtsr, orc, "image_lookup")
    images = orc.flat_array(case.flat.arrays_ptr(), "images")[0].view(FLAT_IMAGE)
    assert [(int(i["width"]), int(i["height"])) for i in images] == list(tx.IMAGE_SIZES)
    assert [int(i["first_texel"]) for i in images] == [0, 1, 7, 39]
    kinds = {q.tag.split()[0] for q in case.probes}
    assert {"xy", "xz", "yz", "triangle", "moving", "turned"} <= kinds


def test_sphere_poles_one_nan_one_finite(rtsr, orc):
    case = tx.build(rtsr, orc, "sphere_uv")
    got = []
    for k in (0, 1):
        handle, origin = case.extra["pole %d" % k]
        rec = orc.o1_hit(case.b.graph_ptr(), handle, origin, (0.0, -1.0, 0.0))
        got.append(bool(np.isnan(rec["v"])))
        assert rec["u"] == 0.5
        if got[-1]:  # the reference reads texel row 0 there: clamp passes the NaN and `NaN as i32` is 0
            assert tx.texel_index(rec["u"], rec["v"], 8, 4) == (0, 4) and tx.texel_index(0.5, 1.0, 8, 4) == (0, 4)
            assert tx.texel_index(0.5, 0.0, 8, 4) == (3, 4)  # what a clamp that returns a bound for a NaN could read instead
    assert got == [True, False]
    seam = [q for q in case.probes if q.tag.startswith("seam")]
    us = [orc.o1_hit(case.b.graph_ptr(), q.handle, q.o, q.d)["u"] for q in seam]
    assert min(us) < 1e-3 and max(us) > 1.0 - 1e-3 and 0.0 in us, us


@pytest.mark.parametrize("name,variant", [(n, {}) for n in tx.CASES] + [("checker_depth", {"as_bvh": True})], ids=_id)
def test_o1_equals_o2_on_a_small_frame(rtsr, orc, name, variant):
    case = tx.build(rtsr, orc, name, **variant)
    h = rtsr.image_height(case.cfg)
    assert case.cfg.image_width <= 32 and case.cfg.samples_per_pixel == 2
    a1, r1 = orc.o1_render(case.b.graph_ptr(), case.world, case.cam, case.cfg, h, threads=8)
    a2, r2 = orc.o2_render(case.flat.arrays_ptr(), case.cam, case.cfg, h, threads=8)
    assert np.array_equal(a1, a2, equal_nan=True) and np.array_equal(r1, r2)
    assert len(np.unique(a1.reshape(-1, 3), axis=0)) >= 3, "the frame shows the case"  # (two colours at 2 spp: three sums)


def _image_value_f32(texels, x, a0, a1, y, b0, b1):
    """texture.rs:102-121 and the rectangle's (u, v) in IEEE single, operation by operation (numpy float32 arithmetic)."""
    f = np.float32
    u = (f(x) - f(a0)) / (f(a1) - f(a0))
    v = (f(y) - f(b0)) / (f(b1) - f(b0))
    uc, vc = min(max(u, f(0.0)), f(1.0)), f(1.0) - min(max(v, f(0.0)), f(1.0))
    h, w = texels.shape[:2]
    i, j = min(int(uc * f(w)), w - 1), min(int(vc * f(h)), h - 1)
    return (f(1.0) / f(255.0)) * texels[j, i].astype(f)


def test_float_core_is_exact_where_no_platform_function_is_reached(rtsr, orc, chk):
    """Checker parity (only the SIGN of sinf is used: tier A of tests/test_gpu_f32_parity.py's rule) and image lookup on
    rectangles, against closed forms in single precision; and the float probe against the float judge on every probe the
    float mode is held on (the same core twice, through two doors)."""
    edges = tx.build(rtsr, orc, "checker_edges")
    even, odd = np.float32((0.9, 0.8, 0.1)), np.float32((0.1, 0.2, 0.7))
    seen = set()
    for q in edges.probes:
        p32 = [float(np.float32(c)) for c in q.p]
        is_odd = tx.checker_is_odd(p32, f32=True)
        seen.add(is_odd)
        got = orc.core_texture_value(edges.flat.arrays_ptr(), q.tex, 0.0, 0.0, q.p, f32=True)
        assert np.array_equal(got.astype(np.float32), odd if is_odd else even), (q.tag, q.p)
    assert seen == {False, True}
    lookup = tx.build(rtsr, orc, "image_lookup")
    ps, S = tx.host_values(chk, lookup, f32=True)
    rects = {"xy": (3.0, 11.0, 1.0, 3.0, 0, 1, 2), "xz": (13.0, 20.0, -5.0, 0.0, 0, 2, 3), "yz": (1.0, 4.0, 5.0, 7.0, 1, 2, 1)}
    n = 0
    for q, s in zip(ps, S):
        kind = q.tag.split()[0]
        if kind not in rects or q.tag.endswith("1x1"):
            continue
        a0, a1, b0, b1, ia, ib, m = rects[kind]
        want = _image_value_f32(lookup.extra["texels"][m], q.p[ia], a0, a1, q.p[ib], b0, b1)
        assert np.array_equal(s.astype(np.float32), want) and np.array_equal(s.astype(np.float32).astype(np.float64), s), (q.tag, q.p)
        n += 1
    assert n >= 150
    for name in tx.CASES:
        case = tx.build(rtsr, orc, name)
        ps, S = tx.host_values(chk, case, f32=True)
        for q, s in zip(ps, S):
            if q.handle is not None or q.p is None:
                continue
            got = orc.core_texture_value(case.flat.arrays_ptr(), q.tex, q.u, q.v, q.p, f32=True)
            # (u, v) of an image on a rectangle are the float ray's own, not the narrowed f64 ones: the probe holds the rest
            if "image" in q.tag or name == "image_lookup" or (name == "scatter" and q.tag.endswith("image")):
                continue
            assert _same(got, s), (name, q.tag, q.p, got, s)


def test_the_chain_limit_is_one_constant(rtsr):
    """core/flat_types.hpp's RT_MAX_CHECKER_CHAIN bounds texture_value's loop and the flattener's refusal; the cases' MAX_CHAIN
    and the header's sentence at rtx_checker state the same number."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = lambda *p: open(os.path.join(root, "ray-tracing-series-rust_amd", "csrc", *p)).read()
    assert int(re.search(r"constexpr int RT_MAX_CHECKER_CHAIN = (\d+);", src("core", "flat_types.hpp")).group(1)) == tx.MAX_CHAIN
    assert "guard < RT_MAX_CHECKER_CHAIN" in src("core", "shading.hpp") and "<= rt::RT_MAX_CHECKER_CHAIN" in src("host", "flatten.cpp")
    assert "at most %d of them" % tx.MAX_CHAIN in open(os.path.join(root, "include", "rtx_abi.h")).read()


def test_the_lds_plan_keeps_the_records_the_launched_kernel_writes(rtsr, orc, tmp_path):
    """csrc/hip/lds_variant.inc, which plan_lds sizes the LDS by and launch_lds picks the instantiation by, asked on the host:
    Book-1's final scene (static spheres, no checker: P_STATIC_SPHERES exactly) keeps 40-byte sphere records; static spheres
    under a checker -- the BVH form of checker_depth, which faulted in k_trace_lds when the plan asked the scene for moving
    spheres instead -- and a world with movers keep moving-sphere records, one per leaf slot."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "lds_variant_host_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(root, "tests", "lds_variant_host_check.cpp"), "-o", exe], check=True)
    b = rtsr.Builder(1)
    world, _, _ = b.get_world_cam(rtsr.SCENE_BOOK1_CANONICAL)
    static_preset = orc.flat_features(b.flatten(world).arrays_ptr())
    case = tx.build(rtsr, orc, "checker_depth", as_bvh=True)
    info, f = case.flat.info(), orc.flat_features(case.flat.arrays_ptr())
    assert f == static_preset | orc.F_CHECKER and info["n_moving_spheres"] == 0 and info["n_bvh"] == 1
    ask = lambda feat, n_static, slots: [int(x) for x in subprocess.run([exe, "records", str(feat), str(static_preset), str(n_static), str(slots)],
                                                                         capture_output=True, text=True, check=True).stdout.split()]
    n = info["n_spheres"]
    assert ask(static_preset, n, n) == [0, n, 0, 0]
    assert ask(f, n, n) == [1, 0, n, n]
    assert ask(static_preset | 2, 5, n) == [1, 0, n, 5] and ask(static_preset | 2 | orc.F_CHECKER, 5, n) == [1, 0, n, 5]  # F_MOVING_SPHERE


@pytest.mark.parametrize("over_image", [False, True], ids=["solid", "image"])
def test_sixteen_checkers_equal_o1_and_seventeen_are_refused(rtsr, orc, chk, over_image):
    """texture_value follows a chain for 16 steps.  Before the flattener refused deeper chains, one of 17 rendered the
    `color` field of a checker record, (0, 0, 0), where O1 returns the leaf; needs_uv was lost at the same depth."""
    cam = rtsr.Camera.new((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0, 0.0, 10.0, 0.0, 1.0)
    cfg = rtsr.Config.new(1.0, 12, 2, 4, 4, seed=3, background=(0.0, 0.0, 0.0))
    for depth in (1, 15, 16):
        b, world, t = tx.deep_checker(rtsr, depth, over_image)
        flat = b.flatten(world)
        a1, _ = orc.o1_render(b.graph_ptr(), world, cam, cfg, 12, threads=4)
        a2, _ = orc.o2_render(flat.arrays_ptr(), cam, cfg, 12, threads=4)
        assert np.array_equal(a1, a2) and a1.any(), depth
        mats = orc.flat_array(flat.arrays_ptr(), "materials")[0].view(FLAT_MATERIAL)
        assert int(mats[-1]["needs_uv"]) == int(over_image)
    for depth in (17, 18, 40):
        b, world, t = tx.deep_checker(rtsr, depth, over_image)
        a1, _ = orc.o1_render(b.graph_ptr(), world, cam, cfg, 12, threads=4)
        assert a1.any()  # the reference shades it
        with pytest.raises(rtsr.RtxError, match="nested %d deep" % depth) as e:
            b.flatten(world)
        assert e.value.status == rtsr.RTX_EUNSUPPORTED
        # a deep texture nothing in the world wears stays allowed: the world of another material flattens
        plain = b.hittable_list([b.sphere((0.0, 0.0, 0.0), 1.0, b.lambertian((0.5, 0.5, 0.5)))])
        assert b.flatten(plain).info()["n_textures"] >= depth
