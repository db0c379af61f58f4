"""The cases of tests/material_cases.py on the CPU, before the device sees them (tests/test_gpu_material_cases.py): every case's
conditions and flags hold; every statistical point is met by the f64 host judge (tests/rays_host_check.cpp, what the device is
compared with) under light_cases.py's two caps; every deterministic expectation holds against o1_scatter, core_scatter, o1_hit
and core_world_hit; O1 equals the core bit for bit on every probe ray, the draws consumed included, and on adversarial hit
records (a zero normal, a normal of length 2, the direction that is EXACTLY at the critical angle); the casts equal their
numpy restatement; O1 == O2 on a small frame of every case, and on worlds with a NaN density or index (here only)."""
import numpy as np
import pytest

import material_cases as mc
import trace_rays_cases as tc


@pytest.fixture(scope="module")
def chk(orc, tmp_path_factory):
    return tc.checkers(tmp_path_factory)


def _same(a, b):
    return np.array_equal(mc.bits(a), mc.bits(b))


# ---- closed forms on their own ------------------------------------------------------------------------------------------
def test_closed_forms_stand_on_their_own():
    # the cap fraction against the rule itself, simulated in numpy
    for k, (c, f) in enumerate(((0.1, 1.0), (0.3, 0.5), (0.05, 0.25), (0.5, 1.0), (0.26, 0.25))):
        got, se = mc.simulate_absorbed(c, f, 4000000, 100 + k)
        want = mc.absorbed_share(c, f)
        print("[material cases] absorbed share at cos %g fuzz %g: closed form %.6f, simulated %.6f (SE %.6f)" % (c, f, want, got, se))
        assert (got == 0.0) if want == 0.0 else abs(got - want) <= 1.0 * se   # (within ONE standard error at these fixed seeds)
    assert mc.absorbed_share(0.1, 1.7) == mc.absorbed_share(0.1, float("inf")) == mc.absorbed_share(0.1, 1.0)
    assert mc.absorbed_share(0.3, -0.5) == mc.absorbed_share(0.3, 0.5) and mc.absorbed_share(0.3, 0.0) == 0.0
    # Schlick at the two ends, total reflection on the dense side only
    g = mc.glass_closed((0.0, -1.0, 0.0), 1.5, True)
    assert abs(g["share"] - 0.04) < 1e-15 and not g["tir"] and g["tan_t"] == 0
    assert mc.glass_closed(mc.unit_dir(np.deg2rad(89.0), True), 1.5, True)["tir"] is False
    assert mc.glass_closed(mc.unit_dir(np.deg2rad(42.0), False), 1.5, False)["tir"] is True
    assert mc.glass_closed(mc.unit_dir(np.deg2rad(41.0), False), 1.5, False)["tir"] is False
    assert mc.glass_closed(mc.unit_dir(np.deg2rad(89.9), False), 1.0, False)["tir"] is False
    # two media: the three shares are probabilities; without an overlap in densities the rule is symmetric in nothing
    args = (mc.TWO["rho_a"], 4.0, 8.0, mc.TWO["rho_b"], 7.0, 10.0)
    for shares in (mc.two_media_shares(*args), mc.later_first_shares(*args)):
        assert all(0.0 < s < 1.0 for s in shares) and abs(sum(shares) - 1.0) < 1e-15
    # (both orders let the same samples through: a sample passes when neither medium hits on its own interval)
    assert abs(mc.two_media_shares(*args)[2] - np.exp(-0.6 * 4.0 - 0.9 * 3.0)) < 1e-15
    assert abs(mc.later_first_shares(*args)[2] - np.exp(-0.6 * 4.0 - 0.9 * 3.0)) < 1e-15
    # (the two list orders are two derivations of the same competition of two exponentials: which slot draws first decides
    # the streams, not the shares)
    assert np.allclose(mc.two_media_shares(*args), mc.later_first_shares(*args), rtol=0, atol=1e-15)
    assert abs(mc.two_media_shares(*args)[0] - 0.886067400106552) < 1e-12
    # the slab's quadrature: the order is the first whose double moves the value by less than 1e-7; the shell's linear system
    # has the closed solution (1 - r0) / (1 + 3 r0)
    assert mc.slab_order() == mc.SLAB_ORDER
    assert abs(mc.slab_value(mc.SLAB_ORDER) - mc.slab_value(2 * mc.SLAB_ORDER)) <= 1e-7 * mc.slab_value(mc.SLAB_ORDER)
    assert abs(mc.shell_back_share(1.5) - 0.96 / 1.12) < 1e-14 and abs(mc.shell_back_share(2.4) - (1 - 0.49 / 2.89) / (1 + 3 * 0.49 / 2.89)) < 1e-12
    # the bins of the truncated exponential are equally likely under the exponential itself
    rng = np.random.RandomState(3)
    x = rng.exponential(1.0 / 1.25, 400000)
    x = x[x <= 2.0]
    counts = np.bincount(mc.truncated_bins(1.0 + x, 1.0, 3.0, 1.25), minlength=16)
    assert abs(counts - len(x) / 16.0).max() <= 4.5 * np.sqrt(len(x) * 15.0 / 256.0)


def test_list_tie_later_object_wins(rtsr, orc):
    """Two rectangles in one plane, one ray: the hit is the later one's, in either order (HittableList::hit accepts t ==
    closest_so_far); the strips of the panes rely on it."""
    for order in ((0, 1), (1, 0)):
        b = rtsr.Builder(1)
        mats = [b.diffuse_light(mc.RED), b.diffuse_light(mc.BLUE)]
        rects = [b.xz_rect(-5.0, 5.0, -5.0, 5.0, 1.0, mats[k]) for k in order]
        world = b.hittable_list(rects)
        flat = b.flatten(world)
        rec = orc.core_world_hit_mat(flat.arrays_ptr(), (0.3, 3.0, 0.2), (0.0, -1.0, 0.0))
        assert rec["t"] == 2.0 and rec["mat"] == mats[order[1]]
        o1 = orc.o1_hit(b.graph_ptr(), world, (0.3, 3.0, 0.2), (0.0, -1.0, 0.0))
        assert o1["t"] == 2.0


# ---- conditions and flags -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", mc.LIST_WORLDS + [("glass_balls", {})], ids=mc.case_id)
def test_conditions_and_flags(rtsr, orc, name, variant):
    case = mc.build(rtsr, name, **variant)
    for text, ok in case.conditions:
        assert ok, (name, variant, text)
    f = orc.flat_features(case.flat.arrays_ptr())
    general, sphere = bool(f & mc.F_MEDIUM_GENERAL), bool(f & mc.F_MEDIUM_SPHERE)
    want = {"media_sphere": (False, True), "media_general": (True, False), "casts": (True, False), "two_media": (False, True),
            "pair": (False, True), "glass_pane": (False, False), "metal_mirror": (False, False), "metal_fuzz": (False, False),
            "glass_balls": (False, False), "isotropic_slab": (True, False)}
    if name == "surface_in_front":
        assert (general, sphere) == ((False, True) if variant.get("ball", True) else (True, False))
    else:
        assert (general, sphere) == want[name], (name, general, sphere)
    info = case.flat.info()
    assert info["n_gravity_spheres"] == 0 and case.flat.instances()["n_trees"] == 0
    assert info["n_bvh"] == (1 if name in ("media_general", "glass_balls") else 0)
    if name == "glass_balls":
        assert info["n_top_level"] == 1 and info["n_spheres"] == 40 and info["n_rects"] == 0
    if name == "pair":
        # the device pairs a plain sphere with the medium in the NEXT slot when the two sphere records are equal bit for bit
        raw = case.flat.array("spheres")
        sp = np.frombuffer(raw, dtype=np.float64).reshape(-1, 5)[:, :4]
        kinds = case.flat.top_level_kinds()
        twins = [k for k in range(len(sp)) for j in range(len(sp)) if j != k and _same(sp[k], sp[j])]
        assert bool(twins) == (variant["kind"] in ("same", "slot_between", "second_behind", "medium_first")), (variant, sp)
        assert len(kinds) == info["n_top_level"]


def test_medium_density_is_stored_as_minus_one_over_it(rtsr):
    case = mc.build(rtsr, "casts")
    with np.errstate(divide="ignore"):
        for cs in case.extra["sets"]:
            stored = case.flat.medium(cs.slot)["neg_inv_density"]
            assert _same(stored, np.float64(-1.0) / np.float64(cs.density)), (cs.tag, stored)
    assert np.signbit(case.flat.medium([cs for cs in case.extra["sets"] if cs.tag == "density inf"][0].slot)["neg_inv_density"])


def test_an_infinite_fuzz_is_built_but_not_edited(rtsr):
    """rtx_metal takes +inf (stored as 1, hit.rs:1063); rtx_flat_set_shading refuses a value that is not finite, as
    include/rtx_abi.h says, and leaves the scene as it was."""
    case = mc.build(rtsr, "metal_fuzz")
    m = case.extra["mats"][6]
    assert case.flat.material(m)["param"] == 1.0
    with pytest.raises(rtsr.RtxError, match="not finite"):
        case.flat.set_shading([("metal", m, mc.METAL_ALBEDO, float("inf"))])
    assert case.flat.material(m)["param"] == 1.0


# ---- statistics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", mc.STATISTICAL, ids=mc.case_id)
def test_every_statistical_point_on_the_host_judge(rtsr, chk, name, variant):
    case = mc.build(rtsr, name, **variant)
    counts, whole = mc.counts_of(case, mc.host_sums(chk, case))
    assert whole, "a sum is not an integer count times the unit colour"
    lines, failed = mc.check_counts(case, counts)
    print("\n[material cases] " + "\n[material cases] ".join(lines or ["%s: %d points, all exact counts" % (case.name, len(case.points))]))
    assert not failed, failed
    assert (counts.sum(axis=1) <= case.replicas * mc.SPP).all() and counts[:, 1].sum() == 0   # no sample is green


def test_a_surface_in_front_of_a_medium_costs_no_draw(rtsr, chk):
    """The wall before the medium in the list: every sample is that of the world without the medium, bit for bit.  The wall
    after it: the medium draws first (some samples change) and the wall still takes every ray (no sample is black or green)."""
    for ball in (True, False):
        plain = mc.build(rtsr, "surface_in_front", medium=False)
        before = mc.build(rtsr, "surface_in_front", ball=ball)
        after = mc.build(rtsr, "surface_in_front", ball=ball, after=True)
        S0, S1, S2 = [mc.host_sums(chk, c, replicas=4, spp=1) for c in (plain, before, after)]
        assert _same(S0, S1), "the medium behind the wall drew from the stream"
        assert not _same(S0, S2), "the medium listed first did not draw"
        for S in (S0, S2):
            assert (S[:, 1] == 0).all() and ((S[:, 0] + S[:, 2]) == 1.0).all()
        assert 0.25 < S0[:, 0].mean() < 0.75


# ---- scatter probes ------------------------------------------------------------------------------------------------------
def _both_scatter(orc, case_or_builder_flat, mat, o, d, p, normal, ff, seed, time=0.0):
    b, flat = case_or_builder_flat
    a = orc.o1_scatter(b.graph_ptr(), mat, o, d, p, normal, ff, time=time, rng_seed=seed)
    c = orc.core_scatter(flat.arrays_ptr(), mat, o, d, p, normal, ff, time=time, rng_seed=seed)
    assert a["scattered"] == c["scattered"] and a["draws"] == c["draws"] >= 0 and _same(a["direction"], c["direction"]), (mat, d, normal, seed, a, c)
    if a["scattered"]:
        assert _same(a["attenuation"], c["attenuation"]), (mat, a, c)
    return c


@pytest.mark.parametrize("name,variant", mc.LIST_WORLDS + [("glass_balls", {})], ids=mc.case_id)
def test_o1_equals_the_core_on_every_probe_ray(rtsr, orc, name, variant):
    """The first hit of every probe ray (o1_hit on the world against core_world_hit, bit for bit, the medium's draw included)
    and Material::scatter on that record over eight streams: verdict, direction, attenuation and draws consumed."""
    case = mc.build(rtsr, name, **variant)
    n = 0
    for q in case.points:
        for seed in range(1, 5):
            a = orc.o1_hit(case.b.graph_ptr(), case.world, q.o, q.d, time=q.time, rng_seed=seed)
            c = orc.core_world_hit_mat(case.flat.arrays_ptr(), q.o, q.d, time=q.time, rng_seed=seed)
            assert (a is None) == (c is None), (name, q.tag)
            if a is None:
                continue
            # ((u, v) are left out: the flattener skips them for a material that reads no image)
            assert _same([a["t"]] + list(a["p"]) + list(a["normal"]), [c["t"]] + list(c["p"]) + list(c["normal"])) and a["front_face"] == c["front_face"], (name, q.tag, a, c)
            for s2 in (seed, seed + 100):
                _both_scatter(orc, (case.b, case.flat), c["mat"], q.o, q.d, c["p"], c["normal"], c["front_face"], s2, time=q.time)
                n += 1
    print("\n[material cases] %s %s: %d scatter probes, O1 == core" % (name, variant, n))
    assert n > 0


def test_glass_scatter_against_the_closed_forms(rtsr, orc):
    """Every probe of every pane: no uniform is drawn when the ray totally reflects and exactly one otherwise; the sample
    reflects when the closed-form share exceeds the stream's first uniform (the judge's own) and refracts otherwise; either
    direction is the mirror rule's or Snell's to 1e-12."""
    for ir in mc.IRS:
        case = mc.build(rtsr, "glass_pane", ir=ir)
        glass = 0   # the first material the builder made
        assert case.flat.material(glass)["kind"] == "dielectric" and case.flat.material(glass)["param"] == ir
        u = mc.first_uniforms(orc, 1, 8)
        for q in case.points:
            above = q.tag.startswith("above")
            g = mc.glass_closed(q.d, ir, above)
            rec = orc.core_world_hit_mat(case.flat.arrays_ptr(), q.o, q.d)
            assert rec["mat"] == glass and rec["front_face"] == above and abs(rec["p"][0]) < 1e-12 and rec["p"][1] == 0.0
            for k in range(8):
                s = _both_scatter(orc, (case.b, case.flat), glass, q.o, q.d, rec["p"], rec["normal"], rec["front_face"], 1 + k)
                assert s["scattered"] and s["attenuation"] == (1.0, 1.0, 1.0)
                assert s["draws"] == (0 if g["tir"] else 1), (ir, q.tag, s)
                if abs(g["share"] - u[k]) < 1e-9:
                    continue
                reflects = g["tir"] or g["share"] > u[k]
                dx, dy = s["direction"][0], s["direction"][1]
                up = dy > 0
                assert up == (above == reflects), (ir, q.tag, k, s, g["share"], u[k])
                tan = g["tan_i"] if reflects else g["tan_t"]
                # (a refracted direction is 1 / cos^2 as sensitive as its sine: 1e-12 of that, far inside the strip's 1e-6)
                assert s["direction"][2] == 0.0 and abs(dx - float(tan) * abs(dy)) <= 1e-12 * (1.0 + float(tan) ** 2), (ir, q.tag, s)
                assert abs(dx * dx + dy * dy - 1.0) < 1e-12


def _probe_world(rtsr):
    b = rtsr.Builder(1)
    mats = dict(lambertian=b.lambertian((0.5, 0.25, 1.0)), mirror=b.metal((0.5, 0.25, 1.0), 0.0), fuzzy=b.metal((0.5, 0.25, 1.0), 0.3),
                clamped=b.metal((0.5, 0.25, 1.0), 1.7), negative=b.metal((0.5, 0.25, 1.0), -0.5), glass=b.dielectric(1.5), two=b.dielectric(2.0),
                diamond=b.dielectric(2.4), one=b.dielectric(1.0), tiny=b.dielectric(1e-310), infinite=b.dielectric(float("inf")),
                light=b.diffuse_light((1.0, 1.0, 1.0)))
    found = mc.threshold_direction()
    assert found is not None, "no direction and index give ratio * sin == 1 exactly"
    mats["exact"] = b.dielectric(found[1])
    objs = [b.sphere((3.0 * k, 0.0, 0.0), 1.0, m) for k, m in enumerate(mats.values())]
    mats["exact_ir"] = found[1]
    fog = b.constant_medium((0.25, 0.5, 1.0), 0.5, b.sphere((0.0, 10.0, 0.0), 1.0, mats["lambertian"]))
    world = b.hittable_list(objs + [fog])
    flat = b.flatten(world)
    mats["isotropic"] = flat.medium(len(objs))["material"]
    return b, flat, mats


def test_scatter_on_adversarial_records(rtsr, orc):
    """O1 == core on records no scene produces: a zero normal (the record of a medium) and a normal of length 2 under every
    material, incident directions of length 1e-3 and 7, indices whose reciprocal overflows.  And the closed verdicts:
      * a Metal on a zero normal does not scatter (dot = 0 is not > 0), a mirror returns the mirror direction and draws a whole
        sphere sample (a multiple of 3 uniforms) although fuzz is 0;
      * Isotropic returns its sphere sample un-normalised (|direction| < 1) and its albedo;
      * ir = 2 at the direction whose ratio * sin is EXACTLY 1 can still refract: one uniform is drawn (`> 1`, not `>= 1`);
      * a normal of length 2 (cos = 2 before the fmin) reflects with r0 as at cos = 1."""
    b, flat, mats = _probe_world(rtsr)
    dirs = [(0.0, -1.0, 0.0), (0.6, -0.8, 0.0), (0.0007, -0.0001, 0.0002), (6.9, -0.7, 0.4), (0.999, -0.04, 0.0)]
    normals = [(0.0, 1.0, 0.0), (0.0, 0.0, 0.0), (0.0, 2.0, 0.0), (0.6, 0.8, 0.0)]
    n = 0
    for name, m in mats.items():
        if name == "exact_ir":
            continue
        for d in dirs:
            for nrm in normals:
                for ff in (True, False):
                    for seed in range(1, 9):
                        s = _both_scatter(orc, (b, flat), m, (0.0, 1.0, 0.0), d, (0.0, 0.0, 0.0), nrm, ff, seed)
                        n += 1
                        if name in ("mirror", "fuzzy", "clamped", "negative"):
                            assert s["draws"] % 3 == 0 and s["draws"] >= 3
                            if nrm == (0.0, 0.0, 0.0) and name == "mirror":
                                assert not s["scattered"]
                        if name == "mirror" and nrm == (0.0, 1.0, 0.0):
                            L = np.sqrt(sum(x * x for x in d))
                            assert s["scattered"] and np.allclose(s["direction"], (d[0] / L, -d[1] / L, d[2] / L), rtol=0, atol=1e-15)
                            assert s["attenuation"] == (0.5, 0.25, 1.0)
                        if name == "isotropic":
                            assert s["scattered"] and 0.0 < sum(x * x for x in s["direction"]) < 1.0 and s["attenuation"] == (0.25, 0.5, 1.0)
                        if name == "light":
                            assert not s["scattered"] and s["draws"] == 0
    print("\n[material cases] %d adversarial scatter probes, O1 == core" % n)
    # exactly at the critical angle
    d, ir, sin = mc.threshold_direction()
    assert ir == mats["exact_ir"] and ir * sin == 1.0
    refracted = 0
    for seed in range(1, 17):
        s = _both_scatter(orc, (b, flat), mats["exact"], (0.0, -1.0, 0.0), d, (0.0, 0.0, 0.0), (0.0, -1.0, 0.0), False, seed)
        assert s["draws"] == 1, s
        refracted += s["direction"][1] > 0
    assert refracted >= 8   # r0 and (1 - cos)^5 are small: most streams refract, along the surface (sin_t = 1)
    # cos = 2 before the fmin: reflect with probability r0(2.4) = 0.1696 over 64 streams, never with probability 2 r0 - 1 < 0
    u = mc.first_uniforms(orc, 1, 64)
    r0 = ((1.0 - 1.0 / 2.4) / (1.0 + 1.0 / 2.4)) ** 2
    for k in range(64):
        s = _both_scatter(orc, (b, flat), mats["diamond"], (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 0.0), (0.0, 2.0, 0.0), True, 1 + k)
        if abs(u[k] - r0) > 1e-9:
            assert (s["direction"][1] > 0) == (r0 > u[k]), (k, s, u[k])
    assert (u < r0).sum() >= 4


# ---- casts ---------------------------------------------------------------------------------------------------------------
def test_casts_equal_their_restatement_and_closed_verdicts(rtsr, orc):
    case = mc.build(rtsr, "casts")
    records = mc.cast_records(orc, case)
    lines, failed = [], []
    for cs in case.extra["sets"]:
        hit, t = records[cs.tag]
        u = mc.first_uniforms(orc, mc.SEED + cs.first, cs.n)
        want_hit, want_t, t1, t2 = mc.medium_hit_restated(orc, cs, u)
        assert np.array_equal(hit, want_hit) and _same(t, want_t), (cs.tag, int((hit != want_hit).sum()))
        if cs.verdict == "never":
            assert not hit.any(), cs.tag
        if cs.verdict == "at_t1":
            assert hit.all() and (t == t1).all() and t1[0] == 2.0, cs.tag
        if hit.any() and cs.density > 0:
            lo, hi = max(t1[0], cs.t_min, 0.0), min(t2[0], cs.t_max)
            assert (t[hit] >= lo).all() and (t[hit] <= hi).all(), (cs.tag, t[hit].min(), t[hit].max(), lo, hi)
        if cs.share is not None:
            se = np.sqrt(cs.share * (1.0 - cs.share) / cs.n)
            z = abs(hit.mean() - cs.share) / se
            lines.append("casts %s: closed form %.6f, core %.6f, %.2f standard errors, relative SE %.4f" % (cs.tag, cs.share, hit.mean(), z, mc.rel_se(cs.share, cs.n)))
            if not z <= mc.Z_CAP or not mc.rel_se(cs.share, cs.n) <= mc.REL_SE_CAP:
                failed.append(lines[-1])
        if cs.tag == "density -1":
            # hits BEFORE t1, as the reference does: t = t1 + log(u) / |d| with the project's log, which is numpy's to 2 ulps
            assert hit.all() and (t < t1).all() and _same(t, 2.0 + orc.rt_math("log", u) / 1.0)
            assert (np.abs(orc.rt_math("log", u) - np.log(u)) <= 2.0 * np.spacing(np.abs(np.log(u)))).all()
        if cs.tag == "negative t_min, origin inside":
            assert (t[hit] >= 0.0).all() and t1[0] == 0.0
        if cs.tag == "16 bins":
            bins = np.bincount(mc.truncated_bins(t[hit], t1[0], t2[0], cs.density * abs(cs.dx)), minlength=16)
            n = int(hit.sum())
            se = np.sqrt(n * (1.0 / 16.0) * (15.0 / 16.0))
            assert mc.rel_se(1.0 / 16.0, n) <= mc.REL_SE_CAP
            z = np.abs(bins - n / 16.0) / se
            lines.append("casts 16 bins of %d hits: counts %s, max %.2f standard errors" % (n, bins.tolist(), z.max()))
            if not z.max() <= mc.Z_CAP:
                failed.append(lines[-1])
    print("\n[material cases] " + "\n[material cases] ".join(lines))
    assert not failed, failed


def test_cast_exactly_at_the_far_end(rtsr, orc):
    """hit_distance == distance_inside_boundary exactly is a hit (`>`, not `>=`): on the slab [-1, 1] of density 1.25 from x = -3
    (rec2.t = 4) a stream whose distance d = 0.8 |log u| lies in [1, 2) on the grid of 2^-51 makes 4 - d and 4 - (4 - d) exact, so
    t_min = 4 - d puts the draw exactly on the far end: the hit is at t = 4."""
    case = mc.build(rtsr, "casts")
    cs = [s for s in case.extra["sets"] if s.tag == "16 bins"][0]
    o, d = cs.rays()
    u = mc.first_uniforms(orc, 1000, 512)
    dist = (np.float64(-1.0) / np.float64(1.25)) * orc.rt_math("log", u)
    found = 0
    for k in range(512):
        t_min = 4.0 - dist[k]
        if not (1.0 <= dist[k] < 2.0 and 4.0 - t_min == dist[k] and t_min + dist[k] == 4.0):
            continue
        found += 1
        rec = orc.core_world_hit(case.flat.arrays_ptr(), o[0], d[0], 0.0, t_min, float("inf"), rng_seed=1000 + k)
        assert rec is not None and rec["t"] == 4.0, (k, rec)
        rec = orc.core_world_hit(case.flat.arrays_ptr(), o[0], d[0], 0.0, float(np.nextafter(t_min, 5.0)), float("inf"), rng_seed=1000 + k)
        assert rec is None, (k, rec)
    assert found >= 3


def test_float_core_keeps_a_medium_whose_boundary_is_far_in_t(rtsr, orc):
    """Found by these cases: a float absorbs the 0.0001 of the second boundary query from |t| = 2048 on, the query returned the
    entry face again and the float build never saw the medium -- a direction of length 0.001 nine units away, or a slab 3000
    units away.  The float build now starts the second query at the next float (geometry.hpp: medium_second_t_min); its hit
    share is the closed form's again.  The double build keeps the reference's expression."""
    b = rtsr.Builder(1)
    skin = b.lambertian((0.5, 0.5, 0.5))
    world = b.hittable_list([b.constant_medium(mc.WHITE, 1.5, b.rect_prism((-0.5, -5.0, -5.0), (0.5, 5.0, 5.0), skin)),
                             b.constant_medium(mc.WHITE, 1.5, b.rect_prism((3000.0, -5.0, -5.0), (3001.0, 5.0, 5.0), skin))])
    flat = b.flatten(world)
    want = 1.0 - np.exp(-1.5)
    n = 4096
    for o, d, tag in (((-10.0, 0.25, 0.125), (1e-3, 0.0, 0.0), "|d| = 1e-3"), ((-10.0, 0.25, 0.125), (1.0, 0.0, 0.0), "|d| = 1"),
                      ((2990.0, 0.25, 0.125), (-1.0, 0.0, 0.0), "towards the near slab from 3000 away"), ((0.0, 0.25, 0.125), (-1.0, 0.0, 0.0), "from inside")):
        for f32 in (True, False):
            probe = orc.core32_world_hit if f32 else orc.core_world_hit
            hits = sum(probe(flat.arrays_ptr(), o, d, rng_seed=s) is not None for s in range(1, n + 1))
            # (a ray towards +x crosses both slabs: the second one's boundary is 3e6 away in t at |d| = 1e-3)
            p = 1.0 - np.exp(-3.0) if d[0] > 0 else (want if tag != "from inside" else 1.0 - np.exp(-1.5 * (0.5 - 0.001)))
            z = abs(hits / n - p) / np.sqrt(p * (1.0 - p) / n)
            print("[material cases] %s %s: closed form %.4f, core %.4f, %.2f standard errors" % ("float" if f32 else "double", tag, p, hits / n, z))
            assert z <= mc.Z_CAP, (tag, f32, hits / n, p)


@pytest.mark.parametrize("b_first", [False, True])
def test_two_media_first_scatter_shares(rtsr, orc, b_first):
    """2^18 casts along the axis, ray r on the stream of seed + r: which medium scatters the ray first, from the material of
    the hit, against the two exponentials under the reference's rule (the earlier slot draws first)."""
    case = mc.build(rtsr, "two_media", b_first=b_first)
    ma, mb = case.flat.medium(case.extra["slot_a"])["material"], case.flat.medium(case.extra["slot_b"])["material"]
    n = mc.N_SAMPLES
    ptr, q = case.flat.arrays_ptr(), case.points[0]
    mats = np.array([(orc.core_world_hit_mat(ptr, q.o, q.d, rng_seed=mc.SEED + r) or {"mat": -1})["mat"] for r in range(n)])
    args = (mc.TWO["rho_a"], 4.0, 8.0, mc.TWO["rho_b"], 7.0, 10.0)
    want = mc.later_first_shares(*args) if b_first else mc.two_media_shares(*args)
    got = ((mats == ma).mean(), (mats == mb).mean(), (mats == -1).mean())
    for who, w, g in zip(("A", "B", "neither"), want, got):
        z = abs(g - w) / np.sqrt(w * (1.0 - w) / n)
        assert mc.rel_se(w, n) <= mc.REL_SE_CAP
        print("[material cases] two media, %s first: %s closed form %.6f, core %.6f, %.2f standard errors" % ("B" if b_first else "A", who, w, g, z))
        assert z <= mc.Z_CAP


# ---- frames --------------------------------------------------------------------------------------------------------------
def _frames_equal(rtsr, orc, b, world, flat, cam, cfg):
    h = rtsr.image_height(cfg)
    a1, r1 = orc.o1_render(b.graph_ptr(), world, cam, cfg, h, threads=8)
    a2, r2 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=8)
    assert np.array_equal(a1, a2, equal_nan=True) and np.array_equal(r1, r2)
    return a2


@pytest.mark.parametrize("name,variant", mc.LIST_WORLDS + [("glass_balls", {}), ("metal_fuzz", {"edited": True}), ("pair", {"kind": "same", "extra": "instance"}),
                                                           ("media_general", {"extra": "bvh"}), ("media_sphere", {"extra": "gravity"})], ids=mc.case_id)
def test_small_frames_o1_equals_o2(rtsr, orc, name, variant):
    """Every case runs to completion through both CPU walks before a device sees it, and they agree bit for bit."""
    case = mc.build(rtsr, name, **variant)
    if variant.get("edited"):
        # O1 reads the graph, which set_shading does not touch: the edited flat scene equals the one built with the values
        plain = mc.build(rtsr, name)
        h = rtsr.image_height(case.cfg)
        a, _ = orc.o2_render(case.flat.arrays_ptr(), case.cam, case.cfg, h, threads=8)
        b, _ = orc.o2_render(plain.flat.arrays_ptr(), plain.cam, plain.cfg, h, threads=8)
        assert np.array_equal(a, b)
        return
    if variant.get("extra") == "instance":
        # The literal restatement has no instance trees (the reference has none; tests/test_instance_tree.py gives O1 the hoisted
        # graph): O1 is asked for the world with the tree's two members written out as plain list entries, and must equal O2
        # of the instanced world -- an instance tree IS the list of its members.
        hoisted = mc.build(rtsr, name, **dict(variant, extra="hoisted"))
        h = rtsr.image_height(case.cfg)
        a1, r1 = orc.o1_render(hoisted.b.graph_ptr(), hoisted.world, hoisted.cam, hoisted.cfg, h, threads=8)
        a2, r2 = orc.o2_render(case.flat.arrays_ptr(), case.cam, case.cfg, h, threads=8)
        assert np.array_equal(a1, a2) and np.array_equal(r1, r2) and a2.any()
        return
    a = _frames_equal(rtsr, orc, case.b, case.world, case.flat, case.cam, case.cfg)
    assert np.isfinite(a).all() and a.any()


@pytest.mark.parametrize("what", ["density", "ir"])
def test_nan_density_and_nan_index_here_only(rtsr, orc, what):
    """rtx_constant_medium and rtx_dielectric accept a NaN as the reference does; O1 == O2 with NaN equal to NaN.  Not GPU
    cases."""
    b = rtsr.Builder(2)
    nan = float("nan")
    skin = b.lambertian((0.5, 0.5, 0.5))
    objs = [b.xz_rect(-20.0, 20.0, -20.0, 20.0, -1.0, b.lambertian((0.8, 0.6, 0.4)))]
    if what == "density":
        objs.append(b.constant_medium((0.9, 0.9, 0.9), nan, b.sphere((0.0, 0.5, 0.0), 1.5, skin)))
    else:
        objs.append(b.sphere((0.0, 0.5, 0.0), 1.5, b.dielectric(nan)))
    world = b.hittable_list(objs)
    flat = b.flatten(world)
    cam = rtsr.Camera.new((0.0, 2.0, 6.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), 40.0, 1.5, 0.0, 10.0, 0.0, 1.0)
    cfg = rtsr.Config.new(1.5, 24, 4, 8, 4, seed=3, background=(0.7, 0.8, 1.0))
    _frames_equal(rtsr, orc, b, world, flat, cam, cfg)
