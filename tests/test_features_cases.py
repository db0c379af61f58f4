"""The host checker of the feature pass (tests/features_host_check.cpp) and its case table (tests/features_cases.py), proved
on the CPU alone: the checker against the analytic sphere model, against the oracle's own ray query (code that does not share
its pixel loop), the float twin against the f64 build, and every case's conditions -- enough pixels whose samples disagree,
all hit and all miss, both colours of a medium, several values of a texture -- from the checker's `hits` and albedo."""
import numpy as np
import pytest

import features_cases as fc

NAMES = list(fc.CASES)
MEDIA_CASES = ("box_media", "book2", "sphere_media")


@pytest.fixture(scope="module")
def chk(orc, tmp_path_factory):
    return fc.checkers(tmp_path_factory)


def test_the_cases_cover_what_they_must(rtsr):
    cases = [fc.case(rtsr, n) for n in NAMES]
    assert {c.spp for c in cases} == {1, 3, 4, 64}
    assert all(c.cfg.image_width <= 64 and c.cfg.image_width * c.height <= 48 * 40 for c in cases)
    assert any((c.cfg.image_width, c.height) == (33, 17) for c in cases) and any((c.cfg.image_width, c.height) == (64, 4) for c in cases)
    assert any(c.cam.lens_radius > 0.0 for c in cases) and any(c.cam.time1 < c.cam.time2 and c.flat.info()["n_moving_spheres"] > 0 for c in cases)
    info = {c.name: c.flat.info() for c in cases}
    assert info["mesh_room"]["n_triangles"] >= 1900 and info["mesh_room"]["n_bvh"] >= 1 and info["mesh_room"]["n_rects"] >= 6
    assert fc.case(rtsr, "zoo").flat.instances()["n_trees"] == 1
    assert fc.case(rtsr, "gravity").cam.time2 == fc.gravity_time_limit()
    assert set(fc.F32_EXACT) == {c.name for c in cases if c.f32_exact}


def test_checker_equals_the_analytic_sphere(rtsr, orc, chk):
    c = fc.case(rtsr, "one_sphere")
    center, radius, colour = c.sphere
    albedo, normal, hits = fc.reference(chk, rtsr, "one_sphere")
    ahits, nref = fc.analytic_features(rtsr, c.cam, c.cfg, center, radius, c.spp, stream=fc.oracle_stream(orc))
    assert np.array_equal(hits, ahits)
    # albedo exactly: (k colour + (spp - k) background) / spp in f64, summed in sample order -- per pixel, since the order of
    # hits and misses is the pixel's own; where every sample agrees the sum is spp equal terms
    bg = np.array(c.cfg.background[:])
    full, none = hits == c.spp, hits == 0
    assert full.sum() > 50 and none.sum() > 50
    assert np.array_equal(albedo[full], np.broadcast_to(colour, albedo[full].shape))
    assert np.array_equal(albedo[none], np.broadcast_to(np.float32(bg), albedo[none].shape))
    stream = fc.oracle_stream(orc)
    col64 = np.array([0.3, 0.6, 0.9])
    for j, i in np.argwhere(~full & ~none):
        total = np.zeros(3)
        for s in range(c.spp):
            o, d, _ = fc.primary_ray(stream, c.cam, c.cfg, c.height, i, j, s)
            oc = o - center
            disc = (oc @ d) ** 2 - (d @ d) * (oc @ oc - radius * radius)
            total = total + (col64 if disc >= 0 else bg)
        assert np.array_equal(albedo[j, i], np.float32(total * (1.0 / c.spp))), (j, i)
    assert np.abs(normal - nref).max() <= 1e-6
    assert not normal[none].any()


def test_only_media_cases_are_left_out_of_the_ray_query(rtsr):
    assert {n for n in NAMES if not fc.case(rtsr, n).ray_query} == set(MEDIA_CASES)
    assert all(fc.case(rtsr, n).media for n in MEDIA_CASES)


@pytest.mark.parametrize("name", [n for n in NAMES if n != "one_sphere" and n not in MEDIA_CASES])
def test_checker_agrees_with_the_oracles_ray_query(rtsr, orc, chk, name):
    """Each sample's primary ray rebuilt in numpy from the stream and the camera (lens and shutter included), cast through the
    oracle's world_hit: the hit counts equal the checker's and the averaged normals agree to 1e-6.  The three media cases are
    not here: a medium's free path is the next draw of the PATH's stream, and the oracle's probe starts a stream of its own,
    so the same ray scatters elsewhere or not at all.  The checker's position in the stream at that draw is therefore tied to
    the core's path_begin and world_hit alone, which it calls back to back as the integrator does."""
    c = fc.case(rtsr, name)
    assert c.ray_query
    albedo, normal, hits = fc.reference(chk, rtsr, name)
    stream = fc.oracle_stream(orc)
    ptr = c.flat.arrays_ptr()
    w = c.cfg.image_width
    spp = min(c.spp, 4)  # the first four samples of the 64-sample case, against the checker at 4
    if spp != c.spp:
        albedo, normal, hits = fc.reference(chk, rtsr, name, spp=spp)
    nsum, nhit = np.zeros((c.height, w, 3)), np.zeros((c.height, w), dtype=np.int32)
    for j in range(c.height):
        for i in range(w):
            for s in range(spp):
                o, d, time = fc.primary_ray(stream, c.cam, c.cfg, c.height, i, j, s)
                rec = orc.core_world_hit(ptr, tuple(o), tuple(d), float(time), 0.001, float("inf"))
                if rec is not None:
                    nhit[j, i] += 1
                    nsum[j, i] += rec["normal"]
    assert np.array_equal(nhit, hits)
    assert np.abs(nsum / spp - normal).max() <= 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_every_case_exercises_the_edges(rtsr, chk, name):
    c = fc.case(rtsr, name)
    albedo, normal, hits = fc.reference(chk, rtsr, name)
    partial, full, none = (hits > 0) & (hits < c.spp), hits == c.spp, hits == 0
    print("%s: %d x %d x %d spp: %d partial, %d full, %d none" % (name, c.cfg.image_width, c.height, c.spp, partial.sum(), full.sum(), none.sum()))
    assert full.sum() >= 20
    if c.spp > 1:
        assert partial.sum() >= 20
    if c.closed is None:
        assert none.sum() >= 20
    else:
        assert c.spp == 1 and none.sum() == 0, c.closed  # the reason holds
    assert not normal[none].any()
    if c.media:
        # sample 0 of every pixel alone (the checker at one sample), where an albedo is one colour: inside each window some
        # rays scatter in the medium (its colour, no normal) and some cross it and reach what lies behind (that colour, a normal)
        a1, n1, h1 = fc.reference(chk, rtsr, name, spp=1)
        for (j0, j1, i0, i1), medium, behind in c.media:
            win = (slice(j0, j1), slice(i0, i1))
            n_medium = int(((a1[win] == medium).all(axis=2) & (h1[win] == 1) & ~n1[win].any(axis=2)).sum())
            n_behind = int(((a1[win] == behind).all(axis=2) & n1[win].any(axis=2)).sum())
            print("  rows %d..%d, columns %d..%d: %d rays end in the medium, %d on what lies behind" % (j0, j1, i0, i1, n_medium, n_behind))
            assert n_medium >= 3 and n_behind >= 3
    if c.textured:
        # on sample 0 alone, where a pixel's albedo is one texture value and no mixture along an outline
        a1, _, h1 = fc.reference(chk, rtsr, name, spp=1)
        assert len(np.unique(a1[h1 == 1], axis=0)) >= 3


@pytest.mark.parametrize("name", fc.F32_EXACT)
def test_float_checker_stays_near_the_f64_checker(rtsr, chk, name):
    """The float judge is the same loop over the narrowed scene.  A sample can see something else in float only where it
    lies within float precision of an outline or of an edge between two faces: at most 2 % of the pixels may differ in their
    hit count, in albedo by more than 1e-6 (a few float roundings of a colour in [0, 1]) or in normal by more than 1e-3."""
    a64, n64, h64 = fc.reference(chk, rtsr, name)
    a32, n32, h32 = fc.reference(chk, rtsr, name, f32=True)
    assert (h64 != h32).mean() <= 0.02
    assert (np.abs(a32 - a64).max(axis=2) > 1e-6).mean() <= 0.02
    assert (np.abs(n32 - n64).max(axis=2) > 1e-3).mean() <= 0.02
    assert not n32[h32 == 0].any()


def test_large_frame_case_on_the_cpu(rtsr, chk):
    """The frame the GPU test builds for 256 compute units: just over 524 288 pixels, about a second of the checker."""
    c = fc.large_case(rtsr, 256)
    assert c.cfg.image_width * c.height > 256 * 8 * 256 and (c.cfg.image_width * c.height - 256 * 8 * 256) <= 1024
    albedo, normal, hits = fc.host_features(chk, c.flat, c.cam, c.cfg, c.height, 1)
    beyond = hits.reshape(-1)[256 * 8 * 256:]
    assert (hits == 1).sum() > 1000 and (hits == 0).sum() > 1000
    assert beyond.size >= 1 and np.isfinite(albedo).all() and albedo.reshape(-1, 3)[256 * 8 * 256:].any()
