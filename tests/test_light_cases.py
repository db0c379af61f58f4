"""Next-event estimation with MIS against closed forms, on the CPU: the f64 host checker of radiance queries
(tests/rays_host_check.cpp, the bit-equal twin of k_trace_rays) traced on the scenes of tests/light_cases.py with light
sampling and without, at max_depth 2 and 50, and held to expected radiances that share nothing with csrc/.

The two conditions are met by the unmodified checker on the streams chosen in light_cases.py (seed 1, 2^18 samples per point,
2^19 for the half shadows, 2^20 for light_in_front).  Measured, light sampling / plain, the same at both depths (a path ends
at the light or in the black background either way):

    case                     max z         max relative SE
    xz                       2.20 / 2.63   0.0011 / 0.036
    xy                       2.36 / 2.83   0.0013 / 0.043
    yz_through_floor         3.23 / 2.06   0.0026 / 0.049
    sphere                   2.00 / 1.79   0.0003 / 0.029
    multi                    1.98 / 2.83   0.0032 / 0.026
    light_in_front           2.16 / 1.60   0.0035 / 0.0041
    all_zero_weights         2.44 / 1.82   0.0031 / 0.035
    image_rect               3.15 / 2.78   0.0029 / 0.058
    half_shadow_translated   2.09 / 1.80   0.0036 / 0.058
    half_shadow_top_level    2.09 / 1.80   0.0036 / 0.058
    unsampled                2.63 / 2.63   (an empty table: the plain estimator, 0.036)
    sphere_on_horizon        1.84 / 2.02   0.0019 / 0.053
    sphere_axes              1.47 / 1.66   0.0023 / 0.045
    image_sphere             2.46 (both depths), light sampling against plain in combined standard errors
    fog_vertex               2.08 (depth 2), 2.09 (depth 50), light sampling against plain in combined standard errors

scripts/mutate_light_sampling.py seeds thirteen single-line faults in the estimator and runs these comparisons on each
(profiles/light_sampling/mutations.txt)."""
import numpy as np
import pytest

import light_cases as lc
import trace_rays_cases as tc

NAMES = list(lc.CASES)


@pytest.fixture(scope="module")
def chk(orc, tmp_path_factory):
    return tc.checkers(tmp_path_factory)


_scenes = {}


def _tracer(rtsr, chk, name):
    if name not in _scenes:
        b, flat = lc.CASES[name].build(rtsr)
        _scenes[name] = (b, flat, lc.host_tracer(chk, flat))
    return _scenes[name][2]


def test_expected_values_stand_on_their_own():
    """The closed forms against each other and against textbook values; the recorded quadrature order."""
    p = np.array([0.3, 0.0, -0.2])
    # a disc-like check of Lambert's formula: a square of side 2a at height h straight overhead, against its own closed form
    # E / Le = 4 * a / sqrt(a^2 + h^2) * atan(a / sqrt(a^2 + h^2))
    a, h = 0.7, 1.3
    sq = lc.rect_vertices("xz", p[0] - a, p[0] + a, p[2] - a, p[2] + a, h)
    s = np.sqrt(a * a + h * h)
    assert abs(lc.polygon_form(sq, p) - 4 * a / s * np.arctan(a / s)) < 1e-14
    # a vertical rectangle cut by the floor plane equals its upper part
    whole, upper = lc.rect_vertices("yz", -1, 2, -1, 1.5, -4), lc.rect_vertices("yz", 0, 2, -1, 1.5, -4)
    assert abs(lc.polygon_form(whole, p) - lc.polygon_form(upper, p)) < 1e-15
    # the quadrature reproduces pi (r / d)^2 cos(theta) for a sphere clear of the horizon ...
    c, r = np.array([0.5, 2.5, 0.2]), 0.8
    for x, z in lc.POINTS:
        q = np.array([x, 0.0, z])
        assert abs(lc.cone_irradiance(c, r, q, lc.HORIZON_ORDER) / lc.sphere_form(c, r, q) - 1) < 1e-12
    # ... a sphere centred on the floor plane far away sends half of that with cos(theta) -> 4 r / (3 pi d) of the disc
    # (the upper half disc seen edge-on): E / Le -> (2 / 3) (r / d)^3 to first order
    far = lc.cone_irradiance(np.array([0.0, 0.0, 0.0]), 1.0, np.array([400.0, 0.0, 0.0]), lc.HORIZON_ORDER)
    assert abs(far / ((2.0 / 3.0) * (1.0 / 400.0) ** 3) - 1) < 1e-4
    # ... and the recorded order is the one at which doubling moves no point by 1e-7
    H = lc.HORIZON_SPHERE
    pts = [np.array([x, 0.0, z]) for x, z in lc.POINTS]
    found = lc.horizon_order(H["c"], H["r"], pts)
    print("sphere_on_horizon: order %d and its double agree to 1e-7; the double, %d, is used" % (found, lc.HORIZON_ORDER))
    assert 2 * found == lc.HORIZON_ORDER
    for q in pts:
        assert np.linalg.norm(H["c"] - q) > H["r"]
    # the texel mapping: (u, v) = (0.5, 0.5) reads row 1, column 1
    assert lc.texel_of(0.5, 0.5) == (1, 1) and lc.texel_of(0.25, 0.75) == (0, 0) and lc.texel_of(1.0, 0.0) == (1, 1)


@pytest.mark.parametrize("name", NAMES)
def test_light_table(rtsr, name):
    c = lc.CASES[name]
    b, flat = c.build(rtsr)
    got, want = flat.lights(), c.census()
    for k in ("n_lights", "n_rect_lights", "n_sphere_lights", "n_unsampled_emitters"):
        assert got[k] == want[k], (k, got, want)
    assert abs(got["total_area"] - want["total_area"]) <= 1e-12 * max(1.0, want["total_area"])


@pytest.mark.parametrize("name", NAMES)
def test_estimators_against_the_expected_radiance(rtsr, chk, name):
    """Every point and channel within 4.5 standard errors at max_depth 2 and 50, both estimators; light sampling's relative
    standard error <= 0.5 % (a 3 % bias then stands beyond 6 sigma, and light sampling cannot have decayed to the material's
    own sampling, whose relative SE is 3 - 8 %)."""
    lines, failed = lc.statistical_check(lc.CASES[name], _tracer(rtsr, chk, name))
    print("\n".join(lines))
    assert not failed, failed


@pytest.mark.parametrize("name", NAMES)
def test_exact_sums(rtsr, chk, name):
    """max_depth 1: floor rays exactly 0, rays aimed at each light exactly Le; inside_sphere exactly RHO * Le; an empty table
    changes nothing -- all by bit pattern."""
    failed = lc.exact_check(lc.CASES[name], _tracer(rtsr, chk, name))
    assert not failed, failed


def test_light_draw_at_exact_cdf_values(rtsr, tmp_path):
    """nee_connect on streams whose first draw is set to a cdf entry, one grid step under it, 0 and the largest draw."""
    failed = lc.pick_check(rtsr, lc.pick_checker(tmp_path))
    assert not failed, failed
