"""The kernels of next-event estimation on the scenes of tests/light_cases.py: k_trace_rays (with light sampling and plain)
and k_trace_nee equal their host checkers bit for bit on every case -- light tables of four entries, a pmf-0 entry, a textured
light, a vertex inside a light, none of which a catalogue scene has -- and the device's own sums meet the conditions of
tests/test_light_cases.py (whose docstring quotes the measured figures: the sums are the host checker's, bit for bit)."""
import numpy as np
import pytest

import light_cases as lc
import trace_rays_cases as tc

pytestmark = pytest.mark.gpu
NAMES = list(lc.CASES)


@pytest.fixture(scope="module")
def chk(orc, tmp_path_factory):
    return tc.checkers(tmp_path_factory)


@pytest.fixture(scope="module")
def nee_chk(tmp_path_factory):
    return lc.nee_checker(tmp_path_factory)


_scenes = {}


def _scene(rtsr, name):
    if name not in _scenes:
        b, flat = lc.CASES[name].build(rtsr)
        _scenes[name] = (b, flat, flat.upload())
    return _scenes[name]


def _device_tracer(scene):
    def trace(o, d, spp, max_depth, light_sampling):
        r = scene.trace_rays(np.ascontiguousarray(o), np.ascontiguousarray(d), spp=spp, max_depth=max_depth, background=(0, 0, 0),
                             seed=lc.SEED, light_sampling=light_sampling, sumsq=True)
        return r.sum, r.sumsq
    return trace


@pytest.mark.parametrize("name", NAMES)
def test_trace_rays_equals_the_host_checker(rtsr, chk, name):
    c = lc.CASES[name]
    b, flat, scene = _scene(rtsr, name)
    o, d = lc.replicated(*c.rays(), 4)
    ao, ad, _ = c.aimed_rays()
    o, d = np.concatenate([o, ao]), np.concatenate([d, ad])
    dev, host = _device_tracer(scene), lc.host_tracer(chk, flat)
    for depth in (1, 2, 50):
        for nee in (True, False):
            (S, Q), (Sh, Qh) = dev(o, d, 64, depth, nee), host(o, d, 64, depth, nee)
            bad = ~(tc.same_bits(S, Sh) & tc.same_bits(Q, Qh))
            assert not bad.any(), (name, depth, nee, int(bad.sum()))


@pytest.mark.parametrize("name", NAMES)
def test_trace_nee_frames_equal_the_host_checker(rtsr, nee_chk, name):
    b, flat, scene = _scene(rtsr, name)
    cam = lc.frame_camera(rtsr)
    for depth in (1, 2, 50):
        cfg = rtsr.Config.new(1.0, lc.FRAME_WIDTH, lc.FRAME_SPP, depth, 4, seed=lc.FRAME_SEED, background=(0.0, 0.0, 0.0))
        h = rtsr.image_height(cfg)
        gpu = scene.render(cam, cfg, light_sampling=True, want_stats=True)
        assert gpu.stats.trace_kernel == 8 and rtsr.trace_kernel_name(gpu.stats.trace_kernel) == "k_trace_nee"
        host = lc.host_frame(nee_chk, flat, cam, h, depth)
        assert np.array_equal(gpu.accum, host), (name, depth, int((gpu.accum != host).any(axis=2).sum()))
        assert depth == 1 or host.any()


@pytest.mark.parametrize("name", NAMES)
def test_device_sums_against_the_expected_radiance(rtsr, name):
    """tests/test_light_cases.py's two conditions on the device's own sums at the full sample count."""
    lines, failed = lc.statistical_check(lc.CASES[name], _device_tracer(_scene(rtsr, name)[2]))
    print("\n".join(lines))
    assert not failed, failed


@pytest.mark.parametrize("name", NAMES)
def test_exact_sums_on_the_device(rtsr, name):
    failed = lc.exact_check(lc.CASES[name], _device_tracer(_scene(rtsr, name)[2]))
    assert not failed, failed
