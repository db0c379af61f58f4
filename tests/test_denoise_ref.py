"""Properties of the numpy restatement of the denoising rule (tests/denoise_ref.py), without a GPU."""
import numpy as np

import denoise_ref as dr


def _inputs(h, w, seed=0):
    g = np.random.default_rng(seed)
    mean = g.uniform(0.0, 2.0, (h, w, 3))
    var = g.uniform(1e-4, 1e-2, (h, w, 3))
    albedo = g.uniform(0.1, 0.9, (h, w, 3)).astype(np.float32)
    normal = g.normal(size=(h, w, 3)).astype(np.float32)
    return mean, var, albedo, normal


def test_constant_image_stays_constant():
    h, w = 9, 13
    _, var, _, _ = _inputs(h, w)
    mean = np.broadcast_to([0.3, 0.5, 0.7], (h, w, 3)).copy()
    albedo = np.broadcast_to(np.float32([0.6, 0.4, 0.2]), (h, w, 3)).copy()
    normal = np.broadcast_to(np.float32([0.0, 0.0, 1.0]), (h, w, 3)).copy()
    out = dr.denoise(mean, var, albedo, normal, iterations=4)
    np.testing.assert_allclose(out, mean, rtol=1e-12, atol=0)


def test_a_normal_step_edge_is_never_crossed():
    h, w = 8, 16
    _, var, _, _ = _inputs(h, w, 1)
    albedo = np.full((h, w, 3), 0.5, dtype=np.float32)
    normal = np.zeros((h, w, 3), dtype=np.float32)
    normal[:, :8] = (0.0, 0.0, 1.0)
    normal[:, 8:] = (1.0, 0.0, 0.0)  # W_n = max(0, 0)^sigma_n = 0 across the edge
    mean = np.zeros((h, w, 3))
    mean[:, :8] = 1.0
    levels = []
    out = dr.denoise(mean, var, albedo, normal, levels_out=levels, iterations=5)
    assert np.all(out[:, 8:] == 0.0)
    np.testing.assert_allclose(out[:, :8], 1.0, rtol=1e-12)
    for c, _ in levels:
        assert np.all(c[:, 8:] == 0.0)
    # a zero normal next to a nonzero one is an edge too
    normal[:, 8:] = 0.0
    out = dr.denoise(mean, var, albedo, normal, iterations=5)
    assert np.all(out[:, 8:] == 0.0)


def test_one_pixel_comes_back_unchanged():
    mean, var, albedo, normal = _inputs(1, 1, 2)
    for demodulate in (1, -1):
        out = dr.denoise(mean, var, albedo, normal, iterations=8, demodulate=demodulate)
        np.testing.assert_allclose(out, mean, rtol=2 ** -23)


def test_variance_never_rises_on_a_constant_variance_field():
    h, w = 12, 17
    mean, _, albedo, normal = _inputs(h, w, 3)
    var = np.full((h, w, 3), 4e-3)
    levels = []
    dr.denoise(mean, var, albedo, normal, levels_out=levels, iterations=6, demodulate=-1)
    for (_, before), (_, after) in zip(levels, levels[1:]):
        assert np.all(after <= before * (1 + 1e-12))


def test_defaults_and_mean_var():
    r = dr.rule()
    assert (r["iterations"], r["feature_spp"], r["sigma_luminance"], r["sigma_normal"], r["sigma_albedo"]) == (5, 4, 4.0, 32.0, 0.3)
    assert r["demodulate"] and not dr.rule(demodulate=-1)["demodulate"] and dr.rule(demodulate=1)["demodulate"]
    S = np.array([[[4.0, 2.0, 0.0]]])
    Q = np.array([[[6.0, 1.0, 0.0]]])
    m, v = dr.mean_var(S, Q, 4)
    assert np.array_equal(m, [[[1.0, 0.5, 0.0]]])
    assert np.array_equal(v, [[[(6.0 - 4.0) / 3.0 / 4.0, 0.0, 0.0]]])  # (1 - 4/4) / 3 = 0 in the middle channel
