"""numpy f64 restatement of the denoising rule of include/rtx_abi.h (rtx_progressive_denoise / rtx_device_denoise).

Arrays are rows x width x 3 in the frame layout.  The device runs the levels in f32; this restatement runs everything in
f64, so the two agree to f32 rounding, not bit for bit.  The steps and their order follow the header.
"""
import numpy as np

H = np.array([1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16])
LUM = np.array([0.2126, 0.7152, 0.0722])
DEFAULTS = dict(iterations=5, feature_spp=4, demodulate=1, sigma_luminance=4.0, sigma_normal=32.0, sigma_albedo=0.3)
ALBEDO_FLOOR = float(np.float32(1e-3))  # max(A, 1e-3) is taken on the f32 albedo


def rule(**params):
    """The parameters with 0 (or absent) replaced by the defaults."""
    r = dict(DEFAULTS)
    for k, v in params.items():
        if v:
            r[k] = v
    r["demodulate"] = r["demodulate"] >= 0
    return r


def mean_var(S, Q, n):
    """m = S/n and the variance of the mean v = max(0, (Q - S*S/n)/(n - 1))/n, per pixel and channel; n: a count or one per
    pixel (rows x width).  Every operation is correctly rounded, as on the device."""
    n = np.asarray(n, dtype=np.float64)
    if n.ndim == 2:
        n = n[..., None]
    m = S / n
    var = (Q - S * S / n) / (n - 1.0)
    var = np.where(var > 0.0, var, 0.0)
    return m, var / n


def prepare(mean, var, albedo, normal, demodulate=True):
    """-> (c0, sigma2, n^, a): the demodulated colour, the luminance variance, the unit normal (0 where |N| < 1e-3) and the
    albedo factor a (ones without demodulation)."""
    A = np.asarray(albedo, dtype=np.float64)
    a = np.maximum(A, ALBEDO_FLOOR) if demodulate else np.ones_like(A)
    c0 = mean / a
    v = var / (a * a)
    sigma2 = (LUM * LUM * v).sum(axis=-1)
    N = np.asarray(normal, dtype=np.float64)
    length = np.sqrt((N * N).sum(axis=-1))
    nhat = np.where((length >= 1e-3)[..., None], N / np.where(length > 0, length, 1.0)[..., None], 0.0)
    return c0, sigma2, nhat, a


def level(c, sigma2, A, nhat, t, sigma_l, sigma_n, sigma_a):
    """One a-trous level at step t -> (c', sigma2')."""
    h, w = sigma2.shape
    A = np.asarray(A, dtype=np.float64)
    Y, X = np.mgrid[0:h, 0:w]
    lum = c @ LUM
    has_n = np.any(nhat != 0.0, axis=-1)
    denom = sigma_l * np.sqrt(sigma2) + 1e-4
    sw = np.zeros((h, w))
    sc = np.zeros((h, w, 3))
    sv = np.zeros((h, w))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            qy, qx = Y + t * dy, X + t * dx
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            dA = A - A[qy, qx]
            e = -np.abs(lum - lum[qy, qx]) / denom - (dA * dA).sum(axis=-1) / (sigma_a * sigma_a)
            d = (nhat * nhat[qy, qx]).sum(axis=-1)
            hq = has_n[qy, qx]
            wn = np.where(has_n & hq, np.clip(d, 0.0, 1.0) ** sigma_n, np.where(has_n == hq, 1.0, 0.0))
            wt = np.where(inside, H[dy + 2] * H[dx + 2] * np.exp(e) * wn, 0.0)
            if dx == 0 and dy == 0:  # p itself: e = 0 and W_n = 1 exactly
                wt = np.full((h, w), H[2] * H[2])
            sw += wt
            sc += wt[..., None] * c[qy, qx]
            sv += wt * wt * sigma2[qy, qx]
    return sc / sw[..., None], sv / (sw * sw)


def denoise(mean, var, albedo, normal, levels_out=None, **params):
    """The whole filter -> the denoised mean (rows x width x 3).  levels_out, a list, gets (c, sigma2) of the prepared input
    and of every level."""
    r = rule(**params)
    c, s2, nhat, a = prepare(mean, var, albedo, normal, r["demodulate"])
    if levels_out is not None:
        levels_out.append((c, s2))
    for k in range(r["iterations"]):
        c, s2 = level(c, s2, albedo, nhat, 2 ** k, r["sigma_luminance"], r["sigma_normal"], r["sigma_albedo"])
        if levels_out is not None:
            levels_out.append((c, s2))
    return c * a


def tone_map(mean):
    """rt::tone_map(mean, 1): sqrt, clamp to [0, 1], * 255.9, truncated (NaN -> 0)."""
    x = 255.9 * np.clip(np.sqrt(mean), 0.0, 1.0)
    return np.nan_to_num(x, nan=0.0).astype(np.int32).astype(np.uint8)
