"""The host checker, scenes, points and closed forms of tests/test_gather_abi.py and tests/test_gpu_gather.py (a helper module,
not a test file): everything here runs on the CPU, and everything that is expected of a gather is written in numpy alone.

The judge is tests/gather_host_check.cpp built with oracle/Makefile's CXXFLAGS: once as it is (f64) and once with
o2_flat_f32.cpp's four defines (the float judge, linked to liboracle.so for oracle_f32_images).

What is expected, and why:

  surface form, depth 1, background 0, a point of a plane that cannot see itself: a sample is Le where the start direction
  meets the light and 0 elsewhere, the direction is cosine distributed about the normal, so the mean is E / pi = Le * F with
  F = (E / Le) / pi the form factor -- light_cases.polygon_form and sphere_form return E / Le.

  probe form, depth 1, background 0, one sphere light of radiance Le whose centre lies in the unit direction d and which
  subtends the angular radius theta_m (c = cos theta_m): L(w) = Le inside the cap, 0 outside, and the projection of a cap onto
  a real spherical harmonic of degree l is Y_lm(d) * 2 pi * integral_c^1 P_l(t) dt:
      I_0 = 1 - c,   I_1 = (1 - c^2) / 2,   I_2 = (c - c^3) / 2.
  The coefficient estimate 4 pi * S / samples must equal Le * Y_lm(d) * 2 pi * I_l.

  Statistical acceptance: every value within Z_CAP = 4.5 standard errors computed from the returned sumsq (light_cases' bound).
  Sample counts: the rarest event of the plain estimator is the far corner point of the small light, hit with probability
  F ~ 5e-4 per sample; REPLICAS x SPP = 2^16 samples a point expect ~30 hits there, so a point without a hit (standard error
  0) does not occur and the normal approximation holds; every other case has more.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import cast_rays_cases as cc
import light_cases as lc
import trace_rays_cases as tc

ROOT = tc.ROOT
SRC = os.path.join(ROOT, "tests", "gather_host_check.cpp")

SEED = 1
BACKGROUND = (0.7, 0.8, 1.0)
POINTS, SPP, DEPTH = 500, 4, 8      # every bit-for-bit case: 500 points x 4 spp x depth 8
Z_CAP = lc.Z_CAP
REPLICAS, STAT_SPP = 16, 4096       # statistical cases: 2^16 samples a point (the module text says why)

_D = C.POINTER(C.c_double)
_ARGS = [C.c_void_p, C.c_int64, _D, _D, _D, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, _D, C.c_int32,
         C.c_int32, _D, _D]
_checkers = {}


def checkers(tmp_path_factory):
    """{False: the f64 judge's entry, True: the float judge's}, built once per session (needs liboracle.so: the orc fixture)."""
    if not _checkers:
        d = tmp_path_factory.mktemp("gather_host")
        out64, out32 = str(d / "gather_host_check.so"), str(d / "gather_host_check_f32.so")
        subprocess.run(["g++"] + tc.CXXFLAGS + ["-shared", SRC, "-o", out64], check=True)
        subprocess.run(["g++"] + tc.CXXFLAGS + ["-DGATHER_HOST_F32", "-shared", SRC, os.path.join(tc.ORACLE_BUILD, "liboracle.so"),
                        "-Wl,-rpath," + tc.ORACLE_BUILD, "-o", out32], check=True)
        for f32, path, name in ((False, out64, "gather_host_trace"), (True, out32, "gather_host_trace_f32")):
            fn = getattr(C.CDLL(path), name)
            fn.restype, fn.argtypes = C.c_int, _ARGS
            _checkers[f32] = fn
    return _checkers


def sum_shape(n, sh_order):
    return (n, 3) if sh_order == 0 else (n, (sh_order + 1) ** 2, 3)


def host_gather(chk, flat, p, normals=None, time=None, *, spp=SPP, max_depth=DEPTH, background=BACKGROUND, seed=SEED,
                first_sample=0, first_point=0, light_sampling=False, sh_order=0, f32=False, into=None):
    """The judge's (sum, sumsq) of a batch; into=(S, Q): continue those sums in place (accumulate)."""
    n = len(p)
    cont = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    p, normals, time = cont(p), cont(normals), cont(time)
    S, Q = into if into is not None else (np.zeros(sum_shape(n, sh_order)), np.zeros(sum_shape(n, sh_order)))
    bg = np.array(background, dtype=np.float64)
    ptr = lambda a: a.ctypes.data_as(_D) if a is not None else None
    rc = chk[f32](flat.arrays_ptr(), n, ptr(p), ptr(normals), ptr(time), first_point, first_sample, spp, max_depth,
                  1 if into is not None else 0, seed, ptr(bg), 1 if light_sampling else 0, sh_order, ptr(S), ptr(Q))
    assert rc == 0, rc
    return S, Q


def host_gatherer(chk, flat, threads=8):
    """gather(p, normals, spp, max_depth, light_sampling, sh_order) -> (sum, sumsq) by the f64 judge with background 0, the
    points cut into chunks traced side by side: point r keeps the stream of index r, so the sums are those of one call."""
    from concurrent.futures import ThreadPoolExecutor

    def gather(p, normals, spp, max_depth, light_sampling, sh_order=0):
        n = len(p)
        S, Q = np.zeros(sum_shape(n, sh_order)), np.zeros(sum_shape(n, sh_order))
        cuts = np.linspace(0, n, min(4 * threads, n) + 1).astype(int)

        def part(k):
            lo, hi = cuts[k], cuts[k + 1]
            S[lo:hi], Q[lo:hi] = host_gather(chk, flat, p[lo:hi], None if normals is None else normals[lo:hi], spp=spp,
                                             max_depth=max_depth, background=(0, 0, 0), first_point=int(lo),
                                             light_sampling=light_sampling, sh_order=sh_order)
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(part, range(len(cuts) - 1)))
        return S, Q
    return gather


def scene_gatherer(scene):
    """The same callable over Scene.gather (numpy arrays, the host entry)."""
    def gather(p, normals, spp, max_depth, light_sampling, sh_order=0):
        got = scene.gather(np.ascontiguousarray(p), None if normals is None else np.ascontiguousarray(normals), spp=spp,
                           max_depth=max_depth, background=(0.0, 0.0, 0.0), seed=SEED, light_sampling=light_sampling, sh_order=sh_order)
        return got.sum, got.sumsq
    return gather


def same_bits(a, b):
    return tc.same_bits(a, b)


# ---- the real spherical harmonics, restated (nothing here reads csrc/) ---------------------------------------------------------
def sh_basis(d):
    """Y (..., 9) of directions d (..., 3): the real orthonormal basis in the order (0,0), (1,-1), (1,0), (1,1), (2,-2) .. (2,2)."""
    d = np.asarray(d, dtype=np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    pi = np.pi
    return np.stack([
        np.full_like(x, 0.5 * np.sqrt(1.0 / pi)),
        np.sqrt(3.0 / (4.0 * pi)) * y, np.sqrt(3.0 / (4.0 * pi)) * z, np.sqrt(3.0 / (4.0 * pi)) * x,
        0.5 * np.sqrt(15.0 / pi) * x * y, 0.5 * np.sqrt(15.0 / pi) * y * z, 0.25 * np.sqrt(5.0 / pi) * (3.0 * z * z - 1.0),
        0.5 * np.sqrt(15.0 / pi) * x * z, 0.25 * np.sqrt(15.0 / pi) * (x * x - y * y)], axis=-1)


SH_DEGREE = np.array([0, 1, 1, 1, 2, 2, 2, 2, 2])


def sh_basis_in_stated_order(d, order):
    """Y (n, spp, K) with the literals and the order of operations the contract states (include/rtx_abi.h, core/sh_basis.hpp):
    the constant times the parenthesised polynomial.  numpy evaluates each elementwise operation separately rounded."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    Y = [np.full_like(x, 0.28209479177387814)]
    if order >= 1:
        Y += [0.4886025119029199 * y, 0.4886025119029199 * z, 0.4886025119029199 * x]
    if order >= 2:
        Y += [1.0925484305920792 * (x * y), 1.0925484305920792 * (y * z), 0.31539156525252005 * (3.0 * (z * z) - 1.0),
              1.0925484305920792 * (x * z), 0.5462742152960396 * (x * x - y * y)]
    return np.stack(Y, axis=-1)


def sh_sums_in_stated_order(d, L, order):
    """(S, Q) (n, K, 3) from directions d (n, spp, 3) and radiances L (n, spp, 3): for s ascending v = Y_i(dir_s) * L_s[c];
    S += v; Q += v * v."""
    Y = sh_basis_in_stated_order(d, order)
    n, spp, K = Y.shape
    S, Q = np.zeros((n, K, 3)), np.zeros((n, K, 3))
    for s in range(spp):
        v = Y[:, s, :, None] * L[:, s, None, :]
        S = S + v
        Q = Q + v * v
    return S, Q


def cap_coefficients(le, d, cos_max, order=2):
    """(K, 3): Le * Y_lm(d) * 2 pi * I_l of a cap of radiance le around the unit direction d."""
    c = cos_max
    I = np.array([1.0 - c, 0.5 * (1.0 - c * c), 0.5 * (c - c ** 3)])
    K = (order + 1) ** 2
    return (sh_basis(d)[:K] * 2.0 * np.pi * I[SH_DEGREE[:K]])[:, None] * np.asarray(le, dtype=np.float64)[None, :]


# ---- statistics --------------------------------------------------------------------------------------------------------------
def mean_and_se(S, Q, spp, n_points):
    """Per point (and coefficient) and channel: the mean and its standard error over all replicas' samples, from the per-index
    sums; index = replica * n_points + point."""
    S = np.asarray(S, dtype=np.float64)
    S3, Q3 = S.reshape((-1, n_points) + S.shape[1:]), np.asarray(Q, dtype=np.float64).reshape((-1, n_points) + S.shape[1:])
    n = spp * S3.shape[0]
    s, q = S3.sum(axis=0), Q3.sum(axis=0)
    return s / n, np.sqrt(np.maximum(q - s * s / n, 0.0) / (n - 1) / n)


# ---- closed forms of the surface form: light_cases' floor, its lights, its 16 points ------------------------------------------
SMALL_LIGHT = lc.Case("small_sphere", [lc.SMALL_SPHERE])
SURFACE_CASES = {"xz": lc.CASES["xz"], "sphere": lc.CASES["sphere"], "small_sphere": SMALL_LIGHT}
FLOOR_POINTS = np.array([[x, 0.0, z] for x, z in lc.POINTS])


def surface_expected(case):
    """(16, 3): Le * F, F = (E / Le) / pi."""
    out = np.zeros((len(FLOOR_POINTS), 3))
    for L in case.lights:
        for k, p in enumerate(FLOOR_POINTS):
            form = lc.sphere_form(L["c"], L["r"], p) if L["kind"] == "sphere" else lc.polygon_form(lc.rect_vertices(L["kind"], *L["ab"], L["k"]), p)
            out[k] += L["le"] * form / np.pi
    return out


def surface_check(name, gather):
    """Both estimators at depth 1 against Le * F -> (lines, failed conditions).  small_sphere also: light sampling's standard
    error is below the plain estimator's at every point and channel."""
    case = SURFACE_CASES[name]
    ex = surface_expected(case)
    p = np.tile(FLOOR_POINTS, (REPLICAS, 1))
    nrm = np.tile(lc.N_UP, (len(p), 1))
    lines, failed, se = [], [], {}
    for nee in (False, True):
        m, e = mean_and_se(*gather(p, nrm, STAT_SPP, 1, nee), STAT_SPP, len(FLOOR_POINTS))
        z = lc.z_scores(m, e, ex)
        se[nee] = e
        lines.append("%s, light sampling %d: max z %.2f, max relative SE %.4f" % (name, nee, z.max(), (e / ex).max()))
        if not z.max() <= Z_CAP:
            k = np.unravel_index(np.argmax(z), z.shape)
            failed.append("%s light sampling %d: z %.2f at point %d channel %d (%.6g, expected %.6g)" % (name, nee, z.max(), k[0], k[1], m[k], ex[k]))
        if not (m > 0).all():
            failed.append("%s light sampling %d: a point without light" % (name, nee))
    if name == "small_sphere":
        lines.append("small_sphere: SE light sampling / plain, max %.4f" % (se[True] / se[False]).max())
        if not (se[True] < se[False]).all():
            failed.append("small_sphere: light sampling's standard error is not below the plain estimator's everywhere")
    return lines, failed


# ---- closed form of the probe form: one sphere light, probes around it ----------------------------------------------------------
PROBE_LE = np.array([4.0, 3.0, 2.0])
PROBE_LIGHT_C, PROBE_LIGHT_R = np.array([0.6, 1.7, -0.9]), 1.1
PROBES = np.array([[2.0, 0.3, 0.7], [-1.5, 3.1, -2.2], [0.2, -1.0, 1.4], [1.9, 2.8, -3.0]])


def probe_scene(rtsr):
    b = rtsr.Builder(1)
    lst = b.hittable_list()
    b.list_add(lst, b.sphere(tuple(PROBE_LIGHT_C), PROBE_LIGHT_R, b.diffuse_light(tuple(PROBE_LE))))
    return b, b.flatten(lst)


def probe_expected():
    """(4, 9, 3)."""
    out = []
    for p in PROBES:
        oc = PROBE_LIGHT_C - p
        dist = np.linalg.norm(oc)
        assert dist > 1.5 * PROBE_LIGHT_R
        out.append(cap_coefficients(PROBE_LE, oc / dist, np.sqrt(1.0 - (PROBE_LIGHT_R / dist) ** 2)))
    return np.array(out)


def probe_check(gather):
    """Both estimators, order 2, depth 1: the coefficient estimates 4 pi * mean against the cap's -> (lines, failed)."""
    ex = probe_expected()
    p = np.tile(PROBES, (REPLICAS, 1))
    lines, failed = [], []
    for nee in (False, True):
        m, e = mean_and_se(*gather(p, None, STAT_SPP, 1, nee, 2), STAT_SPP, len(PROBES))
        z = lc.z_scores(4.0 * np.pi * m, 4.0 * np.pi * e, ex)
        lines.append("probe, light sampling %d: max z %.2f" % (nee, z.max()))
        if not z.max() <= Z_CAP:
            k = np.unravel_index(np.argmax(z), z.shape)
            failed.append("probe light sampling %d: z %.2f at probe %d coefficient %d channel %d (%.6g, expected %.6g)"
                          % (nee, z.max(), k[0], k[1], k[2], 4.0 * np.pi * m[k], ex[k]))
        if not (e > 0).all():
            failed.append("probe light sampling %d: a coefficient without spread" % nee)
    return lines, failed


# ---- the identity with trace_rays: media-free scenes over a WHITE Lambertian floor ---------------------------------------------
def white_floor_scene(rtsr, kind):
    """kind: "rect_light", "sphere_light", "metal_glass" -> (builder, flat).  The floor is y = 0, solid_color (1, 1, 1)."""
    b = rtsr.Builder(1)
    lst = b.hittable_list()
    b.list_add(lst, b.xz_rect(-50, 50, -50, 50, 0.0, b.lambertian((1.0, 1.0, 1.0))))
    if kind == "rect_light":
        b.list_add(lst, b.xz_rect(-1, 1, -0.5, 1.5, 2.0, b.diffuse_light((4.0, 3.0, 2.0))))
        b.list_add(lst, b.sphere((-1.5, 0.6, 0.4), 0.6, b.lambertian((0.7, 0.3, 0.2))))
    elif kind == "sphere_light":
        b.list_add(lst, b.sphere((0.5, 2.5, 0.2), 0.8, b.diffuse_light((4.0, 3.0, 2.0))))
        b.list_add(lst, b.rect_prism((1.0, 0.0, -1.5), (2.0, 1.2, -0.5), b.lambertian((0.2, 0.6, 0.8))))
    else:
        b.list_add(lst, b.sphere((-1.2, 0.7, 0.3), 0.7, b.metal((0.8, 0.7, 0.5), 0.1)))
        b.list_add(lst, b.sphere((1.3, 0.8, -0.4), 0.8, b.dielectric(1.5)))
        b.list_add(lst, b.sphere((1.3, 0.8, -0.4), -0.7, b.dielectric(1.5)))
        b.list_add(lst, b.yz_rect(0.2, 2.0, -1.0, 1.0, -3.0, b.diffuse_light((6.0, 5.0, 1.0))))
    return b, b.flatten(lst)


def floor_rays(n, seed=31):
    """n rays from above the floor, tilted downwards, so that most of them meet the floor first."""
    rng = np.random.default_rng(seed)
    o = np.column_stack([rng.uniform(-3.5, 3.5, n), rng.uniform(2.6, 4.0, n), rng.uniform(-3.5, 3.5, n)])
    target = np.column_stack([rng.uniform(-4.0, 4.0, n), np.zeros(n), rng.uniform(-4.0, 4.0, n)])
    return np.ascontiguousarray(o), np.ascontiguousarray(target - o)


# ---- points of the bit-for-bit cases: the first hits of tests/trace_rays_cases.py's rays -----------------------------------------
def points_of(c, n=POINTS):
    """(p, normals, times) of case c (trace_rays_cases.case): the oracle's hit point and normal where ray r hits, the ray's origin
    and its reversed direction where it misses; normals scaled by 0.5, 1 or 1.5 (they are taken as given)."""
    rec = c.first_hits[:n]
    hit = rec[:, 0] == 1.0
    p = np.where(hit[:, None], rec[:, 2:5], c.o[:n])
    nrm = np.where(hit[:, None], rec[:, 5:8], -c.d[:n]) * (0.5 + 0.5 * (np.arange(n) % 3))[:, None]
    return np.ascontiguousarray(p), np.ascontiguousarray(nrm), np.ascontiguousarray(c.time[:n])
