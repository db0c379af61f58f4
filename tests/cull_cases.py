"""Boxes and rays whose exact relation is known, for the no-false-miss tests of the f32 culling code (core/cull32.hpp and the
wide step): tests/test_cull_conservative.py runs the host functions on them, tests/test_gpu_cull_steps.py the device's.

Every number is dyadic, so `fractions` can say exactly whether the closed box meets the ray within [t_min, t_max]:

  touch   a point p of the closed box -- a corner, the middle of an edge, a point of a face, an inner point -- and a direction
          d; the origin is o = p - 2^k d, kept only where that difference is exact in f64 (TwoSum leaves no error): the ray is
          at p at t = 2^k exactly.  t_min is 0.001 or half of that, t_max is inf or exactly 2^k, so the answer is "meets" by
          construction; `exact_meets` confirms it on a sample.
  near    the same with p pushed off the box by one ulp-sized step, which the exact test then classifies either way: the cases
          the culling efficiency is counted on.

f64 cases: box coordinates with 20-bit mantissas at 2^-10 .. 2^10, direction components with 12-bit mantissas at 2^-15 .. 2^15,
one in 16 of them +0.0 and one in 16 -0.0, k in -4 .. 8.  f32 cases (every number a float): 10-bit and 6-bit mantissas, k < 6.
Special classes: zero-thickness boxes, rays that start inside, origins 2^20 away from a box of size 2^-10, and slopes on either
side of make_ray32's finite_slope threshold on an axis whose touched plane is 0: components of 2^-99, 2^-100, 2^-101 in f64
(1 / d against 1e30) and 2^-59, 2^-60, 2^-61 under RT_F32 (1 / d below 2^60, equal to it and above it)."""
import os
import subprocess
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = ("may_hit", "nf", "nf_pos", "hit2_a", "hit2_b", "wide")  # verdict bits 0 .. 5; bit 6: nf_pos was asked (t_min > 0)
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:verify_asan_link_order=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}

INF = float("inf")


def _dyadic(rng, n, bits, e_lo, e_hi):
    m = rng.integers(1 << (bits - 1), 1 << bits, size=n).astype(np.float64)
    e = rng.integers(e_lo, e_hi + 1, size=n)
    return np.ldexp(m, e - bits) * rng.choice([-1.0, 1.0], size=n)


def _exact_difference(a, b):
    """a - b and whether it is exact (TwoSum's error term is zero)."""
    s = a - b
    bb = s - a
    err = (a - (s - bb)) + (-b - bb)
    return s, (err == 0.0) & np.isfinite(s)


def generate(n, f32, seed):
    """-> dict of arrays: box (m, 6), ray (m, 8) = origin, direction, t_min, t_max, kind (m,) int (0 corner, 1 edge, 2 face,
    3 inside, 4 zero thickness, 5 far origin, 6 slope threshold), touch (m,) bool (False: a `near` case), zero_on_plane (m,):
    an axis with a zero direction component whose origin lies exactly on one of the box's planes of that axis."""
    rng = np.random.default_rng(seed)
    bb, db, kmax = (10, 6, 5) if f32 else (20, 12, 8)
    a, b = _dyadic(rng, (n, 3), bb, -10, 10), _dyadic(rng, (n, 3), bb, -10, 10)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    kind = rng.integers(0, 4, size=n)
    thin = rng.random((n, 3)) < 1.0 / 16.0
    hi = np.where(thin, lo, hi)
    kind = np.where(thin.any(axis=1), 4, kind)
    far = rng.random(n) < 1.0 / 16.0  # a box of size 2^-10, the origin 2^20 away
    lo_far = _dyadic(rng, (n, 3), 10 if not f32 else 6, -6, -4)
    lo = np.where(far[:, None], lo_far, lo)
    hi = np.where(far[:, None], lo_far + 2.0 ** -10, hi)
    kind = np.where(far, 5, kind)
    # the touched point: per axis lo, hi or an inner dyadic point; `kind` says how many axes sit on a plane
    mid = 0.5 * (lo + hi)
    inner = mid + 0.25 * (hi - mid) * rng.choice([-1.0, 0.0, 1.0], size=(n, 3))
    plane = np.where(rng.random((n, 3)) < 0.5, lo, hi)
    n_on = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [3, 2, 1, 0], default=rng.integers(0, 4, size=n))
    order = np.argsort(rng.random((n, 3)), axis=1)  # which axes sit on a plane
    on = order < n_on[:, None]
    p = np.where(on, plane, inner)
    d = _dyadic(rng, (n, 3), db, -15, 15)
    d = np.where(far[:, None], _dyadic(rng, (n, 3), db, 10, 14), d)
    z = rng.random((n, 3))
    d = np.where(z < 1.0 / 16.0, 0.0, np.where(z < 2.0 / 16.0, -0.0, d))
    d[:, 0] = np.where(np.all(d == 0.0, axis=1), 1.0, d[:, 0])
    k = rng.integers(-4, kmax + 1, size=n)
    k = np.where(far, rng.integers(6, 9, size=n) if not f32 else 5, k)
    # slope thresholds: one axis whose touched plane is 0 and whose direction component is 2^-e around the threshold
    thr = rng.random(n) < 1.0 / 32.0
    ax = rng.integers(0, 3, size=n)
    exps = np.array([59, 60, 61] if f32 else [99, 100, 101])
    which = rng.integers(0, 3, size=n)
    tiny = np.ldexp(1.0, -exps[which]) * rng.choice([-1.0, 1.0], size=n)
    for axis in range(3):
        sel = thr & (ax == axis)
        side = rng.random(n) < 0.5  # the plane at 0 is the low or the high one
        lo[:, axis] = np.where(sel, np.where(side, 0.0, -np.abs(lo[:, axis]) - 1.0), lo[:, axis])
        hi[:, axis] = np.where(sel, np.where(side, np.abs(hi[:, axis]) + 1.0, 0.0), hi[:, axis])
        p[:, axis] = np.where(sel, 0.0, p[:, axis])
        d[:, axis] = np.where(sel, tiny, d[:, axis])
    kind = np.where(thr, 6, kind)
    # `near` cases: p moved off the box along one axis by a small dyadic step (half of them; the exact test classifies them)
    touch = rng.random(n) < 0.5
    step = np.ldexp(1.0, rng.integers(-24 if not f32 else -12, 3, size=n)) * np.maximum(np.abs(hi - lo).max(axis=1), 2.0 ** -10)
    axn = rng.integers(0, 3, size=n)
    outward = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    p_near = p.copy()
    rows = np.arange(n)
    p_near[rows, axn] = np.where(outward < 0, lo[rows, axn] - step, hi[rows, axn] + step)
    p = np.where((touch | thr)[:, None], p, p_near)
    touch = touch | thr
    s = np.ldexp(d, k[:, None])
    o, exact = _exact_difference(p, s)
    ok = exact.all(axis=1)
    if f32:
        allv = np.concatenate([lo, hi, o, d], axis=1)
        with np.errstate(over="ignore", under="ignore"):
            ok &= (allv.astype(np.float32).astype(np.float64) == allv).all(axis=1)
    hit_t = np.ldexp(1.0, k)
    t_min = np.where(rng.random(n) < 0.5, 0.001 if not f32 else float(np.float32(0.001)), 0.5 * hit_t)
    t_max = np.where(rng.random(n) < 0.5, INF, hit_t)
    box = np.concatenate([lo, hi], axis=1)[ok]
    ray = np.concatenate([o, d, t_min[:, None], t_max[:, None]], axis=1)[ok]
    zero_on_plane = ((ray[:, 3:6] == 0.0) & ((ray[:, 0:3] == box[:, 0:3]) | (ray[:, 0:3] == box[:, 3:6]))).any(axis=1)
    return {"box": box, "ray": ray, "kind": kind[ok], "touch": touch[ok], "zero_on_plane": zero_on_plane, "hit_t": hit_t[ok]}


def exact_meets(box, ray):
    """Does the closed box meet origin + t direction for some t in [t_min, t_max]?  Exact: `fractions` on the f64 inputs."""
    lo_t, hi_t = Fraction(ray[6]), (None if ray[7] == INF else Fraction(ray[7]))
    for a in range(3):
        lo, hi, o, d = Fraction(box[a]), Fraction(box[3 + a]), Fraction(ray[a]), Fraction(ray[3 + a])
        if d == 0:
            if not lo <= o <= hi:
                return False
            continue
        t0, t1 = (lo - o) / d, (hi - o) / d
        if t0 > t1:
            t0, t1 = t1, t0
        lo_t = max(lo_t, t0)
        hi_t = t1 if hi_t is None else min(hi_t, t1)
    return hi_t is None or lo_t <= hi_t


def build_host_check(directory, f32):
    """tests/wide_step_host_check.cpp under the sanitizers, in the f64 or the fast mode's arithmetic."""
    exe = os.path.join(str(directory), "wide_step_host_check" + ("_f32" if f32 else ""))
    if not os.path.exists(exe):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + (["-DRT_F32", "-DRT_REAL=float"] if f32 else []) +
                       [os.path.join(ROOT, "tests", "wide_step_host_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, mode, src, dst):
    out = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, env=dict(os.environ, **SAN_ENV), timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "wide step host check clean" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def host_verdicts(exe, directory, tag, box, ray):
    """-> (ray32 (n, 8) float32, key (n,) float32, verdict (n,) uint32) of the host functions."""
    src, dst = os.path.join(str(directory), tag + ".in"), os.path.join(str(directory), tag + ".out")
    with open(src, "wb") as f:
        f.write(np.array([len(box)], dtype="<i8").tobytes())
        f.write(np.ascontiguousarray(np.concatenate([box, ray], axis=1), dtype="<f8").tobytes())
    _run(exe, "verdicts", src, dst)
    raw = np.fromfile(dst, dtype=np.uint8).reshape(len(box), 40)
    return raw[:, :32].copy().view("<f4"), raw[:, 32:36].copy().view("<f4").reshape(-1), raw[:, 36:40].copy().view("<u4").reshape(-1)


def host_steps(exe, directory, tag, kind, bottom, levels, nodes, items):
    """-> (cur (n,), n (n,), slots (n, levels)) of the restated step; dead slots hold 0x0badf00d."""
    src, dst = os.path.join(str(directory), tag + ".in"), os.path.join(str(directory), tag + ".out")
    with open(src, "wb") as f:
        f.write(np.array([{"step32": 0, "step4": 1}[kind], 1 if bottom else 0, levels, len(nodes)], dtype="<i4").tobytes())
        f.write(np.array([len(items)], dtype="<i8").tobytes())
        f.write(np.ascontiguousarray(nodes).tobytes())
        f.write(np.ascontiguousarray(items).tobytes())
    _run(exe, "steps", src, dst)
    out = np.fromfile(dst, dtype="<i4").reshape(len(items), 2 + levels)
    return out[:, 0], out[:, 1], out[:, 2:]


def missing_bits(verdict):
    """Per case, the verdict bits that say "miss" (bit 2 only where it was asked)."""
    v = np.asarray(verdict, dtype=np.uint32)
    need = np.where(v & 64, 0b111111, 0b111011).astype(np.uint32)
    return need & ~v
