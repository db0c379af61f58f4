"""No false miss: the f32 box tests that let the walks skip subtrees (core/cull32.hpp: cull32_may_hit, _nf, _nf_pos, _may_hit2,
and the wide step's slab test) never say "miss" for a box the ray really meets.  The CPU half: the host side of those functions
(tests/wide_step_host_check.cpp, under ASan + UBSan) on the cases of tests/cull_cases.py, whose truth is exact -- dyadic
inputs, `fractions` as the judge.  tests/test_gpu_cull_steps.py asks the device the same questions.

The cap on exclusions is ZERO, with one class excepted and counted: RT_F32, a direction component of exactly 0 and the origin
exactly on a plane of that axis.  The fast mode gives such an axis a slope of 2^60 (make_ray32 says why), which puts that plane at
t = 0 instead of "inside for all t"; the float CPU oracle runs the same code.

A fast-mode component below 2^-60 that is not 0 (2^-61 in the slope-threshold class) used to fail it too, in every form: the
slope was clamped into +-2^60, which halved every plane distance of that axis -- 752 of 1 824 such touches were missed.
make_ray32 now replaces only a slope that is not finite.

A direction component of -0.0 (one in 16 here) used to fail this test in the forms that take their planes already picked:
`d < 0` is false for it while the slope 1 / d is -inf (or -2^60), and the "near" plane came out at +inf.  The pick now follows
the slope's sign (ray32_dir_neg).

Counts (seed 1): 1 453 953 f64 and 422 087 fast-mode cases with exact origins, 778 129 and 254 269 of which must be hit; the
judge confirms 8 000 touches and classifies 30 000 `near` cases in each mode.

Culling efficiency, recorded and not asserted: of the judged `near` cases the exact ray MISSES (the touched point pushed off the
box by 2^-24 .. 2^2 of its size), the share each form lets through (host, seed 1): f64 may_hit / hit2 43.6 %, nf 36.7 %, nf_pos
and wide 35.8 % -- the min / max forms also pass what a zero component turns into NaN; RT_F32 (coarser inputs, 2^60 in place
of an infinite slope) 2.6 % in every form."""
import numpy as np
import pytest

import cull_cases as cc

N = {False: 1500000, True: 1000000}  # generated; the exact-origin ones are kept (f64: almost all, about 2 / 5 of the floats)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("cull")


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_no_form_of_the_box_test_misses_a_box_the_ray_meets(workdir, f32):
    c = cc.generate(N[f32], f32, seed=1)
    n = len(c["box"])
    touch = c["touch"]
    print("%s: %d of %d cases kept (exact origins), %d touch; kinds %s; -0.0 components %d, +0.0 %d" % (
        "f32" if f32 else "f64", n, N[f32], int(touch.sum()), np.bincount(c["kind"], minlength=7).tolist(),
        int(((c["ray"][:, 3:6] == 0.0) & np.signbit(c["ray"][:, 3:6])).sum()), int(((c["ray"][:, 3:6] == 0.0) & ~np.signbit(c["ray"][:, 3:6])).sum())))
    assert n > N[f32] // 3 and touch.sum() > n // 3
    # (an origin 2^20 away from a box of size 2^-10 is no float: the fast mode's share of that class is what survives)
    assert all(cnt > 1000 for kd, cnt in enumerate(np.bincount(c["kind"], minlength=7)) if not (kd == 5 and f32))
    # the judge on a sample of the touch cases (they meet by construction) and on the first near cases
    idx_t = np.nonzero(touch)[0][::max(1, int(touch.sum()) // 8000)]
    assert all(cc.exact_meets(c["box"][i], c["ray"][i]) for i in idx_t)
    idx_n = np.nonzero(~touch)[0][:30000]
    meets_n = np.array([cc.exact_meets(c["box"][i], c["ray"][i]) for i in idx_n])
    exe = cc.build_host_check(workdir, f32)
    q, key, v = cc.host_verdicts(exe, workdir, "f32" if f32 else "f64", c["box"], c["ray"])
    assert (v & 64).astype(bool).all()  # every t_min here is positive: the nf_pos form is asked throughout
    miss = cc.missing_bits(v)
    must = touch.copy()
    must[idx_n[meets_n]] = True
    excepted = must & c["zero_on_plane"] if f32 else np.zeros(n, dtype=bool)
    bad = np.nonzero(must & ~excepted & (miss != 0))[0]
    print("must hit: %d; excepted class (f32, zero component, origin on a plane of its axis): %d, of which missed by some form: %d" % (
        int(must.sum()), int(excepted.sum()), int((excepted & (miss != 0)).sum())))
    for i in bad[:5]:
        print("FALSE MISS bits", [cc.BITS[b] for b in range(6) if miss[i] >> b & 1], "kind", c["kind"][i], "box", c["box"][i].tolist(), "ray", c["ray"][i].tolist(), "q", q[i].tolist())
    assert len(bad) == 0, "%d false misses" % len(bad)
    if not f32:
        assert not (c["zero_on_plane"] & must & (miss != 0)).any()
    # culling efficiency on the near cases the exact ray misses
    away = idx_n[~meets_n]
    print("near cases judged: %d, the exact ray misses %d; let through:" % (len(idx_n), len(away)),
          {cc.BITS[b]: "%.2f %%" % (100.0 * float((v[away] >> b & 1).mean())) for b in range(6)})
    assert len(away) > 1000
