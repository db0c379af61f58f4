"""Adaptive sampling on the GPU: a pixel that stopped at n_p samples holds the bits of a uniform render at n_p spp, and the
stopping rule restated in numpy on uniform snapshots gives exactly the library's per-pixel counts."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_progressive import SPLIT_CASES, _noise_tree, _rel_err, _setup, _with

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "ray-tracing-series-rust_amd", "lib", "rtx_render")


def _snapshots(scene, cam, cfg, steps, shard=None):
    """A uniform handle's (S, Q, rgb8) after each of the sample counts steps add up to: {spp: (S, Q, rgb8)}."""
    ref = scene.progressive(cam, cfg, shard=shard)
    snaps = {}
    for n in steps:
        ref.add(n)
        S, Q = ref.moments()
        snaps[ref.spp_done] = (S, Q, ref.screen(want_accum=False).rgb8)
    del ref
    return snaps


def _boundaries(start, batch, budget):
    out, k = [], start
    while k < budget:
        k = min(k + batch, budget)
        out.append(k)
    return out


def _walk(snaps, checks, min_spp, target, rows_active=None):
    """The rule of rtx_abi.h restated on uniform snapshots.  checks: spp_done at every retirement opportunity in order (the
    start of each round, then the final check of until_adaptive at the budget); a check runs when spp_done >= max(2,
    min_spp).  -> (n_p per pixel with 0 on rows never rendered, spp_done at the end, pixels still active)."""
    shape = next(iter(snaps.values()))[0].shape[:2]
    counts = np.zeros(shape, dtype=np.int32)
    active = np.zeros(shape, dtype=bool)
    active[:shape[0] if rows_active is None else rows_active] = True
    done = 0
    for spp in checks:
        done = spp
        if spp >= max(2, min_spp):
            S, Q, _ = snaps[spp]
            retire = active & (_rel_err(S, Q, spp) <= target)
            counts[retire] = spp
            active &= ~retire
        if not active.any():
            break
    counts[active] = done
    return counts, done, int(active.sum())


def _expected_until(snaps, start, batch, budget, min_spp, target, rows_active=None):
    """until_adaptive from spp_done = start: a check at the start, at every batch boundary and at the budget."""
    return _walk(snaps, [start] + _boundaries(start, batch, budget), min_spp, target, rows_active)


def _own(snaps, counts, k):
    """Plane k of the snapshot each pixel's own count selects (zeros where the count is 0)."""
    ref = next(iter(snaps.values()))[k]
    out = np.zeros_like(ref)
    for spp, snap in snaps.items():
        sel = counts == spp
        out[sel] = snap[k][sel]
    return out


def _own_rel_err(snaps, counts):
    r = np.zeros(counts.shape)
    for spp, (S, Q, _) in snaps.items():
        if spp >= 2:
            sel = counts == spp
            r[sel] = _rel_err(S, Q, spp)[sel]
    return r


def _check_frame(prog, snaps, counts, what=""):
    assert np.array_equal(prog.pixel_spp(), counts), what
    S, Q = prog.moments()
    assert np.array_equal(S, _own(snaps, counts, 0)), "%s: S differs in %d pixels" % (what, int((S != _own(snaps, counts, 0)).any(axis=2).sum()))
    assert np.array_equal(Q, _own(snaps, counts, 1)), what
    assert np.array_equal(prog.screen(want_accum=False).rgb8, _own(snaps, counts, 2)), what


def _check_stats(st, snaps, counts, done, n_active, min_spp, target):
    r = _own_rel_err(snaps, counts)[counts > 0]
    assert (st.spp_done, st.min_spp, st.pixels, st.target_rel_err) == (done, min_spp, r.size, target)
    assert st.pixels_active == n_active
    assert st.pixels_above == int((r > target).sum())
    assert st.samples == int(counts.sum())
    assert st.max_rel_err == r.max()
    assert st.mean_rel_err == _noise_tree(r, target).sum / r.size


def _median_target(snaps, spp):
    S, Q, _ = snaps[spp]
    return float(np.median(_rel_err(S, Q, spp)))


@pytest.mark.parametrize("name,sid,width,aspect,opts", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_adaptive_pixels_equal_uniform_snapshots(rtsr, name, sid, width, aspect, opts):
    budget, batch, min_spp = 24, 4, 6
    b, flat, scene, cam, cfg = _setup(rtsr, sid, width, aspect, budget, opts)
    kernel = scene.render_device(cam, cfg, want_stats=True).trace_kernel
    snaps = _snapshots(scene, cam, cfg, [batch] * (budget // batch))
    target = _median_target(snaps, 8)  # the first check at or past min_spp is at 8
    counts, done, n_active = _expected_until(snaps, 0, batch, budget, min_spp, target)
    retired = int((counts < done).sum())
    assert 0 < retired < counts.size, (name, retired)
    # round by round through add_adaptive: every round after the first retirement traces the listed pixels only
    prog = scene.progressive(cam, cfg)
    while prog.spp_done < budget:
        st = prog.add_adaptive(batch, min_spp, target, want_stats=True)
        n_p = prog.pixel_spp()
        active = int((n_p == prog.spp_done).sum())
        assert st.samples == batch * active, name
        if active:
            assert st.trace_kernel == kernel, (rtsr.trace_kernel_name(st.trace_kernel), rtsr.trace_kernel_name(kernel))
    fin = prog.until_adaptive(batch, min_spp, target)  # at the budget: the final check only
    assert prog.spp_done == fin.spp_done == done
    _check_frame(prog, snaps, counts, name)
    _check_stats(fin, snaps, counts, done, n_active, min_spp, target)
    assert fin.pixels_above == fin.pixels_active
    # the same in one call, twice: identical counts, sums and stats bytes; a repeated call changes nothing
    runs = []
    for _ in range(2):
        p2 = scene.progressive(cam, cfg)
        st2 = p2.until_adaptive(batch, min_spp, target)
        assert bytes(st2) == bytes(fin)
        assert bytes(p2.until_adaptive(batch, min_spp, target)) == bytes(st2)
        runs.append((p2.pixel_spp(), p2.moments()[0]))
        del p2
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert np.array_equal(runs[0][0], counts)


def test_rgb8_equals_one_shot_renders_at_each_count(rtsr):
    budget, batch = 16, 4
    b, flat, scene, cam, cfg = _setup(rtsr, 100, 40, 1.5, budget)
    snaps = _snapshots(scene, cam, cfg, [batch] * 4)
    target = _median_target(snaps, 4)
    prog = scene.progressive(cam, cfg)
    prog.until_adaptive(batch, 2, target)
    counts = prog.pixel_spp()
    got = prog.screen()
    assert len(np.unique(counts)) > 1
    for k in np.unique(counts):
        one = scene.render(cam, _with(rtsr, cfg, samples_per_pixel=int(k)))
        sel = counts == k
        assert np.array_equal(got.rgb8[sel], one.rgb8[sel]) and np.array_equal(got.accum[sel], one.accum[sel]), k


@pytest.mark.parametrize("variant", ["simple", "wavefront", "f32", "small_buffer"])
def test_adaptive_variants(rtsr, monkeypatch, variant):
    budget, batch, min_spp = 24, 4, 4
    if variant in ("simple", "wavefront"):
        monkeypatch.setenv("RTX_TRACE_KERNEL", variant)
    b, flat, scene, cam, cfg = _setup(rtsr, 100, 48, 1.5, budget, f32=variant == "f32")
    if variant == "small_buffer":  # one sample of every pixel: a round of 4 takes several passes (pipelined two deep once
        cfg = _with(rtsr, cfg, sample_buffer_bytes=24 * 48 * 32)  # at most half of the pixels are left, without stats)
    kernel = scene.render_device(cam, cfg, want_stats=True).trace_kernel
    if variant in ("simple", "wavefront"):
        assert rtsr.trace_kernel_name(kernel) == {"simple": "k_trace_simple", "wavefront": "k_wf_trace"}[variant]
    snaps = _snapshots(scene, cam, cfg, [batch] * (budget // batch))
    target = _median_target(snaps, 4)
    counts, done, n_active = _expected_until(snaps, 0, batch, budget, min_spp, target)
    assert 0 < int((counts < done).sum()) < counts.size
    prog = scene.progressive(cam, cfg)
    prog.add_adaptive(batch, min_spp, target)
    st = prog.add_adaptive(batch, min_spp, target, want_stats=True)  # the first round with pixels retired
    assert st.trace_kernel == kernel and 0 < st.samples < batch * counts.size
    if variant == "small_buffer":
        assert st.passes > 1
    fin = prog.until_adaptive(batch, min_spp, target)
    _check_frame(prog, snaps, counts, variant)
    _check_stats(fin, snaps, counts, done, n_active, min_spp, target)


def test_add_adaptive_rounds_with_varying_n_and_target(rtsr):
    b, flat, scene, cam, cfg = _setup(rtsr, 5, 32, 1.0, 40)  # cornell smoke: k_trace_world
    plan = [(3, None), (2, 0.5), (5, 0.3), (4, 0.7), (6, 0.2), (8, 0.6), (12, 0.0)]  # (n, target: a quantile of active r)
    snaps = _snapshots(scene, cam, cfg, [n for n, _ in plan])
    min_spp = 4
    prog = scene.progressive(cam, cfg)
    h = next(iter(snaps.values()))[0].shape[0]
    counts = np.zeros((h, 32), dtype=np.int32)
    active = np.ones((h, 32), dtype=bool)
    spp = 0
    for n, q in plan:
        target = 0.1  # (no check before min_spp)
        if spp >= min_spp:
            target = float(np.quantile(_rel_err(snaps[spp][0], snaps[spp][1], spp)[active], q))
            retire = active & (_rel_err(snaps[spp][0], snaps[spp][1], spp) <= target)
            counts[retire] = spp
            active &= ~retire
        prog.add_adaptive(n, min_spp, target)
        spp += n
        expect = counts.copy()
        expect[active] = spp
        _check_frame(prog, snaps, expect, "after %d" % spp)
    assert 0 < int((counts > 0).sum()) < counts.size


def test_oracle_link(rtsr, orc):
    b, flat, scene, cam, cfg = _setup(rtsr, 4, 8, 8.0 / 6.0, 16)  # cornell box: lit and dark pixels
    h = rtsr.image_height(cfg)
    snaps = _snapshots(scene, cam, cfg, [2] * 8)
    target = _median_target(snaps, 2)
    prog = scene.progressive(cam, cfg)
    prog.until_adaptive(2, 2, target)
    counts = prog.pixel_spp()
    assert 0 < int((counts < 16).sum()) < counts.size
    S, Q = prog.moments()
    for j in range(h):
        for i in range(8):
            s, q = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
            for k in range(int(counts[j, i])):
                x = orc.o2_sample(flat.arrays_ptr(), cam, cfg, h, i, j, k)
                for c in range(3):
                    xc = float(x[c])
                    s[c] = s[c] + xc
                    q[c] = q[c] + xc * xc
            assert list(S[j, i]) == s and list(Q[j, i]) == q, (i, j, int(counts[j, i]))


def test_shard_with_row_chunk_compat(rtsr):
    b, flat, scene, cam, cfg = _setup(rtsr, 100, 40, 1.0, 16, threads=16)
    cfg.row_chunk_compat = 1  # rows 32..39 are never rendered
    shard = (1, 3, 2)
    h = rtsr.image_height(cfg)
    rows = [j for j in range(h) if (j // 2) % 3 == 1]
    rows_active = sum(1 for j in rows if j < 32)
    assert rows_active < len(rows)
    snaps = _snapshots(scene, cam, cfg, [4] * 4, shard=shard)
    S4, Q4, _ = snaps[4]
    target = float(np.median(_rel_err(S4[:rows_active], Q4[:rows_active], 4)))
    counts, done, n_active = _expected_until(snaps, 0, 4, 16, 2, target, rows_active)
    prog = scene.progressive(cam, cfg, shard=shard)
    st = prog.until_adaptive(4, 2, target)
    assert counts[rows_active:].sum() == 0 and 0 < int((counts[:rows_active] < done).sum()) < rows_active * 40
    _check_frame(prog, snaps, counts, "shard")
    S, Q = prog.moments()
    assert not S[rows_active:].any() and not Q[rows_active:].any()
    assert not prog.screen().rgb8[rows_active:].any()
    _check_stats(st, snaps, counts, done, n_active, 2, target)


def test_every_pixel_meets_the_target_at_the_first_check(rtsr):
    b, flat, scene, cam, cfg = _setup(rtsr, 100, 40, 1.5, 64)
    prog = scene.progressive(cam, cfg)
    st = prog.until_adaptive(4, 5, 1e9)  # first boundary at or past min_spp 5: 8
    npix = 40 * rtsr.image_height(cfg)
    assert (st.spp_done, prog.spp_done, st.pixels_active, st.pixels_above, st.samples) == (8, 8, 0, 0, npix * 8)
    assert (prog.pixel_spp() == 8).all()
    again = prog.until_adaptive(4, 5, 1e9)  # nothing active: returns without tracing
    assert prog.spp_done == 8 and bytes(again) == bytes(st)
    assert np.array_equal(prog.screen().accum, scene.render(cam, _with(rtsr, cfg, samples_per_pixel=8)).accum)


def test_target_zero_retires_only_pixels_without_variance(rtsr):
    b, flat, scene, cam, cfg = _setup(rtsr, 6, 32, 1.0, 16)  # book-2 final: a black sky
    snaps = _snapshots(scene, cam, cfg, [4] * 4)
    counts, done, n_active = _expected_until(snaps, 0, 4, 16, 2, 0.0)
    prog = scene.progressive(cam, cfg)
    st = prog.until_adaptive(4, 2, 0.0)
    _check_frame(prog, snaps, counts, "target 0")
    _check_stats(st, snaps, counts, done, n_active, 2, 0.0)
    r = _own_rel_err(snaps, counts)
    assert (r[counts < done] == 0.0).all()


def test_uniform_entries_after_a_retirement(rtsr):
    b, flat, scene, cam, cfg = _setup(rtsr, 100, 40, 1.5, 23)
    snaps = _snapshots(scene, cam, cfg, [3, 4, 4, 4, 4, 4])
    target = _median_target(snaps, 3)
    prog = scene.progressive(cam, cfg)
    prog.add(3)  # a uniform add first is allowed
    prog.add_adaptive(4, 2, target)  # the check at 3 retires about half of the pixels
    assert (prog.pixel_spp() == 3).any()
    with pytest.raises(rtsr.RtxError) as e:
        prog.add(1)
    assert e.value.status == rtsr.RTX_EINVAL and "retired" in str(e.value)
    with pytest.raises(rtsr.RtxError) as e:
        prog.until(4, target)
    assert e.value.status == rtsr.RTX_EINVAL
    prog.until_adaptive(4, 2, target)
    counts, done, _ = _walk(snaps, [3] + _boundaries(3, 4, 23), 2, target)
    assert done == 23 and prog.spp_done == 23
    _check_frame(prog, snaps, counts, "uniform then adaptive")
    st = prog.stats(target)  # each pixel at its own count
    r = _own_rel_err(snaps, counts)
    assert st.pixels_above == int((r > target).sum()) and st.max_rel_err == r.max()


def test_bad_arguments_on_a_live_handle(rtsr):
    b, flat, scene, cam, cfg = _setup(rtsr, 100, 16, 1.5, 8)
    prog = scene.progressive(cam, cfg)
    prog.add(2)
    for n, m, t in ((0, 2, 0.1), (-1, 2, 0.1), (7, 2, 0.1), (2, 1, 0.1), (2, 9, 0.1), (2, 2, -0.1), (2, 2, float("nan"))):
        with pytest.raises(rtsr.RtxError) as e:
            prog.add_adaptive(n, m, t)
        assert e.value.status == rtsr.RTX_EINVAL, (n, m, t)
    for batch, m, t in ((0, 2, 0.1), (4, 1, 0.1), (4, 9, 0.1), (4, 2, -1.0), (4, 2, float("nan"))):
        with pytest.raises(rtsr.RtxError) as e:
            prog.until_adaptive(batch, m, t)
        assert e.value.status == rtsr.RTX_EINVAL, (batch, m, t)
    assert prog.spp_done == 2 and (prog.pixel_spp() == 2).all()
    prog.add(1)  # still a uniform handle


def test_app_adaptive_equals_python(rtsr, tmp_path):
    assert os.path.exists(APP), "apps/rtx_render was not built (python __graft_entry__.py)"
    b, flat, scene, cam, cfg = _setup(rtsr, 100, 48, 1.5, 32, seed=1)
    snaps = _snapshots(scene, cam, cfg, [4, 4])
    target = _median_target(snaps, 8)
    prog = scene.progressive(cam, cfg)
    st = prog.until_adaptive(4, 8, target)
    prog.screen().write_to_ppm_file(str(tmp_path / "py.ppm"))
    counts = prog.pixel_spp()
    assert 0 < int((counts < st.spp_done).sum()) < counts.size
    cmd = [APP, "--scene", "100", "--width", "48", "--aspect", "1.5", "--depth", "50", "--threads", "10", "--seed", "1",
           "--spp", "32", "--batch", "4", "--target-error", repr(target), "--adaptive", "--min-spp", "8",
           "--out", str(tmp_path / "app.ppm"), "--spp-map", str(tmp_path / "app.pgm")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr
    assert (tmp_path / "app.ppm").read_bytes() == (tmp_path / "py.ppm").read_bytes()
    tok = (tmp_path / "app.pgm").read_text().split()
    assert tok[:4] == ["P2", "48", str(counts.shape[0]), "32"]
    pgm = np.array([int(x) for x in tok[4:]], dtype=np.int32).reshape(counts.shape)
    assert np.array_equal(pgm[::-1], counts)  # top row first
    assert "samples traced" in res.stderr and str(st.samples) in res.stderr
