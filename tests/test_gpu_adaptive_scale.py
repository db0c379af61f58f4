"""Adaptive and progressive rendering at real frame sizes, end to end through the C ABI: more than 256 blocks of active
pixels, so k_retire_scan gives each thread several blocks, k_noise_stats_final folds several partials per thread and the
trace kernels claim chunks of long compacted lists.  Every case is bit-exact against uniform snapshots (pixel_spp, S, Q,
rgb8) and its stats exact, mean_rel_err included (_noise_tree)."""
import numpy as np
import pytest

from test_gpu_adaptive import _check_frame, _check_stats, _expected_until, _own_rel_err, _snapshots
from test_gpu_progressive import _noise_tree, _rel_err, _setup, _with

pytestmark = pytest.mark.gpu

SCALE_CASES = [  # (name, scene id, width, aspect, options, budget, batch, min_spp, target spp, kernel, variant)
    ("book1_400", 100, 400, 1.5, {}, 16, 4, 4, 4, "k_trace_lds", None),
    ("book2_1000", 6, 1000, 1.0, {}, 8, 2, 2, 4, "k_trace_world", None),
    ("dragon_640", 11, 640, 16.0 / 9.0, {"mesh_triangles": 20000}, 16, 4, 4, 4, "k_trace_vote", None),
    ("book1_400_pipelined", 100, 400, 1.5, {}, 16, 4, 4, 4, "k_trace_lds", "pipelined"),
    ("book1_400_f32", 100, 400, 1.5, {}, 16, 4, 4, 4, "k_trace_lds", "f32"),
    ("book1_600_shard", 100, 600, 1.5, {}, 16, 4, 4, 4, "k_trace_lds", "shard"),
]


@pytest.mark.parametrize("name,sid,width,aspect,opts,budget,batch,min_spp,target_spp,kernel_name,variant", SCALE_CASES,
                         ids=[c[0] for c in SCALE_CASES])
def test_adaptive_at_frame_size(rtsr, name, sid, width, aspect, opts, budget, batch, min_spp, target_spp, kernel_name,
                                variant):
    shard = (1, 3, 2) if variant == "shard" else None
    threads = 11 if variant == "shard" else 10  # 400 rows in bands of 11: rows 396..399 are never rendered
    b, flat, scene, cam, cfg = _setup(rtsr, sid, width, aspect, budget, opts, f32=variant == "f32", threads=threads)
    if variant == "shard":
        cfg.row_chunk_compat = 1
    kernel = scene.render_device(cam, cfg, shard=shard, want_stats=True).trace_kernel
    assert rtsr.trace_kernel_name(kernel) == kernel_name
    snaps = _snapshots(scene, cam, cfg, [batch] * (budget // batch), shard=shard)
    rows = next(iter(snaps.values()))[0].shape[0]
    rows_active = rows
    if variant == "shard":
        h = rtsr.image_height(cfg)
        shard_rows = [j for j in range(h) if (j // 2) % 3 == 1]
        assert len(shard_rows) == rows
        rows_active = sum(1 for j in shard_rows if j < (h // threads) * threads)
        assert 0 < rows_active < rows
    npix = rows_active * width
    assert npix > 256 * 256  # more than 256 blocks
    S, Q, _ = snaps[target_spp]
    target = float(np.median(_rel_err(S[:rows_active], Q[:rows_active], target_spp)))
    counts, done, n_active = _expected_until(snaps, 0, batch, budget, min_spp, target, rows_active)
    assert 0 < int((counts[:rows_active] < done).sum()) < npix
    first_check = next(k for k in sorted(snaps) if k >= max(2, min_spp))
    r_first = _rel_err(*snaps[first_check][:2], first_check)[:rows_active]
    n_first = int((r_first > target).sum())  # pixels the round after the first check traces
    assert 0 < n_first < npix
    if variant == "pipelined":
        # one sample of the n_first pixels per pass, two passes in flight: the round after the first check takes `batch`
        # pipelined passes over the compacted list (render.hip, prepare_workspace).  A round with stats runs its passes
        # one by one, so the rounds of this variant run without, except the last.
        plane = 24 * n_first
        cfg = _with(rtsr, cfg, sample_buffer_bytes=2 * plane)
        assert batch * plane > 2 * plane and batch >= 3
    prog = scene.progressive(cam, cfg, shard=shard)
    while prog.spp_done < budget:
        before = prog.spp_done
        want = variant != "pipelined" or before + batch >= budget
        st = prog.add_adaptive(batch, min_spp, target, want_stats=want)
        active = int((prog.pixel_spp()[:rows_active] == prog.spp_done).sum())
        if before == first_check:
            assert active == n_first
        if want:
            assert st.samples == batch * active, (name, before)
            if active:
                assert st.trace_kernel == kernel, (rtsr.trace_kernel_name(st.trace_kernel), kernel_name)
    fin = prog.until_adaptive(batch, min_spp, target)
    assert prog.spp_done == fin.spp_done == done
    _check_frame(prog, snaps, counts, name)
    _check_stats(fin, snaps, counts, done, n_active, min_spp, target)
    st = prog.stats(target)  # rtx_progressive_stats: each pixel at its own count, the same reduction
    r = _own_rel_err(snaps, counts)[counts > 0]
    tree = _noise_tree(r, target)
    assert (st.pixels, st.pixels_above, st.max_rel_err, st.mean_rel_err) == (npix, tree.above, tree.max, tree.sum / npix)
    if variant == "shard":
        S, Q = prog.moments()
        assert not S[rows_active:].any() and not Q[rows_active:].any() and not counts[rows_active:].any()
    if name == "book2_1000":  # the same frame again: the same stats bytes and counts
        again = scene.progressive(cam, cfg)
        fin2 = again.until_adaptive(batch, min_spp, target)
        assert bytes(fin2) == bytes(fin)
        assert np.array_equal(again.pixel_spp(), counts)
        del again
    del prog


def test_uniform_stats_at_1000_by_1000(rtsr):
    """rtx_progressive_stats of a uniform 1000 x 1000 frame (3907 partials): exact against _noise_tree at several targets,
    and the same bytes on a second call."""
    b, flat, scene, cam, cfg = _setup(rtsr, 6, 1000, 1.0, 6)
    prog = scene.progressive(cam, cfg)
    for n in (2, 4):
        prog.add(n)
        S, Q = prog.moments()
        r = _rel_err(S, Q, prog.spp_done)
        assert r.size == 1000000
        for target in (0.0, float(np.median(r)), 1.0):
            st = prog.stats(target)
            tree = _noise_tree(r, target)
            assert (st.spp_done, st.pixels, st.pixels_above) == (prog.spp_done, r.size, tree.above)
            assert st.max_rel_err == tree.max and st.mean_rel_err == tree.sum / r.size
            assert bytes(prog.stats(target)) == bytes(st)
