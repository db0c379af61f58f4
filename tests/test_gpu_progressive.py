"""Progressive rendering on the GPU: a frame built from several rtx_progressive_add calls is the one-shot frame at the
same sample count, bit for bit; the second moment and the noise estimate equal their numpy restatements exactly."""
import collections
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "ray-tracing-series-rust_amd", "lib", "rtx_render")


def _setup(rtsr, sid, width, aspect, spp, opts=None, seed=3, f32=False, threads=10):
    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(sid, **(opts or {}))
    cfg = rtsr.Config.new(aspect, width, spp, 50, threads, seed=seed, background=bg)
    flat = b.flatten(world)
    return b, flat, flat.upload(f32=f32), cam, cfg


def _with(rtsr, cfg, **fields):
    c = rtsr.RtxConfig.from_buffer_copy(cfg)
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def _rel_err(S, Q, n):
    """The per-pixel relative error of rtx_progressive_stats, restated in numpy (every op correctly rounded)."""
    n = float(n)
    m = S / n
    var = (Q - S * S / n) / (n - 1.0)
    var = np.where(var > 0.0, var, 0.0)
    rc = np.sqrt(var / n) / (m + 1.0 / 256.0)
    r = np.zeros(S.shape[:-1])
    for c in range(3):
        r = np.where(rc[..., c] > r, rc[..., c], r)
    return r


NoiseTree = collections.namedtuple("NoiseTree", "max sum above")


def _block_tree(x):
    """noise_block_reduce on rows of 256 lanes: lane 0 of each wave64's xor butterfly (x[:32] + x[32:], then 16, 8, 4, 2, 1;
    the butterfly's other lanes add the same pairs the other way round, and an IEEE add commutes), then the block's four
    waves as ((w0 + w1) + w2) + w3."""
    w = x.reshape(-1, 4, 64)
    for h in (32, 16, 8, 4, 2, 1):
        w = w[..., :h] + w[..., h:2 * h]
    w = w[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _noise_tree(r, target):
    """rtx_progressive_stats' reduction of the per-pixel errors r (>= 0, never NaN; pixel order) in the device's exact order:
    stage 1 pads r to whole 256-pixel blocks with zeros and reduces each block (_block_tree) to one partial; stage 2 lets
    thread t add 0.0 + p[t] + p[t + 256] + ... in order and reduces those 256 sums with the same tree.  (Zeros past the last
    partial change nothing: every sum is >= +0.)  -> NoiseTree(max r, sum r bit for bit, count r > target)."""
    r = np.ascontiguousarray(r, dtype=np.float64).ravel()
    nb = -(-r.size // 256)
    x = np.zeros(nb * 256)
    x[:r.size] = r
    part = _block_tree(x)
    per = -(-nb // 256)
    p = np.zeros(per * 256)
    p[:nb] = part
    t = np.zeros(256)
    for row in p.reshape(per, 256):
        t = t + row
    return NoiseTree(float(r.max()), float(_block_tree(t)[0]), int((r > target).sum()))


SPLIT_CASES = [  # (name, scene id, width, aspect, options)
    ("book1_canonical", 100, 48, 1.5, {}),
    ("book1_head", 13, 48, 16.0 / 9.0, {}),
    ("cornell_smoke", 5, 32, 1.0, {}),
    ("book2_final", 6, 32, 1.0, {}),
    ("dragon_room", 11, 48, 16.0 / 9.0, {"mesh_triangles": 20000}),
]


@pytest.mark.parametrize("name,sid,width,aspect,opts", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_split_invariance(rtsr, name, sid, width, aspect, opts):
    b, flat, scene, cam, cfg = _setup(rtsr, sid, width, aspect, 32, opts)
    one = scene.render(cam, cfg)
    kernel = scene.render_device(cam, cfg, want_stats=True).trace_kernel
    npix = one.accum.shape[0] * one.accum.shape[1]
    for c in (cfg, _with(rtsr, cfg, sample_buffer_bytes=3 * 24 * npix)):  # small buffer: one add = several pipelined passes
        prog = scene.progressive(cam, c)
        st = prog.add(7, want_stats=True)
        assert st.trace_kernel == kernel, (rtsr.trace_kernel_name(st.trace_kernel), rtsr.trace_kernel_name(kernel))
        prog.add(1)
        prog.add(24)
        assert prog.spp_done == 32
        got = prog.screen()
        assert np.array_equal(got.accum, one.accum), "%s: %d pixels differ" % (name, int((got.accum != one.accum).any(axis=2).sum()))
        assert np.array_equal(got.rgb8, one.rgb8)
        del prog


def test_intermediate_frames_equal_one_shot_renders(rtsr):
    b, flat, scene, cam, cfg = _setup(rtsr, 100, 40, 1.5, 16)
    prog = scene.progressive(cam, cfg)
    for n, k in ((1, 1), (2, 3), (5, 8), (8, 16)):
        prog.add(n)
        got = prog.screen()
        one = scene.render(cam, _with(rtsr, cfg, samples_per_pixel=k))
        assert np.array_equal(got.accum, one.accum) and np.array_equal(got.rgb8, one.rgb8), k


def test_progressive_frame_equals_oracle(rtsr, orc):
    b, flat, scene, cam, cfg = _setup(rtsr, 100, 48, 1.5, 32)
    prog = scene.progressive(cam, cfg)
    for n in (7, 1, 24):
        prog.add(n)
    got = prog.screen()
    ref_accum, ref_rgb8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, rtsr.image_height(cfg), threads=16)
    assert np.array_equal(got.accum, ref_accum) and np.array_equal(got.rgb8, ref_rgb8)


def test_second_moment_is_the_in_order_sum_of_squares(rtsr, orc):
    b, flat, scene, cam, cfg = _setup(rtsr, 4, 8, 8.0 / 6.0, 16)  # cornell box: lit and dark pixels
    h = rtsr.image_height(cfg)
    assert h == 6
    prog = scene.progressive(cam, cfg)
    prog.add(5)
    prog.add(11)
    S, Q = prog.moments()
    s_ref = np.zeros((h, 8, 3))
    q_ref = np.zeros((h, 8, 3))
    for j in range(h):
        for i in range(8):
            s, q = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
            for k in range(16):
                x = orc.o2_sample(flat.arrays_ptr(), cam, cfg, h, i, j, k)
                for c in range(3):
                    xc = float(x[c])
                    s[c] = s[c] + xc
                    q[c] = q[c] + xc * xc  # two roundings, as on the device
            s_ref[j, i], q_ref[j, i] = s, q
    assert np.array_equal(S, s_ref)
    assert np.array_equal(Q, q_ref)
    assert (Q > 0).any()


def test_noise_stats_equal_numpy_restatement_and_converge(rtsr):
    b, flat, scene, cam, cfg = _setup(rtsr, 100, 40, 1.5, 1024)
    prog = scene.progressive(cam, cfg)
    maxes, means = [], []
    for n, spp in ((4, 4), (60, 64), (960, 1024)):
        prog.add(n)
        S, Q = prog.moments()
        r = _rel_err(S, Q, spp)
        for target in (0.0, float(np.median(r)), 0.05, 10.0):
            st = prog.stats(target)
            assert (st.spp_done, st.pixels, st.target_rel_err) == (spp, r.size, target)
            assert st.pixels_above == int((r > target).sum())
            assert st.max_rel_err == r.max()
            assert st.mean_rel_err == _noise_tree(r, target).sum / r.size
            again = prog.stats(target)
            assert bytes(again) == bytes(st)
        maxes.append(st.max_rel_err)
        means.append(st.mean_rel_err)
    assert maxes[0] > maxes[1] > maxes[2] and means[0] > means[1] > means[2], (maxes, means)


def test_stop_rule_and_budget(rtsr):
    b, flat, scene, cam, cfg = _setup(rtsr, 100, 40, 1.5, 64)
    ref = scene.progressive(cam, cfg)
    with pytest.raises(rtsr.RtxError) as e:
        ref.screen()
    assert e.value.status == rtsr.RTX_EINVAL
    for bad in (0, -1, 65):
        with pytest.raises(rtsr.RtxError) as e:
            ref.add(bad)
        assert e.value.status == rtsr.RTX_EINVAL
    ref.add(1)
    with pytest.raises(rtsr.RtxError) as e:
        ref.stats(0.1)  # one sample has no variance
    assert e.value.status == rtsr.RTX_EINVAL
    ref = scene.progressive(cam, cfg)
    trail = []
    while ref.spp_done < 64:
        ref.add(4)
        trail.append(ref.stats(0.0).max_rel_err)
    target = trail[5]  # reached at 24 spp; the first boundary at or below it may come earlier
    expect = 4 * (next(k for k, m in enumerate(trail) if m <= target) + 1)
    prog = scene.progressive(cam, cfg)
    st = prog.until(4, target)
    assert st.pixels_above == 0 and st.spp_done == prog.spp_done == expect
    assert st.max_rel_err == trail[expect // 4 - 1]
    assert np.array_equal(prog.screen().accum, scene.render(cam, _with(rtsr, cfg, samples_per_pixel=expect)).accum)
    # an unreachable target stops at the budget, the last batch clipped to it
    prog = scene.progressive(cam, _with(rtsr, cfg, samples_per_pixel=30))
    st = prog.until(8, 0.0)
    assert st.spp_done == prog.spp_done == 30 and st.pixels_above > 0
    with pytest.raises(rtsr.RtxError):
        prog.add(1)


def test_shard_with_row_chunk_compat(rtsr):
    import torch
    b, flat, scene, cam, cfg = _setup(rtsr, 100, 40, 1.0, 8, threads=16)
    cfg.row_chunk_compat = 1  # rows 32..39 are never rendered
    shard = (1, 3, 2)
    h = rtsr.image_height(cfg)
    rows = [j for j in range(h) if (j // 2) % 3 == 1]
    assert rtsr.shard_rows(cfg, shard) == len(rows)
    d_acc = torch.full((len(rows) * 40 * 3,), -1.0, dtype=torch.float64, device="cuda")
    d_rgb = torch.full((len(rows) * 40 * 3,), 7, dtype=torch.uint8, device="cuda")
    scene.render_device(cam, cfg, shard=shard, d_accum=d_acc.data_ptr(), d_rgb8=d_rgb.data_ptr(),
                        stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    prog = scene.progressive(cam, cfg, shard=shard)
    prog.add(3)
    prog.add(5)
    got = prog.screen()
    S, Q = prog.moments()
    assert np.array_equal(got.accum, d_acc.cpu().numpy().reshape(len(rows), 40, 3))
    assert np.array_equal(got.rgb8, d_rgb.cpu().numpy().reshape(len(rows), 40, 3))
    skipped = [k for k, j in enumerate(rows) if j >= 32]
    assert skipped and not S[skipped].any() and not Q[skipped].any() and not got.rgb8[skipped].any()
    active = len(rows) - len(skipped)
    st = prog.stats(0.0)
    assert st.pixels == active * 40
    assert st.max_rel_err == _rel_err(S[:active], Q[:active], 8).max()


def test_f32_scene_split_invariance(rtsr):
    b, flat, scene, cam, cfg = _setup(rtsr, 100, 48, 1.5, 32, f32=True)
    assert scene.is_f32
    one = scene.render(cam, cfg)
    prog = scene.progressive(cam, cfg)
    for n in (7, 1, 24):
        prog.add(n)
    got = prog.screen()
    assert np.array_equal(got.accum, one.accum) and np.array_equal(got.rgb8, one.rgb8)
    assert prog.stats(0.1).spp_done == 32


def test_app_progressive_equals_one_shot(tmp_path):
    assert os.path.exists(APP), "apps/rtx_render was not built (python __graft_entry__.py)"
    base = [APP, "--scene", "100", "--width", "48", "--aspect", "1.5", "--depth", "50", "--threads", "10", "--seed", "1"]

    def run(*extra):
        res = subprocess.run(base + list(extra), capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert res.returncode == 0, res.stderr
        return res.stderr

    run("--spp", "32", "--out", str(tmp_path / "one.ppm"))
    run("--spp", "16", "--out", str(tmp_path / "one16.ppm"))
    err = run("--spp", "32", "--batch", "8", "--target-error", "0", "--snapshot-every", "16", "--out", str(tmp_path / "prog.ppm"))
    assert "spp reached: 32 of 32" in err
    assert (tmp_path / "prog.ppm").read_bytes() == (tmp_path / "one.ppm").read_bytes()
    assert (tmp_path / "prog.ppm.16.ppm").read_bytes() == (tmp_path / "one16.ppm").read_bytes()
    err = run("--spp", "32", "--batch", "8", "--target-error", "0", "--out", str(tmp_path / "until.ppm"))
    assert "spp reached: 32 of 32" in err
    assert (tmp_path / "until.ppm").read_bytes() == (tmp_path / "one.ppm").read_bytes()
    err = run("--spp", "64", "--batch", "8", "--target-error", "1e9", "--out", str(tmp_path / "early.ppm"))
    assert "spp reached: 8 of 64" in err  # every pixel meets a huge target at the first boundary
