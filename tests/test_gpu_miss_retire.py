"""Miss retire (csrc/hip/trace_lds.inc) is a schedule: k_trace_lds with a ring hands the finished
misses of a round on before the round ends.  No path's arithmetic, stream or slot changes, so every frame must be the CPU
oracle's bit for bit, as tests/test_gpu_parity.py compares them, under every (RTX_RETIRE_DONE, RTX_RETIRE_MIN): 0 / 0 (off),
1 / 1 (the loop leaves after every second finished walk and any miss retires), 16 / 8, 40 / 24 and 63 / 64 (never fires: a
wave has no 64 misses while another lane walks) -- each with the defaults and with RTX_RING=1 and chunks of 64 and of 512 items.

Frames: Book-1 canonical at 64 x 42, 4 spp; 7 x 5 at 3 spp (105 items: no multiple of 64); 1 x 1 (its rays are not finite and
start at the root); depth 1 (every path ends in bounce begin); a world every primary ray misses (each lane retires inside the
loop and the ring drains to the queue's end); a world no ray can miss (the rule never finds a miss); a shard; an adaptive pass
over a pixel list; and HEAD Book-1, whose ringless instantiations do not have the rule."""
import numpy as np
import pytest

from test_gpu_progressive import _rel_err, _with

pytestmark = pytest.mark.gpu

RULES = [("0", "0"), ("1", "1"), ("16", "8"), ("40", "24"), ("63", "64")]
SETTINGS = [{"RTX_RETIRE_DONE": d, "RTX_RETIRE_MIN": m} for d, m in RULES]
SETTINGS += [{"RTX_RETIRE_DONE": d, "RTX_RETIRE_MIN": m, "RTX_RING": "1", "RTX_CHUNK": c} for d, m in RULES for c in ("64", "512")]
SKY = (0.7, 0.8, 1.0)
BOOK1_CAMERA = ((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, 1.5, 0.1, 10.0, 0.0, 1.0)


def _upload_under(monkeypatch, flat, env):
    """The scene uploaded under the switches of env (they are read at upload)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene = flat.upload()
    for k in env:
        monkeypatch.delenv(k)
    return scene


def _catalogue(rtsr, sid, width, aspect, spp, depth=50):
    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(sid, camera_aspect=aspect)
    return b, b.flatten(world), cam, rtsr.Config.new(aspect, width, spp, depth, 4, seed=7, background=bg)


def _spheres(rtsr, which):
    b = rtsr.Builder(1)
    lst = b.hittable_list()
    if which == "all_miss":  # four small spheres behind the camera, which looks the other way
        for k in range(4):
            b.list_add(lst, b.sphere((26.0 + 1.5 * k, 4.0 + 0.5 * (k % 2), 6.0 + 0.7 * k), 0.4, b.lambertian((0.6, 0.3, 0.2))))
    else:  # "no_miss": the camera inside one large Lambertian sphere, two small ones beside it
        b.list_add(lst, b.sphere((0.0, 0.0, 0.0), 60.0, b.lambertian((0.8, 0.7, 0.6))))
        b.list_add(lst, b.sphere((0.0, 0.5, 0.0), 0.5, b.metal((0.8, 0.8, 0.9), 0.1)))
        b.list_add(lst, b.sphere((2.0, 0.4, 1.0), 0.4, b.dielectric(1.5)))
    world = b.hittable_list([b.bvh_from_list(lst, 0.0, 1.0)])
    return b, b.flatten(world), rtsr.Camera.new(*BOOK1_CAMERA), rtsr.Config.new(1.5, 64, 4, 50, 4, seed=7, background=SKY)


FRAMES = {
    "book1_64x42": lambda r: _catalogue(r, 100, 64, 1.5, 4),
    "7x5": lambda r: _catalogue(r, 100, 7, 1.4, 3),
    "1x1": lambda r: _catalogue(r, 100, 1, 1.0, 3),
    "depth_1": lambda r: _catalogue(r, 100, 64, 1.5, 4, depth=1),
    "all_miss": lambda r: _spheres(r, "all_miss"),
    "no_miss": lambda r: _spheres(r, "no_miss"),
}


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_every_rule_renders_the_oracles_frame(rtsr, orc, monkeypatch, name):
    b, flat, cam, cfg = FRAMES[name](rtsr)
    h = rtsr.image_height(cfg)
    assert (cfg.image_width, h) == {"7x5": (7, 5), "1x1": (1, 1)}.get(name, (64, 42))
    ref_accum, ref_rgb8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=8)
    if name == "all_miss":
        assert np.array_equal(ref_accum, np.broadcast_to(np.array(SKY) * cfg.samples_per_pixel, ref_accum.shape))
    if name == "no_miss":  # nothing ever reaches the sky, and nothing emits
        assert not ref_accum.any()
    for env in SETTINGS:
        screen = _upload_under(monkeypatch, flat, env).render(cam, cfg, want_stats=True)
        assert rtsr.trace_kernel_name(screen.stats.trace_kernel) == "k_trace_lds", env
        bad = int((screen.accum != ref_accum).any(axis=2).sum())
        assert bad == 0, "%s under %r: %d pixels differ" % (name, env, bad)
        assert np.array_equal(screen.rgb8, ref_rgb8), (name, env)


def test_a_shard_under_every_rule(rtsr, orc, monkeypatch):
    b, flat, cam, cfg = FRAMES["book1_64x42"](rtsr)
    h, shard = rtsr.image_height(cfg), (1, 3, 1)
    ref_accum, ref_rgb8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, shard=shard, threads=8)
    assert ref_accum.shape == (14, 64, 3)
    for env in SETTINGS:
        prog = _upload_under(monkeypatch, flat, env).progressive(cam, cfg, shard=shard)
        prog.add(cfg.samples_per_pixel)
        got = prog.screen()
        assert np.array_equal(got.accum, ref_accum) and np.array_equal(got.rgb8, ref_rgb8), env


def test_an_adaptive_pass_over_a_pixel_list(rtsr, orc, monkeypatch):
    """8 uniform samples, then one adaptive round of 5 over the half of the pixels with the larger error: a retired lane stores
    to the slot its list entry was given.  Every pixel's sums are the sums of the oracle's samples, added in sample order."""
    b, flat, cam, cfg = _catalogue(rtsr, 100, 24, 1.5, 13)
    h = rtsr.image_height(cfg)
    target, want = None, None
    for env in SETTINGS:
        prog = _upload_under(monkeypatch, flat, env).progressive(cam, cfg)
        prog.add(8)
        if target is None:
            S, Q = prog.moments()
            target = float(np.median(_rel_err(S, Q, 8)))
        prog.add_adaptive(5, 6, target)
        counts = prog.pixel_spp()
        S, Q = prog.moments()
        if want is None:
            assert 0 < int((counts == 13).sum()) < counts.size and set(np.unique(counts)) == {8, 13}
            want = np.zeros_like(S)
            for j in range(h):
                for i in range(24):
                    s = [0.0, 0.0, 0.0]
                    for k in range(int(counts[j, i])):
                        x = orc.o2_sample(flat.arrays_ptr(), cam, cfg, h, i, j, k)
                        s = [s[c] + float(x[c]) for c in range(3)]
                    want[j, i] = s
            want_counts = counts
        assert np.array_equal(counts, want_counts), env
        assert np.array_equal(S, want), env


def test_head_book1_has_no_rule(rtsr, orc, monkeypatch):
    """HEAD Book-1 runs the instantiations without a ring, which regenerate in the lane: the switches are read and change nothing."""
    b, flat, cam, cfg = _catalogue(rtsr, 13, 64, 1.5, 4)
    h = rtsr.image_height(cfg)
    ref_accum, ref_rgb8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=8)
    for env in SETTINGS[:5]:
        screen = _upload_under(monkeypatch, flat, env).render(cam, cfg, want_stats=True)
        assert rtsr.trace_kernel_name(screen.stats.trace_kernel) == "k_trace_lds"
        assert np.array_equal(screen.accum, ref_accum) and np.array_equal(screen.rgb8, ref_rgb8), env
