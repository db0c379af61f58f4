"""scripts/wave_model.cpp: the host model of one wave of k_trace_lds.  The test builds the tool (g++ only).

1. Exactness.  The model runs the kernel's loop with the core's own arithmetic, so every sample it stores is the oracle's
   sample of that (pixel, sample), bit for bit -- with the miss-retire rule off and on, and for every item order.  A schedule
   that loses a path, traces one twice or stores to another lane's slot fails here, on the CPU.
2. Counts.  Its rays are oracle_lds_walk_render's.  Its node visits are that walk's, less one for every walk that entered
   below the root (the root step is not run), plus one for every such walk whose root step would have culled child 1: the
   oracle's walk then never visits child 1, while a walk that enters below the root finds it on its stack and pays one visit
   to learn the same (trace_lds.inc, "a ray it would have spared child 1 ...").  The model counts both kinds.
3. Direction.  Groups of two pixels cost fewer priced instructions than row strips, as measured on the device
   (profiles/item_order/README.md: + 5.5 %).  The sign only."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ray-tracing-series-rust_amd", "csrc", "host")
STRIP = 1 << 30


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("wave_model")
    exe = str(d / "wave_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "scripts", "wave_model.cpp")] +
                   [os.path.join(HOST, f) for f in ("scene_graph.cpp", "flatten.cpp", "bvh_build.cpp", "scenes.cpp")] + ["-o", exe], check=True)

    def run(sid, width, aspect, spp, depth, seed, samples=False, **options):
        args = [exe, str(sid), str(width), repr(aspect), str(spp), str(depth), str(seed)]
        for k, v in options.items():
            args += ["--" + k.replace("_", "-"), str(v)]
        path = str(d / "samples.bin")
        if samples:
            args += ["--samples-out", path]
        out = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        fields = {}
        for line in out.stdout.splitlines()[1:]:
            words = line.split()
            fields[words[0]] = float(words[1])
        return fields, (np.fromfile(path, dtype=np.float64).reshape(spp, -1, width, 3) if samples else None)
    return run


@pytest.fixture(scope="module")
def book1(rtsr, orc):
    """Book-1 canonical at 33 x 17, 3 spp, depth 50: the flat scene, and the oracle's samples [s, j, i, 3], computed once."""
    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(100)
    aspect = 1.9
    cfg = rtsr.Config.new(aspect, 33, 3, 50, 4, seed=5, background=bg)
    h = rtsr.image_height(cfg)
    assert h == 17
    flat = b.flatten(world)
    ref = np.zeros((3, h, 33, 3))
    for s in range(3):
        for j in range(h):
            for i in range(33):
                ref[s, j, i] = orc.o2_sample(flat.arrays_ptr(), cam, cfg, h, i, j, s)
    ref.setflags(write=False)
    return b, flat, cam, cfg, h, aspect, ref


@pytest.mark.parametrize("group", [1, 2, STRIP])
@pytest.mark.parametrize("rule", [(0, 0), (1, 1), (16, 8), (40, 24)], ids=lambda r: "%d_%d" % r)
def test_every_sample_is_the_oracles(model, book1, rule, group):
    b, flat, cam, cfg, h, aspect, ref = book1
    fields, got = model(100, 33, aspect, 3, 50, 5, samples=True, group=group, retire_done=rule[0], retire_min=rule[1])
    assert got.shape == ref.shape and fields["paths"] == 33 * 17 * 3
    bad = int((got != ref).any(axis=3).sum())
    assert bad == 0, "%d of %d samples differ" % (bad, 33 * 17 * 3)
    if rule == (0, 0):
        assert fields["retire_passes"] == 0
    if rule == (1, 1):
        assert fields["retire_passes"] > 0


def test_rays_and_node_visits_are_the_lds_walks(model, orc, book1):
    b, flat, cam, cfg, h, aspect, ref = book1
    _, counts = orc.lds_walk_render(flat.arrays_ptr(), cam, cfg, h, use_motion=False, threads=4)
    for rule in [(0, 0), (40, 24)]:
        f, _ = model(100, 33, aspect, 3, 50, 5, retire_done=rule[0], retire_min=rule[1])
        assert f["rays"] == counts["rays"]
        assert f["walks_below_root"] == f["rays"]  # Book-1's root is leaf-first and every ray of this frame is finite
        assert f["node_visits"] == counts["node_visits"] - f["walks_below_root"] + f["root_would_spare_child1"], (f, counts)
        assert 0 < f["root_would_spare_child1"] < f["rays"]


def test_groups_of_two_cost_less_than_row_strips(model):
    two, _ = model(100, 64, 1.5, 8, 50, 1, group=2)
    strip, _ = model(100, 64, 1.5, 8, 50, 1, group=STRIP)
    assert two["paths"] == strip["paths"] == 64 * 42 * 8 and two["rays"] == strip["rays"]
    assert two["priced_instructions"] < strip["priced_instructions"]
