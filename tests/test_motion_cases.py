"""The scenes of tests/motion_cases.py on the CPU, before the device sees them (tests/test_gpu_motion_cases.py): the literal
object-graph oracle O1, the flat oracle O2 and the CPU restatement of k_trace_lds's walk render one frame bit for bit under
every interval of the table, the time-aware boxes hold their spheres and cull, a ray from a mover's centre leaves its sphere
at t = r, and the launcher's host-side choice of k_trace_lds instantiation (csrc/hip/lds_variant.inc) follows the table.
The two cases without one frame through a BVH -- `straddle` (ray times outside the BVH's interval) and `degenerate`
(time0 == time1: NaN roots) -- are held to what does hold, and the reason is given."""
import os
import subprocess

import numpy as np
import pytest

import motion_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _diff(a, b):
    return "%d pixels differ" % int((~((a == b) | (np.isnan(a) & np.isnan(b)))).any(axis=2).sum())


@pytest.mark.parametrize("case_id,shutter", [p for p in mc.SHUTTERS if p[0] in mc.PARITY], ids=lambda v: str(v))
def test_oracles_and_the_lds_walk_render_one_frame(rtsr, orc, case_id, shutter):
    b, world, cam, cfg, movers = mc.build(rtsr, case_id, shutter)
    assert (cfg.image_width, cfg.samples_per_pixel, cfg.max_depth) == (96, 4, 20) and len(movers) == 89
    h = rtsr.image_height(cfg)
    flat = b.flatten(world)
    info = flat.info()
    assert info["n_bvh"] == 1 and info["n_refs"] == mc.N_BVH and info["n_moving_spheres"] == len(movers)
    a1, r1 = orc.o1_render(b.graph_ptr(), world, cam, cfg, h, threads=8)
    a2, r2 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=8)
    static, c_static = orc.lds_walk_render(flat.arrays_ptr(), cam, cfg, h, use_motion=False, threads=8)
    assert np.isfinite(a1).all() and len(np.unique(a1.reshape(-1, 3), axis=0)) >= 50, "the frame shows the scene"
    assert np.array_equal(a1, a2), _diff(a1, a2)
    assert np.array_equal(r1, r2)
    assert np.array_equal(static, a2), _diff(static, a2)
    rc, checked = orc.audit_motion(flat.arrays_ptr(), 32)
    assert rc == 0, "audit_motion code %d" % rc
    if case_id == "reversed_bvh":
        # build_motion_boxes makes none for a BVH with time0 >= time1: the walk over them says so (code 3) instead of rendering
        assert checked == 0 and not mc.shutter_inside(case_id, shutter)
        with pytest.raises(RuntimeError, match=r"failed \(3\)"):
            orc.lds_walk_render(flat.arrays_ptr(), cam, cfg, h, use_motion=True, threads=8)
        return
    assert checked > 0 and mc.shutter_inside(case_id, shutter)
    moving, c_moving = orc.lds_walk_render(flat.arrays_ptr(), cam, cfg, h, use_motion=True, threads=8)
    assert np.array_equal(moving, a2), _diff(moving, a2)
    # the slopes are there and cull: an all-zero slope array would render the same frame
    assert c_moving["rays"] == c_static["rays"] and c_moving["node_visits"] < c_static["node_visits"], (c_static, c_moving)


@pytest.mark.parametrize("case_id", mc.PARITY)
def test_a_ray_from_a_movers_centre_leaves_it_at_its_radius(rtsr, orc, case_id):
    """c(t) in longdouble from the table, a ray from it along +y, +x and -z at four instants of the BVH's interval: t = r within
    1e-9 relative.  The bound is derived: the f64 quadratic on these rays is good to 1e-14, and a wrong interval, ratio or end
    point moves a centre by at least 1e-3 of a travel of at least 0.25.  A ray that a neighbouring sphere answers first (worked
    out in longdouble in motion_cases.centre_rays) claims nothing; those are at most a quarter of any instant's rays."""
    b, world, cam, cfg, movers = mc.build(rtsr, case_id)
    flat = b.flatten(world)
    for c0, c1, t0, t1, r in movers:
        assert np.abs(np.array(c1) - np.array(c0)).max() >= 0.25
    n_claimed = 0
    for t, origins, dirs, radii, blocked in mc.centre_rays(case_id, movers):
        assert len(origins) == 3 * len(movers)
        assert 4 * blocked.sum() <= len(blocked), (case_id, t, int(blocked.sum()), len(blocked))
        worst = 0.0
        for k in np.nonzero(~blocked)[0]:
            rec = orc.core_world_hit(flat.arrays_ptr(), origins[k], dirs[k], time=t)
            assert rec is not None, (case_id, t, k)
            worst = max(worst, abs(rec["t"] - radii[k]) / radii[k])
            assert abs(rec["t"] - radii[k]) <= 1e-9 * radii[k], (case_id, t, k, rec["t"], radii[k])
            n_claimed += 1
        print("[motion cases] %s t = %g: %d of %d rays answered by a neighbour, worst |t - r| / r = %.3g" % (
            case_id, t, int(blocked.sum()), len(blocked), worst))
    assert n_claimed >= 3 * len(movers) * 3


@pytest.mark.parametrize("case_id,shutter", [p for p in mc.SHUTTERS if p[0] in ("straddle", "degenerate")], ids=lambda v: str(v))
def test_list_form_of_the_cases_without_one_bvh_frame(rtsr, orc, case_id, shutter):
    """straddle: ray times beyond the BVH's interval, where a sphere may be outside the box the reference gives it
    (tests/test_gpu_compat.py: test_time_aware_boxes_on_the_device says why no frame is claimed there).  degenerate:
    time0 == time1 makes the ratio x / 0 and the root a NaN, which `root < t_min || t_max < root` lets through (hit.rs, restated
    literally by sphere_root): such a sphere answers every ray that reaches it with t = NaN and whatever is tested next
    replaces it, so the outcome depends on the order of the tests.  A plain list fixes that order: O1 == O2 there."""
    b, world, cam, cfg, movers = mc.build(rtsr, case_id, shutter, as_list=True)
    h = rtsr.image_height(cfg)
    flat = b.flatten(world)
    assert flat.info()["n_bvh"] == 0 and flat.info()["n_top_level"] == mc.N_LIST and len(movers) == 29
    a1, r1 = orc.o1_render(b.graph_ptr(), world, cam, cfg, h, threads=8)
    a2, r2 = orc.o2_render(flat.arrays_ptr(), cam, cfg, h, threads=8)
    assert np.array_equal(a1, a2, equal_nan=True), _diff(a1, a2)
    assert np.array_equal(r1, r2)
    if case_id == "straddle":
        assert np.isfinite(a1).all() and len(np.unique(a1.reshape(-1, 3), axis=0)) >= 50
    if case_id == "degenerate":
        # the reference's NaN behaviour, recorded: these movers are NOT invisible (without boxes in front of them every ray
        # reaches them, and the last of them in the list answers it)
        b0, world0, _, _, none = mc.build(rtsr, case_id, shutter, as_list=True, with_movers=False)
        assert none == []
        flat0 = b0.flatten(world0)  # (kept: arrays_ptr points into it)
        a0, _ = orc.o2_render(flat0.arrays_ptr(), cam, cfg, h, threads=8)
        assert np.isfinite(a0).all() and not np.array_equal(a0, a2, equal_nan=True)
        # what they do to it: a NaN root is no miss, so every ray of every bounce meets SOMETHING, none reaches the sky, and a
        # scene lit by its background alone is black.  (The same holds under a BVH: such a mover's boxes are not finite.)
        assert not a2.any()
        bb, bvh_world, _, _, _ = mc.build(rtsr, case_id, shutter)
        bvh_flat = bb.flatten(bvh_world)
        assert orc.audit_motion(bvh_flat.arrays_ptr(), 32)[0] == 3  # "a box does not hold its sphere": none can, the centres are not finite
        assert not orc.o2_render(bvh_flat.arrays_ptr(), cam, cfg, h, threads=8)[0].any()


@pytest.fixture(scope="module")
def variant_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lds_variant") / "lds_variant_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "lds_variant_host_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0", UBSAN_OPTIONS="halt_on_error=1")

    def run(*args):
        out = subprocess.run([exe] + [repr(a) if isinstance(a, float) else str(a) for a in args], capture_output=True, text=True, env=env, timeout=60)
        assert out.returncode == 0 and "runtime error" not in out.stderr, out.stdout + out.stderr
        return out.stdout.split()
    return run


def test_the_launchers_choice_follows_the_table(variant_exe):
    """csrc/hip/lds_variant.inc, the code plan_lds and launch_lds decide with, asked on the host for every (case, shutter): the
    common ratio only for ONE interval that is not empty (time0 == time1 would make every static sphere's centre a NaN), the
    time-aware boxes only for a shutter inside an ordered BVH interval, so `straddle` and `reversed_bvh` fall back."""
    for case_id, (intervals, bvh, shutters, axes) in mc.CASES.items():
        per_mover = [intervals[k % len(intervals)] for k in range(1, 13) if k % 4]
        got = variant_exe("common", *[x for iv in per_mover for x in iv])
        common = case_id not in ("mixed", "degenerate")
        assert [float(x) for x in got] == ([1.0, intervals[0][0], intervals[0][1]] if common else [0.0]), (case_id, got)
        for k, (s0, s1) in enumerate(shutters):
            axis = 1 if axes == "y" else -1
            fits = bvh[0] < bvh[1]  # plan_lds fits the time-aware variant for an ordered interval only
            got = int(variant_exe("variant", int(fits), bvh[0], bvh[1], s0, s1, axis, int(common))[0])
            assert got == mc.expected_variant(case_id, k), (case_id, k, got)
            # a plan that offered the boxes for a reversed interval all the same is still refused per render
            assert int(variant_exe("variant", 1, bvh[0], bvh[1], s0, s1, axis, int(common))[0]) == got
    assert variant_exe("common") == ["0"]  # no movers: nothing to share
    assert mc.expected_variant("straddle", 0) == mc.COMMON_RATIO and mc.expected_variant("straddle", 1) == mc.COMMON_RATIO
    assert mc.expected_variant("reversed_bvh") == mc.COMMON_RATIO and mc.expected_variant("degenerate") == mc.TIME_BOXES
    assert mc.expected_variant("y_only_offset") == 7 and mc.expected_variant("x_only") == 5 and mc.expected_variant("mixed") == 1
