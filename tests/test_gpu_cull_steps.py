"""The f32 culling code on the device, asked directly (rtx_device_cull_verdicts, rtx_device_walk_steps, and the resident 4-wide
tree through rtx_device_scene_array): what an image test cannot see.

  * the resident FlatNode4 array and the stack levels of a scene uploaded under RTX_WIDE=1 are, byte for byte, those of
    tests/wide_tree_host_check.cpp, which tests/test_wide_tree.py audits against the tree's definition;
  * one step of walk_node_step4 / walk_node_step32, with LdsStack and LdsStackB, equals a plain restatement
    (tests/wide_step_host_check.cpp: fmaf / fminf / fmaxf, a stable sort, a std::vector) in the next item, in n and in every live
    slot [0, n); dead slots are not compared; the guard slots above `levels` still hold their canary;
  * no form of the box test says "miss" for a box the exact ray meets (tests/cull_cases.py; the CPU half and the one excepted
    class: tests/test_cull_conservative.py).  The device differs from the host by v_rcp_f32 (1 ulp) and v_med3_f32 only.

Culling efficiency on the device, recorded and not asserted (share of the judged `near` cases the exact ray misses that a form
lets through; MI355X, seed 2): f64 may_hit / hit2 44.1 %, nf 36.7 %, nf_pos and wide 35.7 %; fast mode 2.45 % in every form.
The device's verdict words equalled the host's in 196 595 of 196 608 f64 cases and in all 135 456 fast-mode cases."""
import numpy as np
import pytest

import cull_cases as cc
import wide_tree_cases as wt

pytestmark = pytest.mark.gpu

SCENES = [k for k, v in wt.CASES.items() if k not in ("comb", "ties_and_odd_areas")]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("cull_steps")


@pytest.fixture(scope="module")
def host_trees(rtsr, workdir):
    """case id -> (wide records, levels) of the host check, made once."""
    exe = wt.build_host_check(workdir)
    return {k: wt.run_host_check(exe, workdir, k, wt.case(rtsr, k)["nodes"], wt.case(rtsr, k)["roots"]) for k in SCENES}


def test_the_resident_wide_tree_is_the_audited_one(rtsr, host_trees, monkeypatch):
    monkeypatch.setenv("RTX_WIDE", "1")
    accepted = []
    for k in SCENES:
        scene = wt.case(rtsr, k)["flat"].upload()
        got = scene.array("nodes4")
        if got.size == 0:  # plan_wide keeps the binary tree: a sphere world of one BVH
            assert scene.wide_levels() == 0
            continue
        accepted.append(k)
        wide, levels = host_trees[k]
        assert scene.wide_levels() == levels, k
        assert got.tobytes() == np.ascontiguousarray(wide).tobytes(), k
    print("wide trees resident for:", accepted)
    assert {"dragon_2000", "dragon_20000", "book2_final", "two_bvhs", "two_triangle_bvh"} <= set(accepted)


def _rays32(rtsr, workdir, tag, lo, hi, n, seed):
    """n culling rays around the box [lo, hi]: half start outside and aim at a point of it (camera rays), half start inside
    (bounce rays); a tenth have a zero component.  The Ray32 is the HOST's make_ray32 (so no reciprocal enters the step)."""
    rng = np.random.default_rng(seed)
    size = hi - lo
    target = lo + size * rng.random((n, 3))
    outside = lo + size * (rng.random((n, 3)) * 5.0 - 2.0)
    inside = lo + size * rng.random((n, 3))
    o = np.where((np.arange(n) % 2 == 0)[:, None], outside, inside)
    d = target - o + 1e-3 * size * (rng.random((n, 3)) - 0.5)
    d = np.where(rng.random((n, 3)) < 1.0 / 30.0, np.where(rng.random((n, 3)) < 0.5, 0.0, -0.0), d)
    d[:, 0] = np.where(np.all(d == 0.0, axis=1), 1.0, d[:, 0])
    ray = np.concatenate([o, d, np.full((n, 1), 0.001), np.full((n, 1), np.inf)], axis=1)
    q, _, _ = cc.host_verdicts(cc.build_host_check(workdir, False), workdir, tag, np.tile(np.concatenate([lo, hi]), (n, 1)), ray)
    return q, d


ITEM = np.dtype([("node", "<i4"), ("second_node", "<i4"), ("q", "<f4", (8,)), ("dir", "<f8", (3,)), ("t_max32", "<f4"),
                 ("n_stack", "<i4"), ("stack", "<i4", (4,))])  # RtxWalkStepItem


def _items(nodes_idx, q, d, t_max32, n_stack, stack=None, second=None):
    it = np.zeros(len(nodes_idx), dtype=ITEM)
    it["node"], it["second_node"] = nodes_idx, -1 if second is None else second
    it["q"], it["dir"], it["t_max32"], it["n_stack"] = q, d, t_max32, n_stack
    it["stack"] = np.array([0x100, 0x101, 0x102, 0x103], dtype=np.int32) if stack is None else stack
    return it


def _compare(rtsr, workdir, tag, kind, nodes, levels, items):
    """Both stack types: device == restatement in the item, n and the live slots; canaries intact."""
    assert ITEM == rtsr.WALK_STEP_ITEM
    exe = cc.build_host_check(workdir, False)
    for bottom in (False, True):
        keep = items["n_stack"] + (1 if bottom else 0) <= levels
        its = items[keep]
        want_cur, want_n, want_slots = cc.host_steps(exe, workdir, "%s_%d" % (tag, bottom), kind, bottom, levels, nodes, its)
        for first in range(0, len(its), 65536):
            sl = slice(first, first + 65536)
            cur, n, slots = rtsr.device_walk_steps(kind, bottom, nodes, levels, its[sl])
            assert np.array_equal(cur, want_cur[sl]), (tag, bottom, int(np.nonzero(cur != want_cur[sl])[0][0]))
            assert np.array_equal(n, want_n[sl]), (tag, bottom)
            live = np.arange(levels)[None, :] < n[:, None]
            assert np.array_equal(np.where(live, slots[:, :levels], 0), np.where(live, want_slots[sl], 0)), (tag, bottom)
            assert (slots[:, levels:] == rtsr.WALK_CANARY).all(), (tag, bottom, "a store above `levels`")
        print(tag, "bottom" if bottom else "plain", len(its), "steps; n after:", np.bincount(want_n, minlength=1).tolist()[:12])


@pytest.mark.parametrize("case_id", ["dragon_2000", "book2_final"])
def test_a_wide_step_on_every_node_of_a_tree_equals_its_restatement(rtsr, workdir, host_trees, case_id):
    """Every wide node a walk reaches, 64 rays each, with 0, 1 and the node's worst-case number of entries below it."""
    c = wt.case(rtsr, case_id)
    wide, levels = host_trees[case_id]
    below = wt.worst_below(wide, c["roots"])
    idx = np.array(sorted(below), dtype=np.int32)
    root = c["roots"][0]
    lo = np.minimum(c["nodes"]["bmin"][root][0], c["nodes"]["bmin"][root][1])
    hi = np.maximum(c["nodes"]["bmax"][root][0], c["nodes"]["bmax"][root][1])
    q, d = _rays32(rtsr, workdir, case_id + "_rays", lo, hi, 64 * len(idx), seed=5)
    node = np.repeat(idx, 64)
    rng = np.random.default_rng(6)
    t_max32 = np.where(rng.random(len(node)) < 0.5, np.inf, np.float32(np.linalg.norm(hi - lo)) * rng.random(len(node))).astype(np.float32)
    parts = [_items(node, q, d, t_max32, depth) for depth in (0, 1)]
    parts.append(_items(node, q, d, t_max32, np.repeat(np.array([below[i] for i in idx], dtype=np.int32), 64)))
    assert max(below.values()) + 4 + 1 >= levels  # the deepest node's worst case reaches the top level
    _compare(rtsr, workdir, case_id, "step4", wide, levels, np.concatenate(parts))


@pytest.mark.parametrize("case_id", ["dragon_2000", "book2_final"])
def test_a_binary_step_on_every_node_of_a_tree_equals_its_restatement(rtsr, workdir, case_id):
    """walk_node_step32's both / one / none arithmetic, on every node of the tree's array, 64 rays each, 0, 1 and 7 entries below."""
    c = wt.case(rtsr, case_id)
    root = c["roots"][0]
    lo = np.minimum(c["nodes"]["bmin"][root][0], c["nodes"]["bmin"][root][1])
    hi = np.maximum(c["nodes"]["bmax"][root][0], c["nodes"]["bmax"][root][1])
    n_nodes = len(c["nodes32"])
    q, d = _rays32(rtsr, workdir, case_id + "_rays32", lo, hi, 64 * n_nodes, seed=7)
    node = np.repeat(np.arange(n_nodes, dtype=np.int32), 64)
    rng = np.random.default_rng(8)
    t_max32 = np.where(rng.random(len(node)) < 0.5, np.inf, np.float32(np.linalg.norm(hi - lo)) * rng.random(len(node))).astype(np.float32)
    items = np.concatenate([_items(node, q, d, t_max32, depth) for depth in (0, 1, 7)])
    _compare(rtsr, workdir, case_id + "_bin", "step32", c["nodes32"], 12, items)
    # the fast mode's compilation of the same step, on the same data: one item in seven
    sub = items[::7][:65536]
    for bottom in (False, True):
        a = rtsr.device_walk_steps("step32", bottom, c["nodes32"], 12, sub, f32=False)
        b = rtsr.device_walk_steps("step32", bottom, c["nodes32"], 12, sub, f32=True)
        live = np.arange(12)[None, :] < a[1][:, None]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(np.where(live, a[2][:, :12], 0), np.where(live, b[2][:, :12], 0)) and (b[2][:, 12:] == rtsr.WALK_CANARY).all()


def _synthetic_wide():
    """Hand-made records: 0 four identical boxes, 1 / 2 / 3 with one / two / three empty slots, 4 zero-thickness boxes, 5 boxes
    in the eight octants' directions (two records), 7 one subnormal plane, 8 boxes far apart (t_max32 below their entry)."""
    L = wt.make_leaf
    w = np.zeros(9, dtype=wt.NODE4)
    w["lo"], w["hi"], w["child"] = np.inf, -np.inf, wt.EMPTY

    def put(i, k, lo, hi, code):
        w["lo"][i][:, k], w["hi"][i][:, k], w["child"][i][k] = lo, hi, code
    for k in range(4):
        put(0, k, (-1, -1, -1), (1, 1, 1), L(k, 1))
    for i, filled in ((1, 3), (2, 2), (3, 1)):
        for k in range(filled):
            put(i, k, (-1 + k, -1, -1), (1 + k, 1, 1), L(10 * i + k, 1))
    for k in range(4):
        put(4, k, (0.5 * k, -1, -1), (0.5 * k, 1, 1), L(40 + k, 1))
    signs = [(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    for j, s in enumerate(signs):
        c = 3.0 * np.array(s, dtype=np.float32)
        put(5 + j // 4, j % 4, c - 1, c + 1, 50 + j)  # inner codes: they go on the stack like any other
    put(7, 0, (np.float32(1e-45), -1, -1), (1, 1, 1), L(70, 1))
    put(7, 1, (-1, -1, -1), (np.float32(-1e-45), 1, 1), L(71, 1))
    for k in range(4):
        put(8, k, (100.0 * (k + 1), -1, -1), (100.0 * (k + 1) + 1, 1, 1), L(80 + k, 1))
    return w


def test_wide_steps_on_hand_made_records_equal_their_restatement(rtsr, workdir):
    w = _synthetic_wide()
    levels = 10  # five entries and the bottom slot below, four hits: slot 9 is the highest a step here can write
    rng = np.random.default_rng(9)
    # rays from every octant towards the origin, from inside, along the axes (zero components of both signs)
    dirs = [(sx, sy, sz) for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)]
    dirs += [(1.0, 0.0, 0.0), (-1.0, -0.0, 0.0), (0.0, 1.0, -0.0), (-0.0, -0.0, 1.0), (1.0, 1e-30, -1e-30)]
    rays = []
    for dv in dirs:
        for o in ((0.0, 0.0, 0.0), (0.25, -0.5, 0.125), tuple(-6.0 * np.array(dv)), tuple(-6.0 * np.array(dv) + 0.3), (0.5, 0.0, 0.0), (1.0, 1.0, 1.0)):
            rays.append(list(o) + list(dv) + [0.001, np.inf])
    ray = np.array(rays)
    q, _, _ = cc.host_verdicts(cc.build_host_check(workdir, False), workdir, "synthetic_rays", np.tile([-1.0, -1, -1, 1, 1, 1], (len(ray), 1)), ray)
    special = np.zeros((6, 8), dtype=np.float32)  # the Ray32 as data
    special[0] = 0.0                                         # zero slopes, oi = 0, t_min = 0: every plane at t = 0, every box hit
    special[1] = (1, 1, 1, np.nan, 0, 0, 0, 0.001)           # a NaN entry distance on x: the key is t_min
    special[2] = (np.inf, 1, 1, np.inf, 0, 0, 0, 0.001)      # inf - inf
    special[3] = (1, 1, 1, -np.inf, 0, 0, 0, 0.001)          # every plane at +inf: the key clamps to 3e38
    special[4] = (-1, -1, -1, 3, 3, 3, np.float32(1e-6), 0.001)
    special[5] = (np.float32(1e-45), 1, 1, 0, 0, 0, 0, 0.001)  # a subnormal slope
    q = np.concatenate([q, special])
    d = np.concatenate([ray[:, 3:6], np.sign(special[:, 0:3]).astype(np.float64)])
    parts = []
    for node in range(len(w)):
        for t_max32 in (np.inf, 50.0, 2.0, 0.0005):
            for n_stack in (0, 1, 4, 5):
                parts.append(_items(np.full(len(q), node, dtype=np.int32), q, d, np.float32(t_max32), n_stack))
    # nothing hit with only the sentinel below (record 8, t_max32 short), then a new walk on the same lane at record 0
    parts.append(_items(np.full(len(q), 8, dtype=np.int32), q, d, np.float32(2.0), 0, second=0))
    parts.append(_items(np.full(len(q), 0, dtype=np.int32), q, d, np.float32(np.inf), 3, second=5))
    items = np.concatenate(parts)
    _compare(rtsr, workdir, "synthetic4", "step4", w, levels, items)
    # four identical boxes: equal keys, so the order is the slots' -- slot 0 next, then 1, 2, 3 from the top of the stack down
    exe = cc.build_host_check(workdir, False)
    one = _items(np.array([0], dtype=np.int32), q[:1], d[:1], np.float32(np.inf), 0)
    cur, n, slots = cc.host_steps(exe, workdir, "identical", "step4", True, levels, w, one)
    L = wt.make_leaf
    assert (int(cur[0]), int(n[0]), slots[0, :4].tolist()) == (L(0, 1), 4, [wt.EMPTY, L(3, 1), L(2, 1), L(1, 1)])
    dcur, dn, dslots = rtsr.device_walk_steps("step4", True, w, levels, one)
    assert (int(dcur[0]), int(dn[0]), dslots[0, :4].tolist()) == (L(0, 1), 4, [wt.EMPTY, L(3, 1), L(2, 1), L(1, 1)])
    # the fast mode's compilation runs the same step on the same data
    sub = items[:: max(1, len(items) // 20000)]
    for bottom in (False, True):
        a = rtsr.device_walk_steps("step4", bottom, w, levels, sub, f32=False)
        b = rtsr.device_walk_steps("step4", bottom, w, levels, sub, f32=True)
        live = np.arange(levels)[None, :] < a[1][:, None]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(np.where(live, a[2][:, :levels], 0), np.where(live, b[2][:, :levels], 0))


def test_the_hooks_refuse_what_could_leave_the_stack(rtsr):
    w = _synthetic_wide()
    one = np.zeros(1, dtype=rtsr.WALK_STEP_ITEM)
    one["second_node"] = -1
    for change, levels in ((("n_stack", 9), 9), (("node", 9), 9), (("node", -1), 9), (("second_node", 9), 9), (("n_stack", 0), 61), (("n_stack", 0), 0)):
        it = one.copy()
        it[change[0]] = change[1]
        with pytest.raises(rtsr.RtxError):
            rtsr.device_walk_steps("step4", True, w, levels, it)
    it = one.copy()
    it["n_stack"] = 9  # LdsStack takes 9 entries on 9 levels, LdsStackB (one more slot in use) does not
    rtsr.device_walk_steps("step4", False, w, 9, it)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_the_device_never_misses_a_box_the_ray_meets(rtsr, workdir, f32):
    c = cc.generate(250000 if not f32 else 320000, f32, seed=2)
    n = min(len(c["box"]), 3 * 65536)
    box, ray, touch = c["box"][:n], c["ray"][:n], c["touch"][:n]
    q = np.zeros((n, 8), dtype=np.float32)
    v = np.zeros(n, dtype=np.uint32)
    for first in range(0, n, 65536):
        sl = slice(first, first + 65536)
        q[sl], _, v[sl] = rtsr.device_cull_verdicts(box[sl], ray[sl], f32=f32)
    hq, _, hv = cc.host_verdicts(cc.build_host_check(workdir, f32), workdir, "dev_%d" % f32, box, ray)
    # the device's Ray32 is the host's but for the reciprocal: within an ulp or two in the slopes, hence in o * slope
    fin = np.isfinite(hq[:, :6]) & np.isfinite(q[:, :6])
    with np.errstate(invalid="ignore"):
        rel = np.abs(q[:, :6].astype(np.float64) - hq[:, :6]) <= 4 * 2.0 ** -23 * np.abs(hq[:, :6].astype(np.float64))
    assert (rel | ~fin).all() and np.array_equal(np.isfinite(hq[:, :6]), np.isfinite(q[:, :6]))
    assert np.array_equal(np.signbit(q[:, :3]), np.signbit(hq[:, :3])) and np.array_equal(q[:, 7], hq[:, 7])
    print("device verdict words equal to the host's: %d of %d" % (int((v == hv).sum()), n))
    miss = cc.missing_bits(v)
    idx_n = np.nonzero(~touch)[0][:6000]
    meets_n = np.array([cc.exact_meets(box[i], ray[i]) for i in idx_n])
    must = touch.copy()
    must[idx_n[meets_n]] = True
    excepted = must & c["zero_on_plane"][:n] if f32 else np.zeros(n, dtype=bool)
    bad = np.nonzero(must & ~excepted & (miss != 0))[0]
    print("must hit: %d; excepted class: %d, of which missed: %d" % (int(must.sum()), int(excepted.sum()), int((excepted & (miss != 0)).sum())))
    for i in bad[:5]:
        print("FALSE MISS bits", [cc.BITS[b] for b in range(6) if miss[i] >> b & 1], "kind", c["kind"][i], "box", box[i].tolist(), "ray", ray[i].tolist(), "q", q[i].tolist())
    assert len(bad) == 0, "%d false misses on the device" % len(bad)
    away = idx_n[~meets_n]
    print("near cases judged: %d, the exact ray misses %d; the device lets through:" % (len(idx_n), len(away)),
          {cc.BITS[b]: "%.2f %%" % (100.0 * float((v[away] >> b & 1).mean())) for b in range(6)})


@pytest.mark.parametrize("kernel,ran", [("", "k_trace_world"), ("simple", "k_trace_simple")])
def test_a_two_triangle_bvh_beside_a_sphere_bvh_under_the_wide_tree(rtsr, orc, monkeypatch, kernel, ran):
    """The world that would have had a leaf code for a BVH root, had build_bvh not forced a node (tests/wide_tree_cases.py says
    why it cannot), under RTX_WIDE=1 against the oracle, through the two walkers that take a world of two BVHs: k_trace_world,
    which the launcher chooses for it, and k_trace_simple (k_trace_vote, k_trace_lds and the wavefront integrator need a world
    of ONE BVH).  The kernel that ran is checked."""
    c = wt.case(rtsr, "two_triangle_bvh")
    cfg = rtsr.Config.new(1.0, 48, 4, 12, 4, seed=5, background=(0.55, 0.65, 0.85))
    h = rtsr.image_height(cfg)
    ref_accum, ref_rgb8 = orc.o2_render(c["flat"].arrays_ptr(), c["cam"], cfg, h, threads=8)
    assert ref_accum.std() > 0.01
    monkeypatch.setenv("RTX_WIDE", "1")
    if kernel:
        monkeypatch.setenv("RTX_TRACE_KERNEL", kernel)
    scene = c["flat"].upload()
    assert scene.array("nodes4").size > 0 and scene.wide_levels() >= 3
    screen = scene.render(c["cam"], cfg, want_stats=True)
    assert rtsr.trace_kernel_name(screen.stats.trace_kernel) == ran
    assert np.array_equal(screen.accum, ref_accum) and np.array_equal(screen.rgb8, ref_rgb8)
