"""Instance trees on the GPU: every entry point and mode gives, bit for bit, the frame of the hoisted spelling (the members written
into the world list), which is the parent's code path, unchanged.  Scenes: tests/instance_scenes.py, N = 60 and N = 1024."""
import numpy as np
import pytest

from instance_scenes import ZOO_F32_CAPPED, ZOO_F32_EXACT, ZOO_LAYOUTS, ZOO_REFERENCE_ALONE_UNEQUAL, box_field, field_cam_cfg, member_zoo, tie_cam_cfg, tie_scene, zoo_cam_cfg

pytestmark = pytest.mark.gpu

RTX_KERNEL_SIMPLE, RTX_KERNEL_WORLD, RTX_KERNEL_NEE = 0, 6, 8
FRAMES = {60: dict(width=72, spp=16), 1024: dict(width=48, spp=16, depth=12)}


def _pair(rtsr, n, **kw):
    """(flat, scene) of the hoisted and of the instanced spelling, camera, config, height."""
    cam, cfg, h = field_cam_cfg(rtsr, n=n, **FRAMES[n])
    out = []
    for spelling in ("hoisted", "instanced"):
        b, w = box_field(rtsr, spelling, n=n, **kw)
        flat = b.flatten(w)
        out.append((b, flat, flat.upload()))
    assert out[0][1].instances()["n_trees"] == 0 and out[1][1].instances()["n_trees"] == 1
    return out[0], out[1], cam, cfg, h


@pytest.mark.parametrize("kernel", ["default", "simple"])
@pytest.mark.parametrize("n", [60, 1024])
def test_one_shot_render(rtsr, orc, monkeypatch, n, kernel):
    """rtx_render(instanced) == rtx_render(hoisted) == O2(instanced); k_trace_world by default, k_trace_simple when forced."""
    if kernel == "simple":
        monkeypatch.setenv("RTX_TRACE_KERNEL", "simple")
    (bh, fh, sh), (bi, fi, si), cam, cfg, h = _pair(rtsr, n)
    hoisted = sh.render(cam, cfg, want_stats=True)
    inst = si.render(cam, cfg, want_stats=True)
    want = RTX_KERNEL_WORLD if kernel == "default" else RTX_KERNEL_SIMPLE
    assert inst.stats.trace_kernel == want and hoisted.stats.trace_kernel == want
    o2, o2_rgb8 = orc.o2_render(fi.arrays_ptr(), cam, cfg, h, threads=16)
    bad = int((inst.accum != hoisted.accum).any(axis=2).sum())
    print("N %d %s: %d of %d pixels differ from the hoisted frame, %d from O2" % (n, kernel, bad, h * cfg.image_width,
                                                                                int((inst.accum != o2).any(axis=2).sum())))
    assert bad == 0 and np.array_equal(inst.rgb8, hoisted.rgb8)
    assert np.array_equal(inst.accum, o2) and np.array_equal(inst.rgb8, o2_rgb8)


@pytest.mark.parametrize("n", [60, 1024])
def test_shards_progressive_adaptive_multi(rtsr, n):
    """The instanced frame against the hoisted one-shot frame: three shards (each a progressive handle over its shard, the
    whole budget in one add) reassembled; a whole-image handle split 5 + 11; an adaptive until_adaptive run (frame, pixel_spp,
    samples) against the hoisted scene's; rtx_multi_render with two shards on one device."""
    (bh, fh, sh), (bi, fi, si), cam, cfg, h = _pair(rtsr, n)
    whole = sh.render(cam, cfg).accum
    # three shards reassembled
    got = np.zeros_like(whole)
    for s in range(3):
        prog = si.progressive(cam, cfg, shard=(s, 3, 1))
        prog.add(cfg.samples_per_pixel)
        got[[j for j in range(h) if j % 3 == s]] = prog.screen().accum
        del prog
    assert np.array_equal(got, whole)
    # a progressive handle split 5 + 11
    assert cfg.samples_per_pixel == 16
    prog = si.progressive(cam, cfg)
    prog.add(5)
    prog.add(11)
    assert np.array_equal(prog.screen().accum, whole)
    del prog
    # adaptive: frames, per-pixel sample counts and the sample total
    res = []
    for scene in (sh, si):
        prog = scene.progressive(cam, cfg)
        st = prog.until_adaptive(2, 2, 0.05)
        res.append((prog.screen().accum, prog.screen().rgb8, prog.pixel_spp(), st.samples))
        del prog
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert np.array_equal(res[0][2], res[1][2]) and res[0][3] == res[1][3] and res[0][3] > 0
    # rtx_multi_render: two shards on one device
    multi = rtsr.MultiScene(fi, 2, device_ids=[0, 0]).render(cam, cfg)
    assert np.array_equal(multi.accum, whole)


@pytest.mark.parametrize("n", [60, 1024])
def test_denoiser_features_and_frame(rtsr, n):
    (bh, fh, sh), (bi, fi, si), cam, cfg, h = _pair(rtsr, n)
    res = []
    for scene in (sh, si):
        prog = scene.progressive(cam, cfg)
        prog.add(cfg.samples_per_pixel)
        albedo, normal = prog.features(2)
        d = prog.denoise()
        res.append((albedo, normal, d.accum, d.rgb8))
        del prog
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
    assert res[0][0].std() > 0.0


@pytest.mark.parametrize("n", [60, 1024])
def test_light_sampling_with_the_lamp_as_a_member(rtsr, n):
    """The lamp, a plain sphere light, as the first MEMBER: an ordinary slot, so a sampled light exactly as when hoisted."""
    (bh, fh, sh), (bi, fi, si), cam, cfg, h = _pair(rtsr, n, lamp_member=True)
    assert fi.lights() == fh.lights() and fi.lights()["n_sphere_lights"] == 1
    hoisted = sh.render(cam, cfg, light_sampling=True, want_stats=True)
    inst = si.render(cam, cfg, light_sampling=True, want_stats=True)
    assert inst.stats.trace_kernel == RTX_KERNEL_NEE
    assert np.array_equal(inst.accum, hoisted.accum) and np.array_equal(inst.rgb8, hoisted.rgb8)
    assert not np.array_equal(inst.accum, si.render(cam, cfg).accum)  # the estimator did sample the lamp


def test_exact_ties_through_k_trace_world(rtsr, orc):
    cam, cfg, h = tie_cam_cfg(rtsr)
    frames = {}
    for order in ("AB", "BA"):
        b, w = tie_scene(rtsr, order, "list")
        o1, _ = orc.o1_render(b.graph_ptr(), w, cam, cfg, h, threads=8)
        b2, w2 = tie_scene(rtsr, order, "instanced")
        flat = b2.flatten(w2)
        got = flat.upload().render(cam, cfg, want_stats=True)
        assert got.stats.trace_kernel == RTX_KERNEL_WORLD
        assert np.array_equal(got.accum, o1), "order %s: %d pixels differ" % (order, int((got.accum != o1).any(axis=2).sum()))
        frames[order] = o1
    assert int((frames["AB"] != frames["BA"]).any(axis=2).sum()) > 20


@pytest.mark.parametrize("n", [60, 1024])
def test_counting_kernel(rtsr, n):
    """rtx_render_count: the same samples, rays and scatters as the hoisted spelling; at N = 1024 the rectangle tests per ray
    within the cap of the CPU test (one tenth of the hoisted scan's 6 N)."""
    (bh, fh, sh), (bi, fi, si), cam, cfg, h = _pair(rtsr, n)
    ch, ci = sh.render_count(cam, cfg), si.render_count(cam, cfg)
    for name in ("samples", "rays", "scatters"):
        assert getattr(ci, name) == getattr(ch, name) and getattr(ci, name) > 0, name
    per_ray_h, per_ray_i = ch.rect_tests / ch.rays, ci.rect_tests / ci.rays
    print("N %d: rect tests per ray hoisted %.1f, instanced %.2f (ratio %.5f)" % (n, per_ray_h, per_ray_i, per_ray_i / per_ray_h))
    assert per_ray_h >= 6 * n
    if n == 1024:
        assert per_ray_i <= 0.1 * per_ray_h
    else:
        assert per_ray_i < per_ray_h


@pytest.mark.parametrize("kernel", ["default", "simple"])
@pytest.mark.parametrize("n", [60, 1024])
def test_f32_mode_equals_the_float_oracle(rtsr, orc, monkeypatch, n, kernel):
    """The field reaches none of the platform functions (no noise, medium or image texture): tier A of
    tests/test_gpu_f32_parity.py, so the f32 kernels equal O2f bit for bit -- in both spellings."""
    if kernel == "simple":
        monkeypatch.setenv("RTX_TRACE_KERNEL", "simple")
    cam, cfg, h = field_cam_cfg(rtsr, n=n, **FRAMES[n])
    frames = []
    for spelling in ("hoisted", "instanced"):
        b, w = box_field(rtsr, spelling, n=n)
        flat = b.flatten(w)
        scene = flat.upload(f32=True)
        assert scene.is_f32
        got = scene.render(cam, cfg, want_stats=True)
        assert rtsr.trace_kernel_name(got.stats.trace_kernel) == ("k_trace_world" if kernel == "default" else "k_trace_simple")
        ref, ref8 = orc.o2f_render(flat.arrays_ptr(), cam, cfg, h, threads=16)
        bad = int((got.accum != ref).any(axis=2).sum())
        print("f32 N %d %s %s: %d of %d pixels differ from O2f" % (n, spelling, kernel, bad, h * cfg.image_width))
        assert bad == 0 and np.array_equal(got.rgb8, ref8)
        frames.append(got.accum)
    assert np.array_equal(frames[0], frames[1])


def test_the_tree_is_faster_than_the_scan_at_1024(rtsr):
    """N = 1024 at 256 x 256 x 16 spp: the instanced trace_ms is below the hoisted trace_ms of the same run (the hoisted path
    is the parent's code).  Both are warmed up once; the figures are printed."""
    cam, cfg, h = field_cam_cfg(rtsr, n=1024, width=256, spp=16, depth=30)
    cfg.aspect_ratio = 1.0
    h = rtsr.image_height(cfg)
    assert (cfg.image_width, h, cfg.samples_per_pixel) == (256, 256, 16)
    ms, frames = {}, {}
    for spelling in ("hoisted", "instanced"):
        b, w = box_field(rtsr, spelling, n=1024)
        scene = b.flatten(w).upload()
        scene.render(cam, cfg)
        runs = [scene.render(cam, cfg, want_stats=True) for _ in range(3)]
        assert runs[0].stats.trace_kernel == RTX_KERNEL_WORLD
        ms[spelling] = sorted(r.stats.trace_ms for r in runs)
        frames[spelling] = runs[0].accum
    print("trace_ms at N = 1024, 256 x 256 x 16 spp (three runs each): hoisted %s, instanced %s" % (ms["hoisted"], ms["instanced"]))
    assert np.array_equal(frames["hoisted"], frames["instanced"])
    assert ms["instanced"][-1] < ms["hoisted"][0]


# ---- the member zoo (tests/instance_scenes.py): every member kind, every slot layout, 48 x 32 x 8 spp, depth 12 ----
TREE_LAYOUTS = [l for l in ZOO_LAYOUTS if l not in ("one", "empty")]  # the layouts that leave a tree record


def _zoo_pair(rtsr, layout, f32=False):
    cam, cfg, h = zoo_cam_cfg(rtsr)
    assert (cfg.image_width, h, cfg.samples_per_pixel, cfg.max_depth) == (48, 32, 8, 12)
    out = []
    for spelling in ("hoisted", "instanced"):
        b, w = member_zoo(rtsr, spelling, layout)
        flat = b.flatten(w)
        out.append((b, flat, flat.upload(f32=f32)))
    assert out[0][1].instances()["n_trees"] == 0
    assert out[1][1].instances()["n_trees"] == {"two": 2, "one": 0, "empty": 0}.get(layout, 1)
    assert out[1][1].top_level_kinds() == out[0][1].top_level_kinds()
    return out[0], out[1], cam, cfg, h


@pytest.mark.parametrize("kernel", ["default", "simple"])
@pytest.mark.parametrize("layout", ZOO_LAYOUTS)
def test_zoo_one_shot_render(rtsr, orc, monkeypatch, layout, kernel):
    """rtx_render(instanced) == rtx_render(hoisted) == O2(instanced), frame and rgb8, bit for bit; k_trace_world by default."""
    if kernel == "simple":
        monkeypatch.setenv("RTX_TRACE_KERNEL", "simple")
    (bh, fh, sh), (bi, fi, si), cam, cfg, h = _zoo_pair(rtsr, layout)
    hoisted = sh.render(cam, cfg, want_stats=True)
    inst = si.render(cam, cfg, want_stats=True)
    want = "k_trace_world" if kernel == "default" else "k_trace_simple"
    assert rtsr.trace_kernel_name(inst.stats.trace_kernel) == want and rtsr.trace_kernel_name(hoisted.stats.trace_kernel) == want
    o2, o2_rgb8 = orc.o2_render(fi.arrays_ptr(), cam, cfg, h, threads=16)
    bad, bad_o2 = int((inst.accum != hoisted.accum).any(axis=2).sum()), int((inst.accum != o2).any(axis=2).sum())
    print("zoo %s %s: %d of %d pixels differ from the hoisted frame, %d from O2" % (layout, kernel, bad, h * cfg.image_width, bad_o2))
    assert o2.std() > 0.01
    assert bad == 0 and np.array_equal(inst.rgb8, hoisted.rgb8)
    assert bad_o2 == 0 and np.array_equal(inst.rgb8, o2_rgb8)


@pytest.mark.parametrize("layout", ZOO_LAYOUTS)
def test_zoo_light_sampling_progressive_shards_denoiser_count(rtsr, layout):
    """Every other path on the zoo, the instanced spelling against the hoisted one: light sampling (the emissive sphere is a
    member: a sampled light), a progressive handle split 3 + 5, three shards reassembled, features() and denoise(), and
    render_count's samples, rays and scatters."""
    (bh, fh, sh), (bi, fi, si), cam, cfg, h = _zoo_pair(rtsr, layout)
    whole = sh.render(cam, cfg).accum
    if layout not in ("one", "empty"):  # (there the emissive member is not in the world at all)
        assert fi.lights() == fh.lights() and fi.lights()["n_sphere_lights"] == 1
        nh = sh.render(cam, cfg, light_sampling=True, want_stats=True)
        ni = si.render(cam, cfg, light_sampling=True, want_stats=True)
        assert ni.stats.trace_kernel == RTX_KERNEL_NEE
        bad = int((ni.accum != nh.accum).any(axis=2).sum())
        print("zoo %s light sampling: %d pixels differ from the hoisted frame" % (layout, bad))
        assert bad == 0 and np.array_equal(ni.rgb8, nh.rgb8)
        assert not np.array_equal(ni.accum, whole)  # the estimator did sample the lamp
    prog = si.progressive(cam, cfg)
    prog.add(3)
    prog.add(5)
    bad = int((prog.screen().accum != whole).any(axis=2).sum())
    albedo_i, normal_i = prog.features(2)
    den_i = prog.denoise()
    del prog
    got = np.zeros_like(whole)
    for s in range(3):
        part = si.progressive(cam, cfg, shard=(s, 3, 1))
        part.add(cfg.samples_per_pixel)
        got[[j for j in range(h) if j % 3 == s]] = part.screen().accum
        del part
    bad_shards = int((got != whole).any(axis=2).sum())
    prog = sh.progressive(cam, cfg)
    prog.add(cfg.samples_per_pixel)
    albedo_h, normal_h = prog.features(2)
    den_h = prog.denoise()
    del prog
    bad_feat = int((albedo_i != albedo_h).any(axis=2).sum() + (normal_i != normal_h).any(axis=2).sum())
    bad_den = int((den_i.accum != den_h.accum).any(axis=2).sum())
    print("zoo %s: pixels differing from the hoisted spelling: progressive 3 + 5: %d, three shards: %d, features: %d, denoised: %d"
          % (layout, bad, bad_shards, bad_feat, bad_den))
    assert (bad, bad_shards, bad_feat, bad_den) == (0, 0, 0, 0) and np.array_equal(den_i.rgb8, den_h.rgb8)
    assert albedo_h.std() > 0.0
    ch, ci = sh.render_count(cam, cfg), si.render_count(cam, cfg)
    for name in ("samples", "rays", "scatters"):
        assert getattr(ci, name) == getattr(ch, name) and getattr(ci, name) > 0, name


# every other value the switch parser accepts (render.hip, read_switches): RTX_TRACE_KERNEL = vote, vote_diag, world, world_diag,
# wavefront; RTX_WIDE = 0 / 1 (any integer: non-zero is "on")
@pytest.mark.parametrize("switch", [("RTX_TRACE_KERNEL", "vote"), ("RTX_TRACE_KERNEL", "vote_diag"), ("RTX_TRACE_KERNEL", "world"),
                                    ("RTX_TRACE_KERNEL", "world_diag"), ("RTX_TRACE_KERNEL", "wavefront"), ("RTX_WIDE", "0"),
                                    ("RTX_WIDE", "1")])
def test_forced_kernels_render_the_hoisted_frame_or_refuse(rtsr, monkeypatch, switch):
    """A forced kernel or tree width on an instanced world (every layout with a tree): the hoisted frame of the default switches,
    or RTX_EUNSUPPORTED with a message -- never another frame.  Which of the two happens is printed."""
    for layout in TREE_LAYOUTS:
        monkeypatch.delenv(switch[0], raising=False)
        (bh, fh, sh), _, cam, cfg, h = _zoo_pair(rtsr, layout)
        want = sh.render(cam, cfg)
        monkeypatch.setenv(*switch)
        b, w = member_zoo(rtsr, "instanced", layout)
        scene = b.flatten(w).upload()  # (the switches are read at upload)
        try:
            got = scene.render(cam, cfg, want_stats=True)
        except rtsr.RtxError as e:
            print("zoo %s %s=%s: refused: %s" % (layout, switch[0], switch[1], e))
            assert e.status == rtsr.RTX_EUNSUPPORTED and len(str(e)) > 20
            continue
        bad = int((got.accum != want.accum).any(axis=2).sum())
        print("zoo %s %s=%s: %s, %d pixels differ from the hoisted frame" % (layout, switch[0], switch[1],
                                                                          rtsr.trace_kernel_name(got.stats.trace_kernel), bad))
        assert bad == 0 and np.array_equal(got.rgb8, want.rgb8)


def _f32_zoo_frames(rtsr, orc, kind, layout):
    """[(spelling, f32 device frame, O2f frame of the same flat scene)] of one zoo case, both spellings."""
    cam, cfg, h = zoo_cam_cfg(rtsr)
    out = []
    for spelling in ("hoisted", "instanced"):
        b, w = member_zoo(rtsr, spelling, layout, plain=(kind == "plain"))
        flat = b.flatten(w)
        scene = flat.upload(f32=True)
        assert scene.is_f32
        got = scene.render(cam, cfg, want_stats=True)
        assert rtsr.trace_kernel_name(got.stats.trace_kernel) == "k_trace_world"
        ref, ref8 = orc.o2f_render(flat.arrays_ptr(), cam, cfg, h, threads=16)
        assert ref.std() > 0.01
        out.append((spelling, got, ref, ref8))
    return out, cfg


@pytest.mark.parametrize("kind,layout", ZOO_F32_EXACT, ids=["%s-%s" % c for c in ZOO_F32_EXACT])
def test_f32_plain_zoo_equals_the_float_oracle(rtsr, orc, kind, layout):
    """Tier A of tests/test_gpu_f32_parity.py: the zoo with solid colours for its noise and image textures (checker and glass
    stay: the checker reads only the sign of sinf) reaches no platform function value, so the f32 kernel equals O2f bit for
    bit, in both spellings, in every layout without a medium -- the wrapped BVH member, the chains of 1 to 4 ops, the triangle
    BVHs and the tied faces included."""
    frames, cfg = _f32_zoo_frames(rtsr, orc, kind, layout)
    for spelling, got, ref, ref8 in frames:
        bad = int((got.accum != ref).any(axis=2).sum())
        print("f32 plain zoo %s %s: %d of %d pixels differ from O2f" % (layout, spelling, bad, ref.shape[0] * ref.shape[1]))
        assert bad == 0 and np.array_equal(got.rgb8, ref8)
    assert np.array_equal(frames[0][1].accum, frames[1][1].accum)


@pytest.mark.parametrize("kind,layout", ZOO_F32_CAPPED, ids=["%s-%s" % c for c in ZOO_F32_CAPPED])
def test_f32_textured_zoo_stays_within_the_flip_cap(rtsr, orc, kind, layout):
    """Tier B: the zoo with its noise and image textures in every layout, and the plain "pair" with its medium.  Against O2f,
    the unequal pixels (test_gpu_f32_parity.pixels_equal) stay within the cap that the two CPU builds of O2f give
    (instance_scenes.ZOO_REFERENCE_ALONE_UNEQUAL, asserted on the CPU by test_zoo_reference_alone_flip_rate; the cap rule is
    test_gpu_f32_parity.cap_pixels': max(4 x unequal, 5 pixels)); the two spellings equal each other bit for bit, since they
    run the same device arithmetic."""
    from test_gpu_f32_parity import pixels_equal
    frames, cfg = _f32_zoo_frames(rtsr, orc, kind, layout)
    for spelling, got, ref, ref8 in frames:
        unequal = ~pixels_equal(got.accum, ref, cfg.samples_per_pixel)
        cap = max(4 * ZOO_REFERENCE_ALONE_UNEQUAL[(kind, layout)], 5)
        assert cap <= 0.08 * unequal.size
        rel = abs(got.accum.mean() - ref.mean()) / ref.mean()
        print("f32 %s zoo %s %s: %d of %d pixels unequal to O2f (cap %d), %d bit-different, frame means differ by %.3g"
              % (kind, layout, spelling, int(unequal.sum()), unequal.size, cap, int((got.accum != ref).any(axis=2).sum()), rel))
        assert int(unequal.sum()) <= cap and rel <= 1e-3
    bad = int((frames[0][1].accum != frames[1][1].accum).any(axis=2).sum())
    print("f32 %s zoo %s: %d pixels differ between the spellings" % (kind, layout, bad))
    assert bad == 0 and np.array_equal(frames[0][1].rgb8, frames[1][1].rgb8)


def test_exact_ties_with_a_bvh_member_through_k_trace_world(rtsr, orc):
    """tie_scene's pair with prism B inside a BvhNode: close_member's tie rule.  Against O1 on the list, in both orders.  Only
    the top faces (y = 1) are tied, and the node's box does not end there (a ball above B makes it taller; B is narrower in z
    and stands off the floor): the reference's Aabb::hit rejects t_max <= t_min, so a BvhNode whose OWN box ends in a tied
    face never wins that tie, which conservative culling does not reproduce in either spelling."""
    cam, cfg, h = tie_cam_cfg(rtsr)
    frames = {}
    for order in ("AB", "BA"):
        worlds = {}
        for spelling in ("list", "instanced"):
            b = rtsr.Builder(3)
            red, blue, grey = b.lambertian((0.9, 0.1, 0.1)), b.lambertian((0.1, 0.1, 0.9)), b.lambertian((0.5, 0.5, 0.5))
            a_box = b.rect_prism((-1.5, 0.0, -1.0), (0.5, 1.0, 1.0), red)
            b_box = b.bvh_from_list(b.hittable_list([b.rect_prism((-0.5, 0.1, -0.9), (1.5, 1.0, 0.9), blue),
                                                     b.sphere((1.0, 1.6, 0.0), 0.3, blue)]), 0.0, 1.0)
            floor = b.xz_rect(-6.0, 6.0, -6.0, 6.0, 0.0, grey)
            pair = [a_box, b_box] if order == "AB" else [b_box, a_box]
            worlds[spelling] = (b, b.hittable_list([floor] + pair if spelling == "list" else [floor, b.instance_bvh(b.hittable_list(pair))]))
        b, w = worlds["list"]
        o1, _ = orc.o1_render(b.graph_ptr(), w, cam, cfg, h, threads=8)
        b2, w2 = worlds["instanced"]
        got = b2.flatten(w2).upload().render(cam, cfg, want_stats=True)
        assert got.stats.trace_kernel == RTX_KERNEL_WORLD
        bad = int((got.accum != o1).any(axis=2).sum())
        print("tie with a BVH member, order %s: %d pixels differ from O1 on the list" % (order, bad))
        assert bad == 0
        frames[order] = o1
    assert int((frames["AB"] != frames["BA"]).any(axis=2).sum()) > 20
