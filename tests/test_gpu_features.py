"""The denoiser's feature pass on the GPU (csrc/hip/denoise.inc: k_features) against its host checker
(tests/features_host_check.cpp), bit for bit at every pixel of every case of tests/features_cases.py -- silhouettes, textures,
every primitive and material kind, a lens, a shutter, media of ordinary density, an instance tree, GravitySpheres, 1 / 3 / 4 /
64 samples -- in both precisions where no platform function is reached, on a frame large enough for the second trip of the
grid-stride loop, from handles that already hold samples, and across changes of feature_spp on one handle.

(A handle over a shard refuses features() and denoise(): tests/test_denoise_abi.py and test_gpu_denoise.py::test_error_cases.)"""
import numpy as np
import pytest

import features_cases as fc
from instance_scenes import member_zoo, zoo_cam_cfg
from set_transforms_cases import build, random_values, updates_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def chk(orc, tmp_path_factory):
    return fc.checkers(tmp_path_factory)


_scenes = {}


def _scene(rtsr, name, f32=False):
    if (name, f32) not in _scenes:
        _scenes[(name, f32)] = fc.case(rtsr, name).flat.upload(f32=f32)
    return _scenes[(name, f32)]


def _assert_bit_equal(got, ref, what):
    for plane, g, r in (("albedo", got[0], ref[0]), ("normal", got[1], ref[1])):
        assert g.dtype == np.float32 and fc.same_bits(g, r), "%s, %s: %s" % (what, plane, fc.first_difference(g, r))


@pytest.mark.parametrize("name", list(fc.CASES))
def test_features_equal_the_host_checker(rtsr, chk, name):
    c = fc.case(rtsr, name)
    ref = fc.reference(chk, rtsr, name)
    prog = _scene(rtsr, name).progressive(c.cam, c.cfg)
    _assert_bit_equal(prog.features(c.spp), ref, name)
    del prog


@pytest.mark.parametrize("name", ["mesh_room", "book2"])
def test_closed_scenes_at_three_samples(rtsr, chk, name):
    """The two closed scenes take one sample as cases (no pixel of theirs can hold samples that disagree about hitting); here
    they go through the sample loop as well: three samples, against the checker at three."""
    c = fc.case(rtsr, name)
    assert c.closed and c.spp == 1
    prog = _scene(rtsr, name).progressive(c.cam, c.cfg)
    _assert_bit_equal(prog.features(3), fc.reference(chk, rtsr, name, spp=3), name + " at 3 samples")
    del prog


@pytest.mark.parametrize("name", fc.F32_EXACT)
def test_f32_features_equal_the_float_checker(rtsr, chk, name):
    """The cases that reach no platform function (no noise or image texture, no medium; tests/test_gpu_f32_parity.py draws that
    line), nor a lens or a RotateY: the f32 scene's features are the float checker's, bit for bit."""
    c = fc.case(rtsr, name)
    ref = fc.reference(chk, rtsr, name, f32=True)
    scene = _scene(rtsr, name, f32=True)
    assert scene.is_f32
    prog = scene.progressive(c.cam, c.cfg)
    _assert_bit_equal(prog.features(c.spp), ref, name + " (f32)")
    del prog


def test_large_frame_goes_round_the_pixel_loop_twice(rtsr, chk):
    import torch  # (not importorskip: this test alone covers the second trip, and must not turn into a skip)
    n_cu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    c = fc.large_case(rtsr, n_cu)
    w, h = c.cfg.image_width, c.height
    assert w * h > n_cu * 8 * 256  # features_impl caps the grid at n_cu * 8 blocks of 256 lanes: these pixels need a second trip
    ref = fc.host_features(chk, c.flat, c.cam, c.cfg, h, 1)
    scene = c.flat.upload()
    prog = scene.progressive(c.cam, c.cfg)
    got = prog.features(1)
    _assert_bit_equal(got, ref, "large frame (%d x %d, %d compute units)" % (w, h, n_cu))
    tail = slice(n_cu * 8 * 256, None)
    assert got[0].reshape(-1, 3)[tail].any()  # the second trip wrote its pixels
    del prog


@pytest.mark.parametrize("name", ["zoo", "box_media"])
def test_a_handle_that_holds_samples_returns_the_same_features(rtsr, chk, name):
    c = fc.case(rtsr, name)
    ref = fc.reference(chk, rtsr, name)
    scene = _scene(rtsr, name)
    added = scene.progressive(c.cam, c.cfg)
    added.add(3)
    _assert_bit_equal(added.features(c.spp), ref, name + " after add(3)")
    ada = scene.progressive(c.cam, c.cfg)
    ada.until_adaptive(2, 2, 0.3)
    spp = ada.pixel_spp()
    assert (spp < ada.spp_done).any() and (spp == ada.spp_done).any()  # some pixels retired, some did not
    _assert_bit_equal(ada.features(c.spp), ref, name + " after an adaptive run")
    del added, ada


def test_changing_feature_spp_on_one_handle(rtsr, chk):
    name = "textures"
    c = fc.case(rtsr, name)
    prog = _scene(rtsr, name).progressive(c.cam, c.cfg)
    for n in (4, 1, 4):
        _assert_bit_equal(prog.features(n), fc.reference(chk, rtsr, name, spp=n), "%s at %d samples" % (name, n))
    assert not fc.same_bits(fc.reference(chk, rtsr, name, spp=4)[0], fc.reference(chk, rtsr, name, spp=1)[0])
    del prog


def test_a_live_handle_keeps_the_old_pose_across_set_transforms(rtsr, chk):
    """include/rtx_abi.h (rtx_scene_set_transforms): a progressive handle made before an update holds samples of the old pose,
    and the features it has computed are those of the old pose too; a new handle sees the new pose."""
    b, world, calls = build(rtsr, lambda r: member_zoo(r, "instanced", "middle"))
    flat = b.flatten(world)
    cam, cfg, h = zoo_cam_cfg(rtsr, width=48)
    scene = flat.upload()
    old = scene.progressive(cam, cfg)
    old.add(4)
    before = old.features(4)
    den_before = old.denoise()
    _assert_bit_equal(before, fc.host_features(chk, flat, cam, cfg, h, 4), "before the update")
    upd = updates_for(flat, calls, random_values(calls, seed=19, shift=0.4))
    scene.set_transforms(upd)
    flat.set_transforms(upd)
    _assert_bit_equal(old.features(4), before, "the old handle after the update")
    den_after = old.denoise()
    assert np.array_equal(den_after.accum.view(np.uint64), den_before.accum.view(np.uint64)) and np.array_equal(den_after.rgb8, den_before.rgb8)
    new = scene.progressive(cam, cfg)
    moved = fc.host_features(chk, flat, cam, cfg, h, 4)
    assert not fc.same_bits(moved[1], before[1])
    _assert_bit_equal(new.features(4), moved, "a new handle after the update")
    del old, new
