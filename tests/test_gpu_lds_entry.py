"""k_trace_lds enters its walks below a leaf-first root (csrc/hip/lds_variant.inc:
lds_entry_pair): the bounding leaf in hand and the rest of the tree on stack level 1, without the root's own step.  The worlds
of tests/lds_entry_cases.py -- every shape a root can have, cameras whose primary rays the root step would have spared the
ground or the subtree, a tie between the bounding leaf and a sphere below child 1, a time-aware instantiation with and without
a ring, a pass over the active pixels only, frames one pixel wide or high (rays that are not finite, which must still enter at
the root) -- each held to the CPU oracle O2 bit for bit on accumulators and RGB8
(tests/test_lds_entry_plan.py holds O2 to the literal oracle O1 on the same worlds).  Frames of 64 x 42 at 4 spp."""
import numpy as np
import pytest

import lds_entry_cases as ec
from test_gpu_progressive import _rel_err

pytestmark = pytest.mark.gpu

_REFS = {}


def _setup(rtsr, name, which, max_depth, spp=ec.SPP):
    b, world = ec.build(rtsr, name)
    cam = ec.camera(rtsr, which, 0.25, 0.75) if name == "moving" else ec.camera(rtsr, which)  # (a shutter inside the BVH's interval)
    cfg = rtsr.Config.new(ec.ASPECT, ec.WIDTH, spp, max_depth, 8, seed=11, background=ec.SKY)
    assert (cfg.image_width, rtsr.image_height(cfg)) == (64, 42)
    return b, b.flatten(world), cam, cfg


def _reference(rtsr, orc, key, flat, cam, cfg):
    """The oracle's frame for `key`, computed once and shared (read-only) by the cases that render the same thing."""
    if key not in _REFS:
        accum, rgb8 = orc.o2_render(flat.arrays_ptr(), cam, cfg, rtsr.image_height(cfg), threads=16)
        accum.setflags(write=False)
        rgb8.setflags(write=False)
        _REFS[key] = (accum, rgb8)
    return _REFS[key]


def _render_lds(rtsr, scene, cam, cfg):
    st = scene.render_device(cam, cfg, want_stats=True)
    assert rtsr.trace_kernel_name(st.trace_kernel) == "k_trace_lds"
    return st, scene.render(cam, cfg)


def _assert_equal(accum, rgb8, ref):
    diff = np.abs(accum - ref[0]).max(axis=2)
    assert np.array_equal(accum, ref[0]), "%d of %d pixels differ, max |d| = %g" % (int((diff > 0).sum()), diff.size, diff.max())
    assert np.array_equal(rgb8, ref[1])


@pytest.mark.parametrize("max_depth", [1, 50])
@pytest.mark.parametrize("which", ec.CAMERAS)
@pytest.mark.parametrize("name", ec.GROUND_WORLDS)
def test_leaf_first_roots(rtsr, orc, name, which, max_depth):
    """The ground and 2, 3 or 20 spheres.  `up`: no primary ray meets the ground's box, so every one of them now runs the
    ground's exact test, which finds nothing; `book1` and `grazing`: rays that miss the box of the small spheres now take one
    step at its root; depth 1 is primary rays alone, depth 50 every bounce."""
    b, flat, cam, cfg = _setup(rtsr, name, which, max_depth)
    st, screen = _render_lds(rtsr, flat.upload(), cam, cfg)
    assert st.trace_variant == 0
    _assert_equal(screen.accum, screen.rgb8, _reference(rtsr, orc, (name, which, max_depth), flat, cam, cfg))


@pytest.mark.parametrize("name", ["ground_1", "eight_equal", "twins"])
def test_other_roots_and_the_tie(rtsr, orc, name):
    """ground_1: the root's children are both leaves (the builder marks no such root leaf-first: entered at the root).
    eight_equal: no bounding primitive, an ordinary root.  twins: the bounding leaf and a sphere below child 1 are met at
    one t by every ray that meets them; the later one in the list answers, whichever is tested first."""
    for which in ("book1", "grazing"):
        b, flat, cam, cfg = _setup(rtsr, name, which, 50)
        st, screen = _render_lds(rtsr, flat.upload(), cam, cfg)
        _assert_equal(screen.accum, screen.rgb8, _reference(rtsr, orc, (name, which, 50), flat, cam, cfg))
        assert len(np.unique(screen.accum.reshape(-1, 3), axis=0)) >= 8  # (a picture, not a constant)


@pytest.mark.parametrize("name", ["ground_3", "moving"])
@pytest.mark.parametrize("width,aspect", ec.THIN_FRAMES, ids=lambda v: str(v))
def test_frames_one_pixel_wide_or_high(rtsr, orc, name, width, aspect):
    """A frame one pixel wide or high has primary rays with infinite or NaN components (u = x / 0).  Every box test rules such a
    ray out; a sphere's quadratic does not (its root is a NaN, which no range test rejects).  So those lanes must still enter at
    the root, where the ground's box spares them the ground's test."""
    b, world = ec.build(rtsr, name)
    cam = ec.camera(rtsr, "book1", 0.25, 0.75)
    cfg = rtsr.Config.new(aspect, width, ec.SPP, 50, 8, seed=11, background=ec.SKY)
    assert 1 in (cfg.image_width, rtsr.image_height(cfg))
    flat = b.flatten(world)
    st, screen = _render_lds(rtsr, flat.upload(), cam, cfg)
    _assert_equal(screen.accum, screen.rgb8, _reference(rtsr, orc, (name, "thin", width, aspect), flat, cam, cfg))


@pytest.mark.parametrize("ring", [True, False])
def test_time_aware_instantiation(rtsr, orc, monkeypatch, ring):
    """A static ground, movers and static spheres, the shutter inside the BVH's interval: time-aware boxes and every record a
    moving-sphere record (the ground too), entered below the root -- with the primary-ray ring and without."""
    if not ring:
        monkeypatch.setenv("RTX_RING", "0")
    b, flat, cam, cfg = _setup(rtsr, "moving", "book1", 50)
    st, screen = _render_lds(rtsr, flat.upload(), cam, cfg)
    assert st.trace_variant & rtsr.RTX_LDS_VARIANT_TIME_BOXES
    _assert_equal(screen.accum, screen.rgb8, _reference(rtsr, orc, ("moving", "book1", 50), flat, cam, cfg))


def test_a_pass_over_the_active_pixels(rtsr, orc):
    """Two adaptive rounds of 2 samples: the second traces only the pixels above the target (the median of the errors after the
    first, so about half of them), through the kernel's active-pixel map.  A pixel that stopped at 2 holds the oracle's frame
    at 2 spp, the others the oracle's frame at 4."""
    b, flat, cam, cfg = _setup(rtsr, "ground_3", "book1", 50)
    scene = flat.upload()
    prog = scene.progressive(cam, cfg)
    st = prog.add_adaptive(2, 2, 0.0, want_stats=True)  # (nothing done yet: nothing to retire)
    assert rtsr.trace_kernel_name(st.trace_kernel) == "k_trace_lds"
    S, Q = prog.moments()
    target = float(np.median(_rel_err(S, Q, 2)))
    st = prog.add_adaptive(2, 2, target, want_stats=True)
    assert rtsr.trace_kernel_name(st.trace_kernel) == "k_trace_lds"
    counts = prog.pixel_spp()
    stopped = counts == 2
    assert np.array_equal(counts == 4, ~stopped) and 0 < int(stopped.sum()) < counts.size
    assert st.samples == 2 * int((~stopped).sum())
    b2, flat2, cam2, cfg2 = _setup(rtsr, "ground_3", "book1", 50, spp=2)
    ref2 = _reference(rtsr, orc, ("ground_3", "book1", 50, "2 spp"), flat2, cam2, cfg2)
    ref4 = _reference(rtsr, orc, ("ground_3", "book1", 50), flat, cam, cfg)
    screen = prog.screen()
    sel = stopped[..., None]
    _assert_equal(screen.accum, screen.rgb8, (np.where(sel, ref2[0], ref4[0]), np.where(sel, ref2[1], ref4[1])))
