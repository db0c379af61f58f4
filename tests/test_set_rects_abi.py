"""The argument checks of rtx_flat_rect_ids, rtx_flat_set_rects, rtx_scene_set_rects and rtx_scene_set_rects_device that need no
scene, and the ValueErrors of the Python layer.  No GPU: the resident entries are given a scene pointer that is never read -- a
block of poison bytes, which must come back untouched -- because everything here is refused (or is n = 0) before the handle is
looked at."""
import ctypes as C

import numpy as np
import pytest

from rect_update_cases import CASES, update_of
from update_cases import call_set_prims


def _poison():
    return (C.c_uint8 * 256)(*([0xA5] * 256))


def test_struct_sizes_the_bindings_rely_on(rtsr):
    assert rtsr.SCENE_ARRAYS["rects"] == (19, 48, 28)
    for name in ("rtx_flat_rect_ids", "rtx_flat_set_rects", "rtx_scene_set_rects", "rtx_scene_set_rects_device"):
        assert name in rtsr.ABI and hasattr(rtsr.lib, name)
    assert rtsr.ABI["rtx_flat_rect_ids"][0] is C.c_int64 and rtsr.lib.rtx_abi_version() == 1


@pytest.mark.parametrize("entry", ["rtx_scene_set_rects", "rtx_scene_set_rects_device"])
def test_resident_entries_refuse_before_they_read_the_scene(rtsr, entry):
    fn = getattr(rtsr.lib, entry)
    good = np.arange(10, dtype=np.float64) + 1.0
    fake = _poison()
    scene = C.cast(fake, C.c_void_p)
    assert call_set_prims(rtsr, fn, None, [0, 1], None, good, None) == rtsr.RTX_EINVAL and entry + ": the scene is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, scene, [0, 1], -1, good, None) == rtsr.RTX_EINVAL and entry + ": n < 0" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, scene, None, 2, good, None) == rtsr.RTX_EINVAL and entry + ": ids is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, scene, [0, 1], None, None, None) == rtsr.RTX_EINVAL and entry + ": rects is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, scene, [0, 1], 0, good, None) == rtsr.RTX_OK  # n = 0: nothing to do, nothing looked at
    if entry.endswith("_device"):
        two = (C.c_int32 * 2)(0, 1)
        for off in (1, 2, 4):
            assert fn(scene, two, 2, C.c_void_p(good.ctypes.data + off), None) == rtsr.RTX_EINVAL
            assert entry + ": d_rects is not 8-byte aligned" in rtsr.last_error()
    assert bytes(fake) == b"\xa5" * 256


def test_flat_entries_refuse_null_arguments_and_which_19_names_its_size(rtsr):
    good = np.arange(10, dtype=np.float64) + 1.0
    fn = rtsr.lib.rtx_flat_set_rects
    assert call_set_prims(rtsr, fn, None, [0, 1], None, good) == rtsr.RTX_EINVAL and "rtx_flat_set_rects: the scene is NULL" in rtsr.last_error()
    b = rtsr.Builder(1)
    flat = b.flatten(b.hittable_list([b.xy_rect(0.1, 0.9, 0.2, 0.8, 0.5, b.lambertian((0.5, 0.5, 0.5)))]))
    assert call_set_prims(rtsr, fn, flat.ptr, None, 1, good) == rtsr.RTX_EINVAL and "ids is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, flat.ptr, [0], None, None) == rtsr.RTX_EINVAL and "rects is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, flat.ptr, [0], -3, good) == rtsr.RTX_EINVAL and "n < 0" in rtsr.last_error()
    ids = rtsr.lib.rtx_flat_rect_ids
    assert ids(None, b.ptr, 0, None, 0) == -1 and "rtx_flat_rect_ids" in rtsr.last_error()
    assert ids(flat.ptr, None, 0, None, 0) == -1
    assert ids(flat.ptr, b.ptr, 0, None, 1) == -1 and ids(flat.ptr, b.ptr, 0, None, -1) == -1  # no room named / cap < 0
    assert ids(flat.ptr, b.ptr, -1, None, 0) == -1 and "handle" in rtsr.last_error()
    assert rtsr.lib.rtx_flat_array(flat.ptr, 19, None, 7) == rtsr.RTX_EINVAL and "holds 48 bytes" in rtsr.last_error()
    assert rtsr.lib.rtx_flat_array(flat.ptr, 18, None, 0) == rtsr.RTX_EINVAL and "names no host array" in rtsr.last_error()
    assert len(flat.array("rects")) == 48


def test_python_layer_counts_and_types_before_the_library(rtsr):
    case = CASES["walls"](rtsr, False)
    flat = case.flatten()
    before = flat.array("rects")
    ids, vals = update_of(case, flat)
    for bad in (np.ones(5), np.ones((len(ids), 4)), np.ones((len(ids) + 1, 5))):
        with pytest.raises(ValueError) as e:
            flat.set_rects(ids, bad)
        assert "a0 a1 b0 b1 k" in str(e.value)
    with pytest.raises(ValueError):
        flat.set_rects(ids[:1], [["a", 0.0, 0.0, 1.0, 1.0]])
    flat.set_rects([], np.zeros((0, 5)))  # n = 0
    assert np.array_equal(flat.array("rects"), before)
    flat.set_rects(ids, vals.reshape(-1))  # a flat list of 5 n values is as good as (n, 5)
    assert not np.array_equal(flat.array("rects"), before)
    with pytest.raises(rtsr.RtxError) as e:
        flat.set_rects([0, 0], np.ones((2, 5)))
    assert e.value.status == rtsr.RTX_EINVAL and "twice" in str(e.value)
