"""The argument checks of rtx_flat_sphere_ids, rtx_flat_set_spheres, rtx_scene_set_spheres and rtx_scene_set_spheres_device
that need no scene -- the resident ones with their triangle twins, which run the same ladder -- and the ValueErrors of the
Python layer.  No GPU: the resident entries are given a scene pointer that is
never read -- a block of poison bytes, which must come back untouched -- because everything here is refused (or is n = 0)
before the handle is looked at."""
import ctypes as C

import numpy as np
import pytest

from sphere_update_cases import CASES, update_of
from update_cases import call_set_prims


def _poison():
    return (C.c_uint8 * 256)(*([0xA5] * 256))


def test_struct_sizes_the_bindings_rely_on(rtsr):
    assert rtsr.SCENE_ARRAYS["spheres"] == (13, 40, 24) and rtsr.SCENE_ARRAYS["lights"] == (14, 40, 40)
    for name in ("rtx_flat_sphere_ids", "rtx_flat_set_spheres", "rtx_scene_set_spheres", "rtx_scene_set_spheres_device"):
        assert name in rtsr.ABI and hasattr(rtsr.lib, name)
    assert rtsr.ABI["rtx_flat_sphere_ids"][0] is C.c_int64


@pytest.mark.parametrize("entry", ["rtx_scene_set_spheres", "rtx_scene_set_spheres_device", "rtx_scene_set_triangles", "rtx_scene_set_triangles_device"])
def test_resident_entries_refuse_before_they_read_the_scene(rtsr, entry):
    """The four resident entries share one ladder: the same five calls, the values named as each entry's header names them."""
    fn = getattr(rtsr.lib, entry)
    arg = "spheres" if "spheres" in entry else "vertices"
    good = np.arange(18, dtype=np.float64) + 1.0  # two records of either kind
    fake = _poison()
    scene = C.cast(fake, C.c_void_p)
    assert call_set_prims(rtsr, fn, None, [0, 1], None, good, None) == rtsr.RTX_EINVAL and entry + ": the scene is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, scene, [0, 1], -1, good, None) == rtsr.RTX_EINVAL and entry + ": n < 0" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, scene, None, 2, good, None) == rtsr.RTX_EINVAL and entry + ": ids is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, scene, [0, 1], None, None, None) == rtsr.RTX_EINVAL and entry + ": " + arg + " is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, scene, [0, 1], 0, good, None) == rtsr.RTX_OK  # n = 0: nothing to do, nothing looked at
    if entry.endswith("_device"):
        two = (C.c_int32 * 2)(0, 1)
        for off in (1, 2, 4):
            assert fn(scene, two, 2, C.c_void_p(good.ctypes.data + off), None) == rtsr.RTX_EINVAL
            assert entry + ": d_" + arg + " is not 8-byte aligned" in rtsr.last_error()
    assert bytes(fake) == b"\xa5" * 256


def test_flat_entries_refuse_null_arguments(rtsr):
    good = np.arange(8, dtype=np.float64) + 1.0
    fn = rtsr.lib.rtx_flat_set_spheres
    assert call_set_prims(rtsr, fn, None, [0, 1], None, good) == rtsr.RTX_EINVAL and "rtx_flat_set_spheres: the scene is NULL" in rtsr.last_error()
    b = rtsr.Builder(1)
    flat = b.flatten(b.hittable_list([b.sphere((0.3, 0.4, 0.5), 0.2, b.lambertian((0.5, 0.5, 0.5)))]))
    assert call_set_prims(rtsr, fn, flat.ptr, None, 1, good) == rtsr.RTX_EINVAL and "ids is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, flat.ptr, [0], None, None) == rtsr.RTX_EINVAL and "spheres is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, flat.ptr, [0], -3, good) == rtsr.RTX_EINVAL and "n < 0" in rtsr.last_error()
    ids = rtsr.lib.rtx_flat_sphere_ids
    assert ids(None, b.ptr, 0, None, 0) == -1 and "rtx_flat_sphere_ids" in rtsr.last_error()
    assert ids(flat.ptr, None, 0, None, 0) == -1
    assert ids(flat.ptr, b.ptr, 0, None, 1) == -1 and ids(flat.ptr, b.ptr, 0, None, -1) == -1  # no room named / cap < 0
    assert ids(flat.ptr, b.ptr, -1, None, 0) == -1 and "handle" in rtsr.last_error()
    # which = 13, 14 of the host arrays name their sizes like the others
    assert rtsr.lib.rtx_flat_array(flat.ptr, 13, None, 7) == rtsr.RTX_EINVAL and "holds 40 bytes" in rtsr.last_error()
    assert rtsr.lib.rtx_flat_array(flat.ptr, 14, None, 0) == rtsr.RTX_OK  # no sampled light: an empty table
    assert len(flat.array("spheres")) == 40 and len(flat.array("lights")) == 0


def test_python_layer_counts_and_types_before_the_library(rtsr):
    case = CASES["plain"](rtsr, False)
    flat = case.flatten()
    before = flat.array("spheres")
    ids, vals = update_of(case, flat)
    for bad in (np.ones(4), np.ones((len(ids), 3)), np.ones((len(ids) + 1, 4))):
        with pytest.raises(ValueError) as e:
            flat.set_spheres(ids, bad)
        assert "cx cy cz radius" in str(e.value)
    with pytest.raises(ValueError):
        flat.set_spheres(ids[:1], [["a", 0.0, 0.0, 1.0]])
    flat.set_spheres([], np.zeros((0, 4)))  # n = 0
    assert np.array_equal(flat.array("spheres"), before)
    flat.set_spheres(ids, vals.reshape(-1))  # a flat list of 4 n values is as good as (n, 4)
    assert not np.array_equal(flat.array("spheres"), before)
    with pytest.raises(rtsr.RtxError) as e:
        flat.set_spheres([0, 0], np.ones((2, 4)))
    assert e.value.status == rtsr.RTX_EINVAL and "twice" in str(e.value)
