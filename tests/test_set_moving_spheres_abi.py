"""The prototypes of the four rtx_*_moving_sphere* entries in include/rtx_abi.h, the argument checks that need no scene, and
the ValueErrors of the Python layer.  No GPU: the resident entries are given a scene pointer that is never read -- a block of
poison bytes, which must come back untouched -- because everything here is refused (or is n = 0) before the handle is looked at."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from mover_update_cases import CASES, update_of
from update_cases import call_set_prims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rtx_flat_moving_sphere_ids", "rtx_flat_set_moving_spheres", "rtx_scene_set_moving_spheres", "rtx_scene_set_moving_spheres_device")


def _poison():
    return (C.c_uint8 * 256)(*([0xA5] * 256))


def test_the_header_declares_what_the_bindings_call(rtsr):
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtx_abi.h")).read())
    for proto in ("int64_t rtx_flat_moving_sphere_ids(const rtx_flat* f, const rtx_builder* b, rtx_handle object, int32_t* ids, int64_t cap);",
                  "rtx_status rtx_flat_set_moving_spheres(rtx_flat* f, const int32_t* ids, int64_t n, const double* movers);",
                  "rtx_status rtx_scene_set_moving_spheres(rtx_scene* s, const int32_t* ids, int64_t n, const double* movers, void* hip_stream);",
                  "rtx_status rtx_scene_set_moving_spheres_device(rtx_scene* s, const int32_t* ids, int64_t n, const double* d_movers, void* hip_stream);"):
        assert proto in text, proto
    assert rtsr.lib.rtx_abi_version() == 1  # everything is appended
    for name in ENTRIES:
        assert name in rtsr.ABI and hasattr(rtsr.lib, name)
    assert rtsr.ABI["rtx_flat_moving_sphere_ids"][0] is C.c_int64
    assert rtsr.SCENE_ARRAYS["moving_spheres"] == (17, 80, 44)
    assert len({v[0] for v in rtsr.SCENE_ARRAYS.values()}) == len(rtsr.SCENE_ARRAYS)  # no `which` serves two arrays


@pytest.mark.parametrize("entry", ["rtx_scene_set_moving_spheres", "rtx_scene_set_moving_spheres_device"])
def test_resident_entries_refuse_before_they_read_the_scene(rtsr, entry):
    fn = getattr(rtsr.lib, entry)
    good = np.arange(14, dtype=np.float64) + 1.0  # two records
    fake = _poison()
    scene = C.cast(fake, C.c_void_p)
    assert call_set_prims(rtsr, fn, None, [0, 1], None, good, None) == rtsr.RTX_EINVAL and entry + ": the scene is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, scene, [0, 1], -1, good, None) == rtsr.RTX_EINVAL and entry + ": n < 0" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, scene, None, 2, good, None) == rtsr.RTX_EINVAL and entry + ": ids is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, scene, [0, 1], None, None, None) == rtsr.RTX_EINVAL and entry + ": movers is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, scene, [0, 1], 0, good, None) == rtsr.RTX_OK  # n = 0: nothing to do, nothing looked at
    if entry.endswith("_device"):
        two = (C.c_int32 * 2)(0, 1)
        for off in (1, 2, 4):
            assert fn(scene, two, 2, C.c_void_p(good.ctypes.data + off), None) == rtsr.RTX_EINVAL
            assert entry + ": d_movers is not 8-byte aligned" in rtsr.last_error()
    assert bytes(fake) == b"\xa5" * 256


def test_flat_entries_refuse_null_arguments(rtsr):
    good = np.arange(7, dtype=np.float64) + 1.0
    fn = rtsr.lib.rtx_flat_set_moving_spheres
    assert call_set_prims(rtsr, fn, None, [0], None, good) == rtsr.RTX_EINVAL and "rtx_flat_set_moving_spheres: the scene is NULL" in rtsr.last_error()
    b = rtsr.Builder(1)
    mover = b.moving_sphere((0.3, 0.4, 0.5), (0.3, 0.9, 0.5), 0.0, 1.0, 0.2, b.lambertian((0.5, 0.5, 0.5)))
    flat = b.flatten(b.hittable_list([mover]))
    assert call_set_prims(rtsr, fn, flat.ptr, None, 1, good) == rtsr.RTX_EINVAL and "ids is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, flat.ptr, [0], None, None) == rtsr.RTX_EINVAL and "movers is NULL" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, flat.ptr, [0], -3, good) == rtsr.RTX_EINVAL and "n < 0" in rtsr.last_error()
    assert call_set_prims(rtsr, fn, flat.ptr, [1], None, good) == rtsr.RTX_EINVAL and "the scene has 1 moving spheres" in rtsr.last_error()
    ids = rtsr.lib.rtx_flat_moving_sphere_ids
    assert ids(None, b.ptr, 0, None, 0) == -1 and "rtx_flat_moving_sphere_ids" in rtsr.last_error()
    assert ids(flat.ptr, None, 0, None, 0) == -1
    assert ids(flat.ptr, b.ptr, 0, None, 1) == -1 and ids(flat.ptr, b.ptr, 0, None, -1) == -1  # no room named / cap < 0
    assert ids(flat.ptr, b.ptr, -1, None, 0) == -1 and "handle" in rtsr.last_error()
    # which = 17 of the host arrays names its size like the others; the next number is still refused
    assert rtsr.lib.rtx_flat_array(flat.ptr, 17, None, 7) == rtsr.RTX_EINVAL and "holds 80 bytes" in rtsr.last_error()
    assert rtsr.lib.rtx_flat_array(flat.ptr, 18, None, 0) == rtsr.RTX_EINVAL and "names no host array" in rtsr.last_error()
    assert len(flat.array("moving_spheres")) == 80 and list(flat.moving_sphere_ids(b, mover)) == [0]


def test_python_layer_counts_and_types_before_the_library(rtsr):
    case = CASES["plain"](rtsr, False)
    flat = case.flatten()
    before = flat.array("moving_spheres")
    ids, vals = update_of(case, flat)
    no_scene = types.SimpleNamespace(ptr=None)  # never reached: Scene.set_moving_spheres raises before it calls the library
    for bad in (np.ones(7), np.ones((len(ids), 4)), np.ones((len(ids) + 1, 7))):
        with pytest.raises(ValueError) as e:
            flat.set_moving_spheres(ids, bad)
        assert "c0 xyz, c1 xyz, radius" in str(e.value)
        with pytest.raises(ValueError) as e:  # the ValueErrors of Scene.set_spheres
            rtsr.Scene.set_moving_spheres(no_scene, ids, bad)
        assert "c0 xyz, c1 xyz, radius" in str(e.value)
    with pytest.raises(ValueError):
        flat.set_moving_spheres(ids[:1], [["a", 0.0, 0.0, 1.0, 0.0, 0.0, 1.0]])
    import torch
    for bad in (torch.ones((len(ids), 7), dtype=torch.float64), torch.ones((len(ids), 7), dtype=torch.float32)):  # on the CPU
        with pytest.raises(ValueError) as e:
            rtsr.Scene.set_moving_spheres(no_scene, ids, bad)
        assert "contiguous float64 tensor on the GPU" in str(e.value)
    flat.set_moving_spheres([], np.zeros((0, 7)))  # n = 0
    assert np.array_equal(flat.array("moving_spheres"), before)
    flat.set_moving_spheres(ids, vals.reshape(-1))  # a flat list of 7 n values is as good as (n, 7)
    assert not np.array_equal(flat.array("moving_spheres"), before)
    with pytest.raises(rtsr.RtxError) as e:
        flat.set_moving_spheres([0, 0], np.ones((2, 7)))
    assert e.value.status == rtsr.RTX_EINVAL and "twice" in str(e.value)
