"""Occlusion queries' C ABI and Python surface without a GPU: the declarations, the argument checks of rtx_scene_occlusion /
rtx_scene_occlusion_device (which return before any device call and before the handle is read), the alignment check, n = 0 and
Scene.occlusion's own checks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rtx_scene_occlusion", "rtx_scene_occlusion_device"]


def test_symbols_are_declared_exported_and_bound(rtsr):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx_abi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(rtsr.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in rtsr.ABI, name
    vp, batch = C.c_void_p, C.POINTER(rtsr.RtxRayBatch)
    assert rtsr.ABI["rtx_scene_occlusion"] == (C.c_int32, [vp, batch, vp])
    assert rtsr.ABI["rtx_scene_occlusion_device"] == (C.c_int32, [vp, batch, vp, vp])
    assert re.search(r"rtx_status rtx_scene_occlusion\(const rtx_scene\* s, const RtxRayBatch\* rays, double\* tau\);", text)
    assert re.search(r"rtx_status rtx_scene_occlusion_device\(const rtx_scene\* s, const RtxRayBatch\* rays, double\* d_tau, void\* hip_stream\);", text)
    blob = open(rtsr.LIB_PATH, "rb").read()
    assert b"_ZN3rtx11k_occlusion" in blob and b"_ZN5rtx3211k_occlusion" in blob  # both compilations carry the kernel
    assert rtsr.lib.rtx_abi_version() == 1 and re.search(r"#define RTX_ABI_VERSION 1\b", text)


def _batch(rtsr, **kw):
    b = rtsr.RtxRayBatch()
    rtsr.lib.rtx_ray_batch_defaults(C.byref(b))
    o = np.zeros((4, 3))
    b.n, b.origin, b.direction = 4, o.ctypes.data, o.ctypes.data
    for k, v in kw.items():
        setattr(b, k, v)
    return b, o


@pytest.mark.parametrize("entry", NEW)
def test_argument_errors_before_any_device_call(rtsr, entry):
    fn = getattr(rtsr.lib, entry)
    call = (lambda s, b, t: fn(s, b, t, None)) if entry.endswith("_device") else fn
    bogus = C.c_void_p(1)  # never dereferenced: every case below is refused by the argument checks
    out = np.full(4, 7.0)
    T = out.ctypes.data
    good, keep = _batch(rtsr)
    cases = [(None, C.byref(good), T, "scene"), (bogus, None, T, "rays"), (bogus, C.byref(good), None, "tau")]
    for field, kw in (("n", {"n": -1}), ("origin", {"origin": None}), ("direction", {"direction": None}),
                      ("t_min", {"t_min": math.nan}), ("t_max_all", {"t_max_all": math.nan})):
        bad, _ = _batch(rtsr, **kw)
        cases.append((bogus, C.byref(bad), T, field))
    for s, b, t, field in cases:
        assert call(s, b, t) == rtsr.RTX_EINVAL, field
        msg = rtsr.last_error()
        assert entry + ":" in msg and field in msg, (field, msg)
    # the ladder's order: a NULL scene is named before a NULL batch, a NULL batch before a NULL tau
    assert call(None, None, None) == rtsr.RTX_EINVAL and "scene" in rtsr.last_error()
    assert call(bogus, None, None) == rtsr.RTX_EINVAL and "rays" in rtsr.last_error()
    # n = 0 is legal whatever the ray pointers are: RTX_OK, nothing launched, nothing written
    empty, _ = _batch(rtsr, n=0, origin=None, direction=None)
    assert call(bogus, C.byref(empty), T) == rtsr.RTX_OK
    assert np.array_equal(out, np.full(4, 7.0))
    # infinite bounds are not NaN: legal for the checks (n = 0, so nothing goes further)
    wide, _ = _batch(rtsr, n=0, t_min=-math.inf, t_max_all=math.inf)
    assert call(bogus, C.byref(wide), T) == rtsr.RTX_OK


def test_device_entry_names_a_misaligned_pointer(rtsr):
    bogus = C.c_void_p(1)
    out = np.zeros(6)
    T = out.ctypes.data
    good, keep = _batch(rtsr)
    fn = rtsr.lib.rtx_scene_occlusion_device
    assert fn(bogus, C.byref(good), T + 4, None) == rtsr.RTX_EINVAL
    msg = rtsr.last_error()
    assert "rtx_scene_occlusion_device:" in msg and "d_tau" in msg and "8-byte aligned" in msg, msg
    for field in ("origin", "direction", "time", "t_max"):
        bad, _ = _batch(rtsr, **{field: keep.ctypes.data + 4})
        assert fn(bogus, C.byref(bad), T, None) == rtsr.RTX_EINVAL, field
        assert "rays->" + field in rtsr.last_error() and "aligned" in rtsr.last_error()
    # the argument ladder comes first: a NULL tau is "NULL", not "aligned"; n = 0 asks for no alignment
    assert fn(bogus, C.byref(good), None, None) == rtsr.RTX_EINVAL and "NULL" in rtsr.last_error()
    empty, _ = _batch(rtsr, n=0)
    assert fn(bogus, C.byref(empty), T + 4, None) == rtsr.RTX_OK


def test_python_rejects_bad_arguments(rtsr):
    s = object.__new__(rtsr.Scene)  # owns no handle: Scene.occlusion checks its arguments before it touches the handle
    s._p = None
    o, d = np.zeros((8, 3)), np.ones((8, 3))
    bad = [
        ("origins", dict(origins=o.astype(np.float32), directions=d)),
        ("origins", dict(origins=[[0.0, 0.0, 0.0]] * 8, directions=d)),
        ("directions", dict(origins=o, directions=np.asfortranarray(d))),
        ("directions", dict(origins=o, directions=np.ones((7, 3)))),
        ("directions", dict(origins=o, directions=None)),
        ("times", dict(origins=o, directions=d, times=np.zeros(9))),
        ("times", dict(origins=o, directions=d, times=np.zeros((8, 1)))),
        ("t_max", dict(origins=o, directions=d, t_max=np.zeros(7))),
        ("t_max", dict(origins=o, directions=d, t_max=np.zeros(8, dtype=np.float32))),
        ("t_min", dict(origins=o, directions=d, t_min=math.nan)),
        ("t_max_all", dict(origins=o, directions=d, t_max_all=math.nan)),
        ("stream", dict(origins=o, directions=d, stream=5)),
    ]
    for name, kw in bad:
        with pytest.raises(ValueError) as e:
            s.occlusion(**kw)
        assert str(e.value).startswith(name + ":"), (name, str(e.value))
    for name, args in (("a", (o.astype(np.float32), d)), ("b", (o, np.ones((7, 3)))), ("eps", (o, d, 1.0)), ("eps", (o, d, -0.5))):
        with pytest.raises(ValueError) as e:
            s.occlusion_between(*args)
        assert str(e.value).startswith(name + ":"), (name, str(e.value))


def test_result_object(rtsr):
    tau = np.array([0.0, 0.5, math.inf, math.nan])
    r = rtsr.Occlusion(4, tau)
    assert r.tau is tau and r.blocked.tolist() == [False, False, True, False]
    t = r.transmittance
    assert t[0] == 1.0 and t[1] == np.exp(-0.5) and t[2] == 0.0 and np.isnan(t[3])
