"""Nearest-point queries' C ABI and Python surface without a GPU: the declarations, the struct sizes, the defaults, the argument
checks of rtx_scene_nearest / rtx_scene_nearest_device (which return before any device call and before the handle is read), the
alignment check, n = 0 and Scene.nearest's own checks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rtx_scene_nearest", "rtx_scene_nearest_device"]


def test_symbols_are_declared_exported_and_bound(rtsr):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx_abi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(rtsr.LIB_PATH)
    for name in NEW + ["rtx_point_batch_defaults"]:
        assert name in declared and hasattr(lib, name) and name in rtsr.ABI, name
    vp, batch, out = C.c_void_p, C.POINTER(rtsr.RtxPointBatch), C.POINTER(rtsr.RtxNearest)
    assert rtsr.ABI["rtx_scene_nearest"] == (C.c_int32, [vp, batch, out])
    assert rtsr.ABI["rtx_scene_nearest_device"] == (C.c_int32, [vp, batch, out, vp])
    assert re.search(r"rtx_status rtx_scene_nearest\(const rtx_scene\* s, const RtxPointBatch\* points, const RtxNearest\* out\);", text)
    blob = open(rtsr.LIB_PATH, "rb").read()
    assert b"_ZN3rtx9k_nearest" in blob and b"_ZN5rtx329k_nearest" in blob  # both compilations carry the kernel


def test_struct_sizes_and_defaults(rtsr):
    assert C.sizeof(rtsr.RtxPointBatch) == 48 and C.sizeof(rtsr.RtxNearest) == 24
    assert rtsr.RtxPointBatch.r_max_all.offset == 32 and rtsr.RtxPointBatch.media.offset == 40 and rtsr.RtxPointBatch.reserved.offset == 44
    b = rtsr.RtxPointBatch()
    C.memset(C.byref(b), 0xFF, C.sizeof(b))
    rtsr.lib.rtx_point_batch_defaults(C.byref(b))
    assert (b.n, b.points, b.time, b.r_max, b.media, b.reserved) == (0, None, None, None, 0, 0) and b.r_max_all == math.inf
    rtsr.lib.rtx_point_batch_defaults(None)  # a no-op


def _batch(rtsr, **kw):
    b = rtsr.RtxPointBatch()
    rtsr.lib.rtx_point_batch_defaults(C.byref(b))
    p = np.zeros((4, 3))
    b.n, b.points = 4, p.ctypes.data
    for k, v in kw.items():
        setattr(b, k, v)
    return b, p


def _out(rtsr, d, q, ids):
    return rtsr.RtxNearest(d.ctypes.data, q.ctypes.data, ids.ctypes.data)


@pytest.mark.parametrize("entry", NEW)
def test_argument_errors_before_any_device_call(rtsr, entry):
    fn = getattr(rtsr.lib, entry)
    call = (lambda s, b, o: fn(s, b, o, None)) if entry.endswith("_device") else fn
    bogus = C.c_void_p(1)  # never dereferenced: every case below is refused by the argument checks
    d, q, ids = np.full(4, 7.0), np.full((4, 3), 7.0), np.full((4, 4), 7, dtype=np.int32)
    out = _out(rtsr, d, q, ids)
    good, keep = _batch(rtsr)
    cases = [(None, C.byref(good), C.byref(out), "scene"), (bogus, None, C.byref(out), "points is NULL"), (bogus, C.byref(good), None, "out")]
    for field, kw in (("points->n", {"n": -1}), ("points->points", {"points": None}), ("points->r_max_all is NaN", {"r_max_all": math.nan}),
                      ("points->r_max_all < 0", {"r_max_all": -1.0}), ("points->media", {"media": 2}), ("points->media", {"media": -1}),
                      ("points->reserved", {"reserved": 1})):
        bad, _ = _batch(rtsr, **kw)
        cases.append((bogus, C.byref(bad), C.byref(out), field))
    for s, b, o, field in cases:
        assert call(s, b, o) == rtsr.RTX_EINVAL, field
        msg = rtsr.last_error()
        assert entry + ":" in msg and field in msg, (field, msg)
    # the ladder's order
    assert call(None, None, None) == rtsr.RTX_EINVAL and "scene" in rtsr.last_error()
    assert call(bogus, None, None) == rtsr.RTX_EINVAL and "points is NULL" in rtsr.last_error()
    # n = 0 is legal whatever the pointers are: RTX_OK, nothing launched, nothing written; so are all-NULL outputs
    empty, _ = _batch(rtsr, n=0, points=None)
    assert call(bogus, C.byref(empty), C.byref(out)) == rtsr.RTX_OK
    none = rtsr.RtxNearest(None, None, None)
    assert call(bogus, C.byref(empty), C.byref(none)) == rtsr.RTX_OK
    assert np.all(d == 7.0) and np.all(q == 7.0) and np.all(ids == 7)
    zero, _ = _batch(rtsr, n=0, r_max_all=0.0)
    assert call(bogus, C.byref(zero), C.byref(out)) == rtsr.RTX_OK


def test_device_entry_names_a_misaligned_pointer(rtsr):
    bogus = C.c_void_p(1)
    d, q, ids = np.zeros(6), np.zeros((6, 3)), np.zeros((6, 4), dtype=np.int32)
    base = ids.ctypes.data + (-ids.ctypes.data) % 16  # a 16-byte aligned address inside ids
    good, keep = _batch(rtsr)
    fn = rtsr.lib.rtx_scene_nearest_device
    for field, o, what in (("out->d", rtsr.RtxNearest(d.ctypes.data + 4, q.ctypes.data, base), "8-byte"),
                           ("out->q", rtsr.RtxNearest(d.ctypes.data, q.ctypes.data + 4, base), "8-byte"),
                           ("out->ids", rtsr.RtxNearest(d.ctypes.data, q.ctypes.data, base + 8), "16-byte")):
        assert fn(bogus, C.byref(good), C.byref(o), None) == rtsr.RTX_EINVAL, field
        msg = rtsr.last_error()
        assert "rtx_scene_nearest_device:" in msg and field in msg and what + " aligned" in msg, msg
    out = rtsr.RtxNearest(d.ctypes.data, q.ctypes.data, base)
    for field in ("points", "time", "r_max"):
        bad, _ = _batch(rtsr, **{field: keep.ctypes.data + 4})
        assert fn(bogus, C.byref(bad), C.byref(out), None) == rtsr.RTX_EINVAL, field
        assert "points->" + field in rtsr.last_error() and "aligned" in rtsr.last_error()
    empty, _ = _batch(rtsr, n=0)
    assert fn(bogus, C.byref(empty), C.byref(rtsr.RtxNearest(d.ctypes.data + 4, None, None)), None) == rtsr.RTX_OK


def test_python_rejects_bad_arguments(rtsr):
    s = object.__new__(rtsr.Scene)  # owns no handle: Scene.nearest checks its arguments before it touches the handle
    s._p = None
    p = np.zeros((8, 3))
    bad = [
        ("points", dict(points=p.astype(np.float32))),
        ("points", dict(points=[[0.0, 0.0, 0.0]] * 8)),
        ("points", dict(points=np.zeros((8, 2)))),
        ("times", dict(points=p, times=np.zeros(9))),
        ("r_max", dict(points=p, r_max=np.zeros(8, dtype=np.float32))),
        ("want", dict(points=p, want=("d", "normal"))),
        ("stream", dict(points=p, stream=5)),
    ]
    for name, kw in bad:
        with pytest.raises(ValueError) as e:
            s.nearest(**kw)
        assert str(e.value).startswith(name + ":"), (name, str(e.value))


def test_result_object(rtsr):
    ids = np.array([[3, 1, 2, 9], [-1, -1, -1, -1]], dtype=np.int32)
    r = rtsr.Nearest(2, {"d": np.array([1.0, math.inf]), "ids": ids})
    assert r.q is None and r.found.tolist() == [True, False] and r.n == 2
    assert (r.material.tolist(), r.slot.tolist(), r.prim_type.tolist(), r.prim_index.tolist()) == ([3, -1], [1, -1], [2, -1], [9, -1])
    assert rtsr.Nearest(0, {"d": np.zeros(0)}).found is None
