"""Ray queries' C ABI and Python surface, without a GPU: struct layouts, rtx_ray_batch_defaults, the argument checks of
rtx_scene_cast_rays / rtx_scene_cast_rays_device (which return before any device call) and Scene.cast_rays' own checks."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rtx_ray_batch_defaults", "rtx_scene_cast_rays", "rtx_scene_cast_rays_device"]


def test_symbols_are_declared_exported_and_bound(rtsr):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx_abi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(rtsr.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in rtsr.ABI, name
    blob = open(rtsr.LIB_PATH, "rb").read()
    assert b"_ZN3rtx11k_cast_rays" in blob and b"_ZN5rtx3211k_cast_rays" in blob  # both compilations carry the kernel
    assert "RTX_CAST_HOST_SLICE 262144" in text  # the bound on the host entry's staging the header states


def test_struct_layouts(rtsr):
    b, h = rtsr.RtxRayBatch, rtsr.RtxRayHits
    assert C.sizeof(b) == 72 and C.sizeof(h) == 40
    assert [(n, getattr(b, n).offset) for n, _ in b._fields_] == [
        ("n", 0), ("origin", 8), ("direction", 16), ("time", 24), ("t_max", 32), ("t_min", 40), ("t_max_all", 48),
        ("seed", 56), ("stream_step", 64)]
    assert [(n, getattr(h, n).offset) for n, _ in h._fields_] == [("t", 0), ("p", 8), ("normal", 16), ("uv", 24), ("ids", 32)]
    assert rtsr.RAY_COLUMNS == tuple(n for n, _ in h._fields_)


def test_defaults(rtsr):
    b = rtsr.RtxRayBatch(7, 1, 2, 3, 4, -1.0, -2.0, 99, 5)
    rtsr.lib.rtx_ray_batch_defaults(C.byref(b))
    assert (b.n, b.origin, b.direction, b.time, b.t_max) == (0, None, None, None, None)
    assert b.t_min == 0.001 and b.t_max_all == math.inf and b.seed == 1 and b.stream_step == 0
    rtsr.lib.rtx_ray_batch_defaults(None)  # a no-op


def _batch(rtsr, **kw):
    b = rtsr.RtxRayBatch()
    rtsr.lib.rtx_ray_batch_defaults(C.byref(b))
    o = np.zeros((4, 3))
    b.n, b.origin, b.direction = 4, o.ctypes.data, o.ctypes.data
    for k, v in kw.items():
        setattr(b, k, v)
    return b, o


@pytest.mark.parametrize("entry", ["rtx_scene_cast_rays", "rtx_scene_cast_rays_device"])
def test_argument_errors_before_any_device_call(rtsr, entry):
    fn = getattr(rtsr.lib, entry)
    call = (lambda s, b, h: fn(s, b, h, None)) if entry.endswith("_device") else fn
    bogus = C.c_void_p(1)  # never dereferenced: every case below is refused by the argument checks
    hits = rtsr.RtxRayHits()
    good, keep = _batch(rtsr)
    cases = [(None, C.byref(good), C.byref(hits), "scene"), (bogus, None, C.byref(hits), "rays"), (bogus, C.byref(good), None, "hits")]
    for field, kw in (("n", {"n": -1}), ("origin", {"origin": None}), ("direction", {"direction": None}),
                      ("t_min", {"t_min": math.nan}), ("t_max_all", {"t_max_all": math.nan})):
        bad, _ = _batch(rtsr, **kw)
        cases.append((bogus, C.byref(bad), C.byref(hits), field))
    for s, b, h, field in cases:
        assert call(s, b, h) == rtsr.RTX_EINVAL, field
        msg = rtsr.last_error()
        assert entry + ":" in msg and field in msg, (field, msg)
    # n = 0 is legal whatever the pointers are: RTX_OK, nothing launched (there is no device here), nothing written
    empty, _ = _batch(rtsr, n=0, origin=None, direction=None)
    assert call(bogus, C.byref(empty), C.byref(hits)) == rtsr.RTX_OK


def _scene_without_device(rtsr):
    """A Scene object that owns no handle: Scene.cast_rays checks its arrays before it touches the handle."""
    s = object.__new__(rtsr.Scene)
    s._p = None
    return s


def test_python_rejects_bad_arrays(rtsr):
    s = _scene_without_device(rtsr)
    o, d = np.zeros((8, 3)), np.ones((8, 3))
    bad = [
        ("origins", dict(origins=o.astype(np.float32), directions=d)),
        ("directions", dict(origins=o, directions=d.astype(np.float32))),
        ("origins", dict(origins=np.zeros((8, 6))[:, ::2], directions=d)),           # not contiguous
        ("directions", dict(origins=o, directions=np.asfortranarray(d))),
        ("directions", dict(origins=o, directions=np.ones((7, 3)))),                 # mismatched lengths
        ("times", dict(origins=o, directions=d, times=np.zeros(9))),
        ("t_max", dict(origins=o, directions=d, t_max=np.zeros(8, dtype=np.float32))),
        ("t_max", dict(origins=o, directions=d, t_max=np.zeros(16)[::2])),
        ("origins", dict(origins=np.zeros((8, 2)), directions=d)),                   # wrong width
        ("times", dict(origins=o, directions=d, times=np.zeros((8, 1)))),
        ("origins", dict(origins=[[0.0, 0.0, 0.0]] * 8, directions=d)),              # not an array
        ("want", dict(origins=o, directions=d, want=("t", "depth"))),
    ]
    for name, kw in bad:
        with pytest.raises(ValueError) as e:
            s.cast_rays(**kw)
        assert str(e.value).startswith(name + ":"), (name, str(e.value))


def test_binding_loads_without_torch():
    """A child interpreter in which `import torch` fails imports the binding and reaches Scene.cast_rays' numpy checks."""
    code = (
        "import sys, importlib\n"
        "sys.modules['torch'] = None  # any `import torch` now raises ImportError\n"
        "sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "rtsr = importlib.import_module('ray-tracing-series-rust_amd')\n"
        "assert len(rtsr.RAY_COLUMNS) == 5 and rtsr.lib.rtx_abi_version() == 1\n"
        "s = object.__new__(rtsr.Scene)\n"
        "s._p = None\n"
        "try:\n"
        "    s.cast_rays(np.zeros((4, 3), dtype=np.float32), np.ones((4, 3)))\n"
        "except ValueError as e:\n"
        "    assert str(e).startswith('origins:'), str(e)\n"
        "else:\n"
        "    raise AssertionError('no ValueError')\n"
        "assert sys.modules['torch'] is None\n"
        "print('loaded without torch')\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and "loaded without torch" in out.stdout, out.stderr


def test_device_entry_names_a_misaligned_column(rtsr):
    """rtx_scene_cast_rays_device stores uv as double2 and ids as int4: a pointer that is not 16-byte aligned (8 for the other
    columns) is RTX_EINVAL naming the column, before any device call (the scene pointer is never dereferenced)."""
    bogus = C.c_void_p(1)
    good, keep = _batch(rtsr)
    for field, address in (("uv", 0x1008), ("ids", 0x1004), ("ids", 0x1008), ("t", 0x1004), ("p", 0x1002), ("normal", 0x1004)):
        hits = rtsr.RtxRayHits()
        setattr(hits, field, address)
        assert rtsr.lib.rtx_scene_cast_rays_device(bogus, C.byref(good), C.byref(hits), None) == rtsr.RTX_EINVAL, field
        msg = rtsr.last_error()
        assert "rtx_scene_cast_rays_device:" in msg and "hits->" + field in msg and "aligned" in msg, (field, msg)
    bad, _ = _batch(rtsr, time=keep.ctypes.data + 4)
    assert rtsr.lib.rtx_scene_cast_rays_device(bogus, C.byref(bad), C.byref(rtsr.RtxRayHits()), None) == rtsr.RTX_EINVAL
    assert "rays->time" in rtsr.last_error()
