"""Progressive rendering's C ABI and Python surface, without a GPU: symbols, struct layout, argument checks."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "ray-tracing-series-rust_amd", "lib", "rtx_render")
PROGRESSIVE = ["rtx_progressive_create", "rtx_progressive_destroy", "rtx_progressive_spp", "rtx_progressive_add",
               "rtx_progressive_read", "rtx_progressive_stats", "rtx_progressive_until"]


def test_progressive_symbols_are_declared_exported_and_bound(rtsr):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx_abi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(rtsr.LIB_PATH)
    for name in PROGRESSIVE:
        assert name in declared and hasattr(lib, name) and name in rtsr.ABI, name
    assert "typedef struct rtx_progressive rtx_progressive;" in text
    assert rtsr.lib.rtx_abi_version() == 1
    blob = open(rtsr.LIB_PATH, "rb").read()
    for kernel in (b"k_reduce_samples_moments", b"k_noise_stats", b"k_noise_stats_final"):
        assert kernel in blob


def test_noise_stats_layout(rtsr):
    s = rtsr.RtxNoiseStats
    assert C.sizeof(s) == 40
    assert [(n, getattr(s, n).offset) for n, _ in s._fields_] == [
        ("spp_done", 0), ("pixels", 4), ("pixels_above", 8), ("reserved", 12),
        ("max_rel_err", 16), ("mean_rel_err", 24), ("target_rel_err", 32)]


def test_null_handles_and_bad_arguments_are_rejected_without_a_device(rtsr):
    lib = rtsr.lib
    cam = rtsr.Camera.new((13, 2, 3), (0, 0, 0), (0, 1, 0), 20.0, 1.5, 0.1, 10.0, 0.0, 1.0)
    cfg = rtsr.Config.new(1.5, 16, 8, 4, 1)
    out = C.c_void_p()
    ns = rtsr.RtxNoiseStats()
    frame = rtsr.RtxFrame(None, None)
    assert lib.rtx_progressive_create(None, C.byref(cam), C.byref(cfg), None, C.byref(out)) == rtsr.RTX_EINVAL
    assert out.value is None
    assert lib.rtx_progressive_create(None, C.byref(cam), C.byref(cfg), None, None) == rtsr.RTX_EINVAL
    assert lib.rtx_progressive_add(None, 4, None, None) == rtsr.RTX_EINVAL
    assert "NULL handle" in rtsr.last_error()
    for n in (0, -3):
        assert lib.rtx_progressive_add(None, n, None, None) == rtsr.RTX_EINVAL
    assert lib.rtx_progressive_read(None, C.byref(frame), None) == rtsr.RTX_EINVAL
    assert lib.rtx_progressive_stats(None, 0.1, C.byref(ns)) == rtsr.RTX_EINVAL
    assert lib.rtx_progressive_until(None, 8, 0.1, C.byref(ns)) == rtsr.RTX_EINVAL
    assert lib.rtx_progressive_spp(None) == -1
    lib.rtx_progressive_destroy(None)  # NULL-safe


def test_python_front_ends_exist(rtsr):
    assert callable(getattr(rtsr.Scene, "progressive", None))
    for name in ("add", "screen", "moments", "stats", "until"):
        assert callable(getattr(rtsr.Progressive, name, None)), name
    assert isinstance(rtsr.Progressive.spp_done, property)
    assert callable(getattr(rtsr, "render_scene_progressive", None))


@pytest.mark.parametrize("args", [["--batch", "8"], ["--target-error", "0.1"], ["--batch", "0", "--target-error", "0.1"],
                                  ["--batch", "8", "--target-error", "0.1", "--snapshot-every", "8"]])
def test_app_rejects_incomplete_progressive_flags(tmp_path, args):
    assert os.path.exists(APP), "apps/rtx_render was not built (python __graft_entry__.py)"
    res = subprocess.run([APP, "--scene", "10", "--width", "16", "--spp", "8"] + args, capture_output=True, text=True,
                         timeout=60, cwd=str(tmp_path))
    assert res.returncode == 2 and "--" in res.stderr
