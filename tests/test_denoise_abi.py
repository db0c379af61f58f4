"""Denoising's C ABI and Python surface, without a GPU: symbols, struct layout, argument checks, app flags."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "ray-tracing-series-rust_amd", "lib", "rtx_render")
DENOISE = ["rtx_progressive_features", "rtx_progressive_denoise", "rtx_device_denoise"]


def test_denoise_symbols_are_declared_exported_and_bound(rtsr):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtx_abi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(rtsr.LIB_PATH)
    for name in DENOISE:
        assert name in declared and hasattr(lib, name) and name in rtsr.ABI, name
    assert "} RtxDenoiseParams;" in text
    assert rtsr.lib.rtx_abi_version() == 1
    blob = open(rtsr.LIB_PATH, "rb").read()
    for kernel in (b"k_features", b"k_denoise_prepare", b"k_denoise_level"):
        assert kernel in blob, kernel


def test_denoise_params_layout(rtsr):
    s = rtsr.RtxDenoiseParams
    assert C.sizeof(s) == 40
    assert [(n, getattr(s, n).offset) for n, _ in s._fields_] == [
        ("iterations", 0), ("feature_spp", 4), ("demodulate", 8), ("reserved", 12), ("sigma_luminance", 16),
        ("sigma_normal", 24), ("sigma_albedo", 32)]


def _host(rtsr, w=2, h=1):
    n = w * h * 3
    D, F = C.c_double * n, C.c_float * n
    return dict(m=D(*[0.5] * n), v=D(*[0.01] * n), a=F(*[0.5] * n), nrm=F(*[0.0, 0.0, 1.0] * (w * h)), om=D(),
                o8=(C.c_uint8 * n)())


BAD_PARAMS = [dict(iterations=9), dict(iterations=-1), dict(feature_spp=65), dict(feature_spp=-2), dict(demodulate=2),
              dict(demodulate=-2), dict(sigma_luminance=-1.0), dict(sigma_normal=float("nan")),
              dict(sigma_albedo=-math.inf), dict(sigma_luminance=math.inf), dict(sigma_albedo=1.5e30)]


@pytest.mark.parametrize("params", BAD_PARAMS)
def test_bad_parameters_are_rejected_without_a_device(rtsr, params):
    b = _host(rtsr)
    prm = rtsr.denoise_params(**params)
    st = rtsr.lib.rtx_device_denoise(b["m"], b["v"], b["a"], b["nrm"], 2, 1, C.byref(prm), b["om"], b["o8"])
    assert st == rtsr.RTX_EINVAL, params
    # on a NULL handle the handle is what gets reported; a live handle needs a device (tests/test_gpu_denoise.py)
    assert rtsr.lib.rtx_progressive_denoise(None, C.byref(prm), None, None) == rtsr.RTX_EINVAL


def test_null_arguments_are_rejected_without_a_device(rtsr):
    lib = rtsr.lib
    b = _host(rtsr)
    good = [b["m"], b["v"], b["a"], b["nrm"], 2, 1, None, b["om"], b["o8"]]
    for k in range(4):
        args = list(good)
        args[k] = None
        assert lib.rtx_device_denoise(*args) == rtsr.RTX_EINVAL, k
        assert "NULL" in rtsr.last_error()
    for w, h in ((0, 1), (1, 0), (-3, 2), (1 << 16, 1 << 15)):
        args = list(good)
        args[4], args[5] = w, h
        assert lib.rtx_device_denoise(*args) == rtsr.RTX_EINVAL, (w, h)
    f = (C.c_float * 6)()
    assert lib.rtx_progressive_denoise(None, None, None, None) == rtsr.RTX_EINVAL
    assert "NULL handle" in rtsr.last_error()
    assert lib.rtx_progressive_features(None, 4, f, f) == rtsr.RTX_EINVAL
    assert "NULL handle" in rtsr.last_error()


def test_python_front_ends_exist(rtsr):
    for name in ("features", "denoise"):
        assert callable(getattr(rtsr.Progressive, name, None)), name
    assert callable(getattr(rtsr, "device_denoise", None))
    import inspect
    assert inspect.signature(rtsr.render_scene_progressive).parameters["denoise"].default is False
    with pytest.raises(TypeError):
        rtsr.denoise_params(sigma=1.0)
    prm = rtsr.denoise_params(iterations=3, sigma_albedo=0.5)
    assert (prm.iterations, prm.feature_spp, prm.demodulate, prm.sigma_albedo, prm.sigma_normal) == (3, 0, 0, 0.5, 0.0)


BASE = ["--scene", "10", "--width", "16", "--spp", "8"]


@pytest.mark.parametrize("args,message", [
    (["--denoise"], "--denoise needs --batch"),
    (["--denoise", "--batch", "4"], "go together"),
    (["--denoise", "--target-error", "0.1"], "go together"),
    (["--batch", "4", "--target-error", "0.1", "--noisy-out", "n.ppm"], "need --denoise"),
    (["--batch", "4", "--target-error", "0.1", "--albedo-out", "a.ppm"], "need --denoise"),
    (["--batch", "4", "--target-error", "0.1", "--normal-out", "n.ppm"], "need --denoise"),
    (["--normal-out", "n.ppm"], "need --denoise"),
    (["--denoise", "--batch", "4", "--target-error", "0.1", "--row-chunk-compat"], "no --row-chunk-compat")])
def test_app_rejects_incomplete_denoise_flags(tmp_path, args, message):
    assert os.path.exists(APP), "apps/rtx_render was not built (python __graft_entry__.py)"
    res = subprocess.run([APP] + BASE + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    # the flags are known (an app without them stops at "unknown argument") and the combination is what is refused
    assert res.returncode == 2 and message in res.stderr and "unknown argument" not in res.stderr, (res.returncode, res.stderr)
    assert not any(os.scandir(str(tmp_path)))  # nothing written
