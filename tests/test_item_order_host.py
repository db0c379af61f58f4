"""tests/item_order_host_check.cpp: the order of a pass's items (csrc/core/item_order.hpp) swept on the host -- every
(pixel, sample) once, slot = s * npix + lp, contiguous sample-major groups, P >= npix the row-strip order, and the prepared
divisions at passes of 2^30 items.  Built plain and with the address / undefined-behaviour sanitizers; run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "item_order_host_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_item_order_maps_every_pixel_sample_pair_once(tmp_path, flags):
    exe = str(tmp_path / "item_order_host_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unused-function"] + flags + [SRC, "-o", exe], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "item order host check clean" in out.stdout and "runtime error" not in out.stderr
