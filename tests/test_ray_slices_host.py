"""tests/ray_slices_host_check.cpp: the slice rule of the ray queries (csrc/host/ray_slices.hpp) swept on the host -- the
slices tile a batch in order, every column, seed and first_ray advances by its own step, NULL columns and every other field
stay, staging slices cut again into launch slices give each ray what cutting the batch directly gives, and a batch past 2^31
rays goes out in launches of 2^30.  Address arithmetic only: no GPU, no memory."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ray_slices_host_check.cpp")


def test_ray_slices_tile_a_batch_and_nest(tmp_path):
    exe = str(tmp_path / "ray_slices_host_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "ray slices host check clean" in out.stdout
