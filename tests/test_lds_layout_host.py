"""tests/lds_layout_host_check.cpp: k_trace_lds's LDS layout (csrc/hip/lds_layout.inc) swept on the host -- levels 2..64, ring
capacities {0, 32, 48, 64}, the three node record sizes, record counts up to the kernel's limits."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lds_layout_regions_are_disjoint_aligned_and_where_the_kernel_expects_them(tmp_path):
    exe = str(tmp_path / "lds_layout_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "lds_layout_host_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "lds layout host check clean" in out.stdout and "runtime error" not in out.stderr
