"""Single-line faults seeded in the texture code, run on the CPU against tests/test_texture_cases.py.

    python scripts/mutate_textures.py [-j N] [fault ...]    # all faults by default, N side by side; the table goes to stdout
                                                            # (committed as profiles/textures/mutations.txt)

For every fault the package, oracle/, tests/ and include/ are copied to a temporary directory, the fault is applied to the
copy of core/shading.hpp, core/geometry.hpp, core/vec3.hpp or host/flatten.cpp, and `pytest tests/test_texture_cases.py
-m "not gpu"` runs in the copy: its fixtures rebuild the CPU oracle and the host judges from the copy's sources.  A fault in
the core leaves the copied library as it is (the tests use it for the scene graph and the flattener only); a fault in the
flattener recompiles flatten.cpp alone and links it with the copied objects.  No mutated code runs on a GPU, and no fault
that would read outside an array is seeded (the texel index is transposed within its image, never past it).  Device-only
code (k_trace_world's LDS copies) is not mutated: its tests are the placement runs of tests/test_gpu_texture_cases.py."""
import importlib.util, os, pathlib, re, shutil, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "ray-tracing-series-rust_amd"
SHADING, GEOMETRY, VEC3, FLATTEN = "csrc/core/shading.hpp", "csrc/core/geometry.hpp", "csrc/core/vec3.hpp", "csrc/host/flatten.cpp"

FAULTS = {
    "none": None,
    "perlin: (i + di) & 255 -> i & 255": (SHADING, "pn.perm_x[(i + di) & 255u]", "pn.perm_x[i & 255u]"),
    "perlin: perm_x <-> perm_y": (SHADING, "pn.perm_x[(i + di) & 255u], (uint32_t)pn.perm_y[(j + dj) & 255u]",
                                  "pn.perm_y[(i + di) & 255u], (uint32_t)pn.perm_x[(j + dj) & 255u]"),
    "perlin: 7 octaves -> 6": (SHADING, "perlin_turbulence<COUNT>(sv.perlins[t.a], p, 7, cnt)", "perlin_turbulence<COUNT>(sv.perlins[t.a], p, 6, cnt)"),
    "perlin: rt_fabs(accum) dropped": (SHADING, "return rt_fabs(accum);", "return accum;"),
    "perlin: uu -> u": (SHADING, "(i1 * uu + (real(1.0) - i1) * (real(1.0) - uu))", "(i1 * u + (real(1.0) - i1) * (real(1.0) - u))"),
    "noise: scale * p.z -> scale * p.x": (SHADING, "rt_sin(t.scale * p.z +", "rt_sin(t.scale * p.x +"),
    "noise: sv.perlins[t.a] -> sv.perlins[0]": (SHADING, "perlin_turbulence<COUNT>(sv.perlins[t.a],", "perlin_turbulence<COUNT>(sv.perlins[0],"),
    "image: v flip dropped": (SHADING, "real vc = real(1.0) - clamp(v, real(0.0), real(1.0));", "real vc = clamp(v, real(0.0), real(1.0));"),
    "image: i <-> j in the texel index": (SHADING, "(int64_t)j * im.width + i)", "(int64_t)i * im.height + j)"),
    "image: 1 / 255 -> 1 / 256": (SHADING, "real(1.0) / real(255.0)", "real(1.0) / real(256.0)"),
    "image: first_texel ignored": (SHADING, "3 * (im.first_texel + (int64_t)j * im.width + i)", "3 * ((int64_t)j * im.width + i)"),
    "checker: < 0 -> <= 0": (SHADING, "sx * sy * sz < 0;", "sx * sy * sz <= 0;"),
    "checker: even <-> odd": (SHADING, "tex = negative ? t.b : t.a;", "tex = negative ? t.a : t.b;"),
    "flattener: needs_uv ignores the odd child": (FLATTEN, "tex_image[t] = tex_image[(size_t)tx.a] | tex_image[(size_t)tx.b];",
                                                  "tex_image[t] = tex_image[(size_t)tx.a];"),
    "XZ rectangle: v reads a": (GEOMETRY, "rec->u = ((r.origin.x + t * r.direction.x) - q.a0) / (q.a1 - q.a0);\n"
                                          "        rec->v = ((r.origin.z + t * r.direction.z) - q.b0) / (q.b1 - q.b0);",
                                "rec->u = ((r.origin.x + t * r.direction.x) - q.a0) / (q.a1 - q.a0);\n"
                                "        rec->v = ((r.origin.x + t * r.direction.x) - q.a0) / (q.a1 - q.a0);"),
    "triangle: (u, v) = (0, 0)": (GEOMETRY, "rec->u = real(1.0); rec->v = real(1.0);", "rec->u = real(0.0); rec->v = real(0.0);"),
    "clamp returns a bound for a NaN": (VEC3, "  if (x < mn) return mn;", "  if (!(x >= mn)) return mn;"),
    # beyond the issue's list: the refusal itself
    "flattener: chains of 17 admitted": (FLATTEN, "<= rt::RT_MAX_CHECKER_CHAIN) continue;", "<= rt::RT_MAX_CHECKER_CHAIN + 1) continue;"),
}


def _build_module(root):
    spec = importlib.util.spec_from_file_location("rtsr_build_copy", str(root / PKG / "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(name):
    fault = FAULTS[name]
    root = pathlib.Path(tempfile.mkdtemp(prefix="mutate_textures_"))
    try:
        keep_objs = fault is not None and fault[0] == FLATTEN
        shutil.copytree(os.path.join(REPO, PKG), root / PKG, ignore=None if keep_objs else shutil.ignore_patterns("obj", "__pycache__"))
        shutil.copytree(os.path.join(REPO, "oracle"), root / "oracle", ignore=shutil.ignore_patterns("_build", "_ref", "__pycache__"))
        shutil.copytree(os.path.join(REPO, "tests"), root / "tests", ignore=shutil.ignore_patterns("golden", "__pycache__"))
        shutil.copytree(os.path.join(REPO, "include"), root / "include")
        if fault:
            path, old, new = fault
            p = root / PKG / path
            t = p.read_text()
            assert t.count(old) == 1, (name, t.count(old))
            p.write_text(t.replace(old, new))
        lib = root / PKG / "lib" / "librtx_hip.so"
        if keep_objs:
            b = _build_module(root)
            obj = root / PKG / "lib" / "obj" / "flatten.o"
            subprocess.run([b._hipcc()] + b.flags_for(FLATTEN) + ["-c", str(root / PKG / FLATTEN), "-o", str(obj)], check=True, cwd=str(root / PKG))
            objs = [str(root / PKG / "lib" / "obj" / (os.path.basename(s).rsplit(".", 1)[0] + ".o")) for s in b.HIP_SOURCES]
            subprocess.run([b._hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared"] + objs + ["-o", str(lib)], check=True, cwd=str(root / PKG))
        os.utime(lib)  # newer than the copied sources: the tests' fixture does not rebuild it
        out = subprocess.run([sys.executable, "-m", "pytest", "tests/test_texture_cases.py", "-q", "-m", "not gpu", "-p", "no:cacheprovider"],
                             cwd=str(root), capture_output=True, text=True)
        failed = re.findall(r"^FAILED tests/test_texture_cases\.py::(\S+)", out.stdout, flags=re.M)
        errors = re.findall(r"^ERROR tests/test_texture_cases\.py::(\S+)", out.stdout, flags=re.M)
        tail = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else out.stderr.strip()[-200:]
        return name, out.returncode, failed, errors, tail
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    jobs = 4
    if args[:1] == ["-j"]:
        jobs, args = int(args[1]), args[2:]
    names = args or list(FAULTS)
    survivors = []
    with ThreadPoolExecutor(jobs) as ex:
        for name, rc, failed, errors, tail in ex.map(run, names):
            if FAULTS[name] is None:
                print("FAULT none -> %s (%s)" % ("the suite passes" if rc == 0 else "THE SUITE FAILS UNMUTATED", tail), flush=True)
                survivors += [] if rc == 0 else ["none"]
                continue
            if errors or (rc != 0 and not failed):
                print("FAULT %s -> DID NOT RUN (%s)" % (name, tail), flush=True)
                survivors.append(name)
                continue
            print("FAULT %s -> %s" % (name, "caught by %d test(s)" % len(failed) if failed else "SURVIVES"), flush=True)
            for f in failed:
                print("    " + f, flush=True)
            if not failed:
                survivors.append(name)
    print("survivors: %s" % (survivors or "none"))
    sys.exit(1 if survivors else 0)
