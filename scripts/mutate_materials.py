"""Single-line faults seeded in the scatter rules and in ConstantMedium::hit, run on the CPU against tests/test_material_cases.py.

    python scripts/mutate_materials.py [-j N] [fault ...]   # all faults by default, N side by side; the table goes to stdout
                                                            # (committed as profiles/materials/mutations.txt)

Built like scripts/mutate_textures.py.  For every fault the package, oracle/, tests/ and include/ are copied to a temporary
directory, the fault is applied to the copy of core/shading.hpp, core/vec3.hpp, core/geometry.hpp, host/scene_graph.cpp or
host/flatten.cpp, and `pytest tests/test_material_cases.py -m "not gpu"` runs in the copy: its fixtures rebuild the CPU oracle
and the host judges from the copy's sources.  A fault in the core leaves the copied library as it is (the tests use it for the
scene graph and the flattener only); a fault in a host file recompiles that file alone and links it with the copied objects.
No mutated code runs on a GPU.  The device-only copies of the medium's decision in hip/trace_world.inc (medium_decide, the
fused sphere block, the f32 box in front of both) are not mutated: their tests are the frames of
tests/test_gpu_material_cases.py, which hold every list world to O1 through k_trace_world and k_trace_simple."""
import importlib.util, os, pathlib, re, shutil, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "ray-tracing-series-rust_amd"
SHADING, GEOMETRY, VEC3 = "csrc/core/shading.hpp", "csrc/core/geometry.hpp", "csrc/core/vec3.hpp"
GRAPH, FLATTEN = "csrc/host/scene_graph.cpp", "csrc/host/flatten.cpp"
TEST = "test_material_cases"

FAULTS = {
    "none": None,
    "glass: > 1.0 -> >= 1.0 in cannot_refract": (SHADING, "refraction_ratio * sin_theta > real(1.0);", "refraction_ratio * sin_theta >= real(1.0);"),
    "glass: front and back ratio swapped": (SHADING, "rec.front_face ? m.albedo[0] : m.param;", "rec.front_face ? m.param : m.albedo[0];"),
    "glass: albedo[1] <-> albedo[2]": (SHADING, "rec.front_face ? m.albedo[1] : m.albedo[2]", "rec.front_face ? m.albedo[2] : m.albedo[1]"),
    "glass: b * b4 -> b4": (SHADING, "return r0sq + (real(1.0) - r0sq) * (b * b4);", "return r0sq + (real(1.0) - r0sq) * (b4);"),
    "glass: reflect where refract": (SHADING, "direction = refract(unit_direction, rec.normal, refraction_ratio);", "direction = reflect(unit_direction, rec.normal);"),
    "glass: fmin(..., 1) dropped": (SHADING, "real cos_theta = rt_fmin(dot(-unit_direction, rec.normal), real(1.0));", "real cos_theta = dot(-unit_direction, rec.normal);"),
    "metal: > 0 -> >= 0": (SHADING, "return dot(dir, rec.normal) > real(0.0);", "return dot(dir, rec.normal) >= real(0.0);"),
    "metal: fuzz on the unit vector, not the ball sample": (SHADING, "Vec3 dir = reflected + m.param * sphere_sample;", "Vec3 dir = reflected + m.param * unit(sphere_sample);"),
    "isotropic: direction normalised": (SHADING, "*scattered = make_ray(rec.p, sphere_sample, r_in.time);", "*scattered = make_ray(rec.p, unit(sphere_sample), r_in.time);"),
    "reflect: 2 * dot -> dot": (VEC3, "return v - (real(2.0) * dot(v, n)) * n;", "return v - (dot(v, n)) * n;"),
    "refract: the sign of r_out_parallel": (VEC3, "Vec3 r_out_parallel = (-(rt_sqrt(", "Vec3 r_out_parallel = ((rt_sqrt("),
    "medium: 0.0001 -> 0.001": (GEOMETRY, "  return t + real(0.0001);", "  return t + real(0.001);"),
    "medium: t1 < 0 clamp dropped": (GEOMETRY, "      if (t1 < real(0.0)) t1 = real(0.0);\n      real ray_length", "      real ray_length"),
    "medium: fmax(rec1, t_min) -> rec1": (GEOMETRY, "real t1 = rt_fmax(rec1_t, t_min);", "real t1 = rec1_t;"),
    "medium: fmin(rec2, closest) -> rec2": (GEOMETRY, "real t2 = rt_fmin(rec2_t, closest_so_far);", "real t2 = rec2_t;"),
    "medium: ray_length dropped from the distance inside": (GEOMETRY, "real distance_inside_boundary = (t2 - t1) * ray_length;", "real distance_inside_boundary = (t2 - t1);"),
    "medium: ray_length dropped from t": (GEOMETRY, "real t = t1 + hit_distance / ray_length;", "real t = t1 + hit_distance;"),
    "medium: > -> >= in the distance test": (GEOMETRY, "if (hit_distance > distance_inside_boundary) continue;", "if (hit_distance >= distance_inside_boundary) continue;"),
    "medium: the uniform drawn before the t1 >= t2 return": (GEOMETRY, "      if (t1 >= t2) continue;\n      if (t1 < real(0.0)) t1 = real(0.0);\n      real ray_length = length(r.direction);\n"
                                                             "      real distance_inside_boundary = (t2 - t1) * ray_length;\n      real hit_distance = e->f[0] * rt_log(rng_f64(rng));",
                                                             "      real early_u = rng_f64(rng);\n      if (t1 >= t2) continue;\n      if (t1 < real(0.0)) t1 = real(0.0);\n      real ray_length = length(r.direction);\n"
                                                             "      real distance_inside_boundary = (t2 - t1) * ray_length;\n      real hit_distance = e->f[0] * rt_log(early_u);"),
    "builder: fuzz clamp dropped": (GRAPH, "m.param = fuzz < 1.0 ? fuzz : 1.0;", "m.param = fuzz;"),
    "builder: -1 / density -> 1 / density": (GRAPH, "h.f[0] = -1.0 / density;", "h.f[0] = 1.0 / density;"),
    "flattener: dielectric_constants of 1 / ir": (FLATTEN, "rt::dielectric_constants(f.param, f.albedo);", "rt::dielectric_constants(1.0 / f.param, f.albedo);"),
}


def _build_module(root):
    spec = importlib.util.spec_from_file_location("rtsr_build_copy", str(root / PKG / "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(name):
    fault = FAULTS[name]
    root = pathlib.Path(tempfile.mkdtemp(prefix="mutate_materials_"))
    try:
        keep_objs = fault is not None and fault[0] in (GRAPH, FLATTEN)
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
            src = fault[0]
            obj = root / PKG / "lib" / "obj" / (os.path.basename(src).rsplit(".", 1)[0] + ".o")
            subprocess.run([b._hipcc()] + b.flags_for(src) + ["-c", str(root / PKG / src), "-o", str(obj)], check=True, cwd=str(root / PKG))
            objs = [str(root / PKG / "lib" / "obj" / (os.path.basename(s).rsplit(".", 1)[0] + ".o")) for s in b.HIP_SOURCES]
            subprocess.run([b._hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared"] + objs + ["-o", str(lib)], check=True, cwd=str(root / PKG))
        os.utime(lib)  # newer than the copied sources: the tests' fixture does not rebuild it
        out = subprocess.run([sys.executable, "-m", "pytest", "tests/%s.py" % TEST, "-q", "-m", "not gpu", "-p", "no:cacheprovider"],
                             cwd=str(root), capture_output=True, text=True)
        failed = re.findall(r"^FAILED tests/%s\.py::(\S+)" % TEST, out.stdout, flags=re.M)
        errors = re.findall(r"^ERROR tests/%s\.py::(\S+)" % TEST, out.stdout, flags=re.M)
        tail = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else out.stderr.strip()[-200:]
        if out.returncode < 0:  # pytest died with a signal: there is no summary to read, and that is not a verdict
            errors.append("(pytest died with signal %d)" % -out.returncode)
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
            for f in failed[:6]:
                print("    " + f, flush=True)
            if len(failed) > 6:
                print("    ... and %d more" % (len(failed) - 6), flush=True)
            if not failed:
                survivors.append(name)
    print("survivors: %s" % (survivors or "none"))
    sys.exit(1 if survivors else 0)
