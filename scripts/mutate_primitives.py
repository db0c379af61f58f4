"""Single-line faults seeded in the primitive tests and the transform chain, run on the CPU against tests/test_primitive_cases.py.

    python scripts/mutate_primitives.py [-j N] [fault ...]   # all faults by default, N side by side; the table goes to stdout
                                                             # (committed as profiles/primitives/mutations.txt)

Built like scripts/mutate_materials.py.  For every fault the package, oracle/, tests/ and include/ are copied to a temporary
directory, the fault is applied to the copy of core/geometry.hpp, and `pytest tests/test_primitive_cases.py -m "not gpu"` runs
in the copy: its fixtures rebuild the CPU oracle (the f64 and the f32 core) from the copy's sources.  The copied library stays
as it is (the tests use it for the scene graph and the flattener only).  No mutated code runs on a GPU; the device compiles the
same header, and tests/test_gpu_primitive_cases.py holds it to the CPU core bit for bit."""
import os, pathlib, re, shutil, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "ray-tracing-series-rust_amd"
GEOMETRY = "csrc/core/geometry.hpp"
TEST = "test_primitive_cases"

NEAR = "sqrtd) / a;\n  if (root < t_min || t_max < root) {"
FAR = "    root = (-half_b + sqrtd) / a;\n    if (root < t_min || t_max < root) return false;"
RECT_WINDOW = "if (t < t_min || t > t_max) return false;\n  real x = oa"
EXTENTS = "if (x < q.a0 || x > q.a1 || y < q.b0 || y > q.b1) return false;"
TRI_WINDOW = "if (t < t_min || t > t_max) return false;\n  Point3 p = ray_at"
EDGES = ["Vec3 c = cross(v1 - v0, p - v0);\n  if (dot(n, c) < real(0.0))", "c = cross(v2 - v1, p - v1);\n  if (dot(n, c) < real(0.0))",
         "c = cross(v0 - v2, p - v2);\n  if (dot(n, c) < real(0.0))"]
UNWIND = "  xform_record(ops[nops - 1], innermost_ray, rec);\n  for (int k = nops - 2; k >= 0; --k) {"


def _sub(old, a, b):
    assert old.count(a) == 1, (old, a)
    return (old, old.replace(a, b))


FAULTS = {
    "none": None,
    "sphere: discriminant < 0 -> <= 0": ("if (discriminant < real(0.0)) return false;\n#if defined(RT_F32)\n  // In single",
                                         "if (discriminant <= real(0.0)) return false;\n#if defined(RT_F32)\n  // In single"),
    "sphere: near root < t_min -> <=": _sub(NEAR, "root < t_min", "root <= t_min"),
    "sphere: t_max < near root -> <=": _sub(NEAR, "t_max < root", "t_max <= root"),
    "sphere: far root < t_min -> <=": _sub(FAR, "root < t_min", "root <= t_min"),
    "sphere: t_max < far root -> <=": _sub(FAR, "t_max < root", "t_max <= root"),
    "sphere: the far root's sign": _sub(FAR, "(-half_b + sqrtd)", "(-half_b - sqrtd)"),
    "sphere: / a dropped": ("  real root = (-half_b - sqrtd) / a;", "  real root = (-half_b - sqrtd);"),
    "sphere: / radius -> / fabs(radius)": ("Vec3 outward = (rec->p - v3(s.cx, s.cy, s.cz)) / s.radius;", "Vec3 outward = (rec->p - v3(s.cx, s.cy, s.cz)) / rt_fabs(s.radius);"),
    "rect: t < t_min -> <=": _sub(RECT_WINDOW, "t < t_min", "t <= t_min"),
    "rect: t > t_max -> >=": _sub(RECT_WINDOW, "t > t_max", "t >= t_max"),
    "rect: x < a0 -> <=": _sub(EXTENTS, "x < q.a0", "x <= q.a0"),
    "rect: x > a1 -> >=": _sub(EXTENTS, "x > q.a1", "x >= q.a1"),
    "rect: y < b0 -> <=": _sub(EXTENTS, "y < q.b0", "y <= q.b0"),
    "rect: y > b1 -> >=": _sub(EXTENTS, "y > q.b1", "y >= q.b1"),
    "rect: the XZ rectangle reads swapped components": (
        "return rect_core(q, r.origin.y, r.direction.y, r.origin.x, r.direction.x, r.origin.z, r.direction.z, t_min, t_max, t_out);",
        "return rect_core(q, r.origin.y, r.direction.y, r.origin.z, r.direction.z, r.origin.x, r.direction.x, t_min, t_max, t_out);"),
    "triangle: 0.0001 -> 0.001": ("if (rt_fabs(n_dot_d) < real(0.0001)) return false;", "if (rt_fabs(n_dot_d) < real(0.001)) return false;"),
    "triangle: < 0.0001 -> <=": ("if (rt_fabs(n_dot_d) < real(0.0001)) return false;", "if (rt_fabs(n_dot_d) <= real(0.0001)) return false;"),
    "triangle: fabs dropped": ("if (rt_fabs(n_dot_d) < real(0.0001)) return false;", "if (n_dot_d < real(0.0001)) return false;"),
    "triangle: t < t_min -> <=": _sub(TRI_WINDOW, "t < t_min", "t <= t_min"),
    "triangle: t > t_max -> >=": _sub(TRI_WINDOW, "t > t_max", "t >= t_max"),
    "triangle: edge 0 < 0 -> <= 0": _sub(EDGES[0], "< real(0.0)", "<= real(0.0)"),
    "triangle: edge 1 < 0 -> <= 0": _sub(EDGES[1], "< real(0.0)", "<= real(0.0)"),
    "triangle: edge 2 < 0 -> <= 0": _sub(EDGES[2], "< real(0.0)", "<= real(0.0)"),
    "triangle: the vertices of edge 1 swapped": _sub(EDGES[1], "cross(v2 - v1, p - v1)", "cross(v1 - v2, p - v1)"),
    "face: dot < 0 -> <= 0": ("bool ff = dot(r.direction, outward_normal) < real(0.0);", "bool ff = dot(r.direction, outward_normal) <= real(0.0);"),
    "translate: the sign on the way in": ("return make_ray(r.origin - load_v3(op.v), r.direction, r.time);", "return make_ray(r.origin + load_v3(op.v), r.direction, r.time);"),
    "translate: the sign on the way out": ("rec->p = rec->p + load_v3(op.v);", "rec->p = rec->p - load_v3(op.v);"),
    "rotate_y: the sine's sign on the way in": ("  real sin_t = op.v[0], cos_t = op.v[1];\n  Vec3 o = v3(", "  real sin_t = -op.v[0], cos_t = op.v[1];\n  Vec3 o = v3("),
    "rotate_y: the sine's sign on the way out": ("  real sin_t = op.v[0], cos_t = op.v[1];\n  Vec3 p = v3(", "  real sin_t = -op.v[0], cos_t = op.v[1];\n  Vec3 p = v3("),
    "chain: the innermost op re-faced against the outer ray": ("xform_record(ops[nops - 1], innermost_ray, rec);", "xform_record(ops[nops - 1], outer, rec);"),
    "chain: an outer op re-faced against the outer ray": ("    xform_record(ops[k], c, rec);", "    xform_record(ops[k], outer, rec);"),
    "chain: unwound outermost first": _sub(UNWIND, "for (int k = nops - 2; k >= 0; --k) {", "for (int k = 0; k <= nops - 2; ++k) {"),
}


def run(name):
    fault = FAULTS[name]
    root = pathlib.Path(tempfile.mkdtemp(prefix="mutate_primitives_"))
    try:
        shutil.copytree(os.path.join(REPO, PKG), root / PKG, ignore=shutil.ignore_patterns("obj", "__pycache__"))
        shutil.copytree(os.path.join(REPO, "oracle"), root / "oracle", ignore=shutil.ignore_patterns("_build", "_ref", "__pycache__"))
        shutil.copytree(os.path.join(REPO, "tests"), root / "tests", ignore=shutil.ignore_patterns("golden", "__pycache__"))
        shutil.copytree(os.path.join(REPO, "include"), root / "include")
        if fault:
            old, new = fault
            p = root / PKG / GEOMETRY
            t = p.read_text()
            assert t.count(old) == 1, (name, t.count(old))
            p.write_text(t.replace(old, new))
        os.utime(root / PKG / "lib" / "librtx_hip.so")  # newer than the copied sources: the tests' fixture does not rebuild it
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
