"""Single-line faults seeded in next-event estimation, run on the CPU against the comparisons of tests/test_light_cases.py.

    python scripts/mutate_light_sampling.py [fault ...]     # all faults by default; the table goes to stdout
                                                            # (committed as profiles/light_sampling/mutations.txt)

csrc/core and csrc/host are copied to a temporary directory beside a copy of tests/rays_host_check.cpp, one fault is applied
to the copy of core/integrator.hpp, the f64 host checker and the light-draw harness (tests/light_pick_host_check.cpp) are
built from the copy, and light_cases.statistical_check and exact_check run every case, light_cases.pick_check the draws.  No mutated code runs on a GPU."""
import sys, os, importlib, subprocess, shutil, tempfile, pathlib, ctypes as C
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "oracle")]
rtsr = importlib.import_module("ray-tracing-series-rust_amd")
import light_cases as lc, trace_rays_cases as tc
PKG = "ray-tracing-series-rust_amd"

FAULTS = {
    "none": None,
    "light_pdf_rect: YZ reads d.y": ("(q.axis == RECT_XZ ? d.y : d.x));", "(q.axis == RECT_XZ ? d.y : d.y));"),
    "emitted weight: balance heuristic": ("if (pl > real(0.0)) emitted = emitted * mis_power(*last_pdf, pl);",
                                          "if (pl > real(0.0)) emitted = emitted * (*last_pdf / (*last_pdf + pl));"),
    "light_pdf(origin, rec.p) swapped": ("light_pdf(sv, lv, k, ps->ray.origin, rec.p);", "light_pdf(sv, lv, k, rec.p, ps->ray.origin);"),
    "L.pmf dropped in nee_connect": ("const real p_light = L.pmf * pdf_sa;", "const real p_light = pdf_sa;"),
    "L.pmf dropped in light_pdf": ("return L.pmf * ps;", "return ps;"),
    "cone k / (1 + sqrt(1 - k)) -> k / 2": ("return k / (real(1.0) + rt_sqrt(real(1.0) - k));", "return k / real(2.0);"),
    "nee_bsdf_pdf without / length(dir)": ("const real c = dot(rec.normal, dir) / length(dir);\n  return", "const real c = dot(rec.normal, dir);\n  return"),
    "rt_fabs dropped in light_pdf_rect": ("const real dn = rt_fabs(q.axis == RECT_XY ? d.z : (q.axis == RECT_XZ ? d.y : d.x));",
                                          "const real dn = (q.axis == RECT_XY ? d.z : (q.axis == RECT_XZ ? d.y : d.x));"),
    "depth rule >= 1 -> >= 0": ("ps->depth >= 1 &&", "ps->depth >= 0 &&"),
    "light pick ul < cdf -> ul <= cdf": ("!(ul < lv.lights[k].cdf)", "!(ul <= lv.lights[k].cdf)"),
    "cone axis 0.9 test inverted": ("rt_fabs(w.x) > real(0.9) ? v3(0, 1, 0) : v3(1, 0, 0)", "rt_fabs(w.x) > real(0.9) ? v3(1, 0, 0) : v3(0, 1, 0)"),
    # beyond the issue's eleven: the (u, v) of a textured light
    "nee_connect: rectangle v reads a": ("lrec.v = (b - r.b0) / (r.b1 - r.b0);", "lrec.v = (a - r.a0) / (r.a1 - r.a0);"),
    "nee_connect: sphere (u, v) not computed": ("if (sv.materials[L.mat].needs_uv) get_sphere_uv(", "if (false) get_sphere_uv("),
}


def build_checker(fault):
    root = pathlib.Path(tempfile.mkdtemp())
    for sub in ("core", "host"):
        shutil.copytree(os.path.join(REPO, PKG, "csrc", sub), root / PKG / "csrc" / sub)
    shutil.copytree(os.path.join(REPO, "include"), root / "include")
    (root / "tests").mkdir()
    for f in ("rays_host_check.cpp", "light_pick_host_check.cpp"):
        shutil.copy(os.path.join(REPO, "tests", f), root / "tests")
    if fault:
        p = root / PKG / "csrc" / "core" / "integrator.hpp"
        t, (old, new) = open(p).read(), fault
        assert t.count(old) == 1, (old, t.count(old))
        open(p, "w").write(t.replace(old, new))
    out = str(root / "rays_host_check.so")
    subprocess.run(["g++"] + tc.CXXFLAGS + ["-shared", str(root / "tests" / "rays_host_check.cpp"), "-o", out], check=True)
    fn = C.CDLL(out).rays_host_trace
    fn.restype, fn.argtypes = C.c_int, tc._ARGS
    return {False: fn}, lc.pick_checker(root, str(root / "tests" / "light_pick_host_check.cpp"))


def run(name, fault):
    chk, pick = build_checker(fault)
    caught = lc.pick_check(rtsr, pick)
    for c in lc.CASES.values():
        b, flat = c.build(rtsr)
        trace = lc.host_tracer(chk, flat)
        lines, failed = lc.statistical_check(c, trace)
        failed += lc.exact_check(c, trace)
        caught += failed
    print("FAULT %s -> %s" % (name, "caught by %d comparison(s)" % len(caught) if caught else "SURVIVES"), flush=True)
    for f in caught:
        print("    " + f.replace("\n", " ")[:150], flush=True)
    return bool(caught)


if __name__ == "__main__":
    names = sys.argv[1:] or list(FAULTS)
    survivors = [n for n in names if not run(n, FAULTS[n]) and FAULTS[n] is not None]
    print("survivors: %s" % (survivors or "none"))
