"""Mutations of the culling code, run on the CPU against the comparisons of the new tests.

    python scripts/mutate_culling.py steps      # the walk steps: scripts/step_emulator.cpp built from a mutated copy of the step
                                                # functions' text, in place of rtx_device_walk_steps under tests/test_gpu_cull_steps.py
    python scripts/mutate_culling.py collapse   # host/wide_tree.hpp mutated, tests/wide_tree_host_check.cpp + test_wide_tree.audit

No mutated code runs on a GPU: a mutated step may store outside its stack (the emulator gives every lane wide margins and
reports a store into them as a spoilt guard slot)."""
import sys, os, re, importlib, subprocess, shutil, tempfile, pathlib, traceback
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "oracle")]
rtsr = importlib.import_module("ray-tracing-series-rust_amd")
import cull_cases as cc, wide_tree_cases as wt
import test_gpu_cull_steps as T, test_wide_tree as TW
SRC = os.path.join(REPO, "ray-tracing-series-rust_amd", "csrc")

def extract_steps(text):
    a = text.index("template <class STACK>\n__device__ __forceinline__ void walk_node_step32")
    b = text.index("// tri_base >= 0:")
    c = text.index("// One wide step: test the four child boxes")
    d = text.index("// Persistent waves with path regeneration")
    return text[a:b] + text[c:d]

def build_emulator(workdir, mutate=None):
    root = pathlib.Path(workdir)
    for sub in ("core", "host"):
        shutil.copytree(os.path.join(SRC, sub), root / sub.upper(), dirs_exist_ok=True)
    tv = open(os.path.join(SRC, "hip/trace_vote.inc")).read()
    files = {"steps.inc": extract_steps(tv), "CORE/cull32.hpp": open(root / "CORE/cull32.hpp").read(), "HOST/wide_tree.hpp": open(root / "HOST/wide_tree.hpp").read()}
    if mutate:
        f, old, new = mutate
        assert files[f].count(old) >= 1, (f, old, files[f].count(old))
        files[f] = files[f].replace(old, new)
    for f, t in files.items():
        open(root / f, "w").write(t)
    for sub in ("CORE", "HOST"):  # fix relative includes between the copies
        for p in (root / sub).glob("*.hpp"):
            t = open(p).read().replace('"../core/', '"../CORE/').replace('"../host/', '"../HOST/')
            open(p, "w").write(t)
    shutil.copy(os.path.join(REPO, "scripts", "step_emulator.cpp"), root / "emul_main.cpp")
    shutil.copy(os.path.join(REPO, "include", "rtx_abi.h"), root / "rtx_abi.h")
    exe = str(root / "emul")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wno-unused-function", "-I", str(root), str(root / "emul_main.cpp"), "-o", exe], check=True)
    return exe

def step_tests(exe_emul, wd):
    def fake_steps(kind, bottom, nodes, levels, items, f32=False):
        src, dst = os.path.join(wd, "e.in"), os.path.join(wd, "e.out")
        with open(src, "wb") as f:
            f.write(np.array([{"step32": 0, "step4": 1}[kind], 1 if bottom else 0, levels, len(nodes)], dtype="<i4").tobytes())
            f.write(np.array([len(items)], dtype="<i8").tobytes()); f.write(np.ascontiguousarray(nodes).tobytes()); f.write(np.ascontiguousarray(items).tobytes())
        subprocess.run([exe_emul, src, dst], check=True)
        out = np.fromfile(dst, dtype="<i4").reshape(len(items), 2 + levels + 4)
        return out[:, 0], out[:, 1], out[:, 2:]
    rtsr.device_walk_steps = fake_steps
    wdp = pathlib.Path(wd)
    exe = wt.build_host_check(wdp)
    trees = {k: wt.run_host_check(exe, wdp, k, wt.case(rtsr, k)["nodes"], wt.case(rtsr, k)["roots"]) for k in ("dragon_2000",)}
    res = {}
    for name, fn in (("test_wide_steps_on_hand_made_records_equal_their_restatement", lambda: T.test_wide_steps_on_hand_made_records_equal_their_restatement(rtsr, wdp)),
                     ("test_a_wide_step_on_every_node_of_a_tree_equals_its_restatement[dragon_2000]", lambda: T.test_a_wide_step_on_every_node_of_a_tree_equals_its_restatement(rtsr, wdp, trees, "dragon_2000")),
                     ("test_a_binary_step_on_every_node_of_a_tree_equals_its_restatement[dragon_2000]", lambda: T.test_a_binary_step_on_every_node_of_a_tree_equals_its_restatement(rtsr, wdp, "dragon_2000"))):
        try:
            fn(); res[name] = "pass"
        except AssertionError as e:
            res[name] = "FAIL " + str(e)[:90].replace("\n", " ")
    return res

def collapse_tests(mutate):
    wd = tempfile.mkdtemp()
    root = pathlib.Path(wd)
    (root / "tests").mkdir()
    shutil.copytree(SRC, root / "ray-tracing-series-rust_amd/csrc")
    shutil.copytree(os.path.join(REPO, "include"), root / "include")
    shutil.copy(os.path.join(REPO, "tests", "wide_tree_host_check.cpp"), root / "tests")
    p = root / "ray-tracing-series-rust_amd/csrc/host/wide_tree.hpp"
    t = open(p).read(); old, new = mutate
    assert t.count(old) == 1, (old, t.count(old))
    open(p, "w").write(t.replace(old, new))
    wt.ROOT = str(root)
    exe = wt.build_host_check(root)
    res = {}
    for k in ("dragon_2000", "two_bvhs", "inner_3", "comb", "ties_and_odd_areas", "coplanar"):
        c = wt.case(rtsr, k)
        try:
            wide, levels = wt.run_host_check(exe, root, k, c["nodes"], c["roots"])
            TW.audit(c["nodes"], c["nodes32"], c["roots"], wide, levels); res[k] = "pass"
        except AssertionError as e:
            res[k] = "FAIL " + str(e)[:80].replace("\n", " ")
    wt.ROOT = REPO
    return res

STEP_MUT = {
    "none": None,
    "far offset 80 - oy written as 64 - oy": ("steps.inc", "fy = *(const float4*)(base + (80u - oy))", "fy = *(const float4*)(base + (64u - oy))"),
    "tie rule flipped (k1 <= k0)": ("steps.inc", "const int b10 = k1 < k0,", "const int b10 = k1 <= k0,"),
    "clamp removed": ("steps.inc", "return __builtin_amdgcn_fmed3f(entry, t_min, 3.0e38f); }", "(void)t_min; return entry; }"),
    "ch != WALK_DONE dropped": ("steps.inc", " != WALK_DONE;", " != 0x12345678;"),
    "both store moved after the n update (step32)": ("steps.inc", "    if (both) stack.base[stack.n * TRACE_BLOCK] = cs;\n    *cur = hf ? cf : (hs ? cs : top);\n    stack.n += (int)both - (int)!(hf || hs);\n", "    *cur = hf ? cf : (hs ? cs : top);\n    stack.n += (int)both - (int)!(hf || hs);\n    if (both) stack.base[stack.n * TRACE_BLOCK] = cs;\n"),
    "wide plane pick back to d < 0 (x)": ("steps.inc", "rt::real_sign_bit(r.direction.x) * 48u", "(r.direction.x < 0.0 ? 48u : 0u)"),
}
COLLAPSE_MUT = {
    "outward rounding dropped in the collapse": ("if ((double)lo > sl[k].mn[a]) lo = std::nextafterf(lo, -INFINITY);", ""),
    "smallest-area-first": ("half_area(sl[k]) > best_area) {", "(best < 0 || half_area(sl[k]) < best_area)) {"),
    "levels = peak (stack sizing)": ("static inline int wide_stack_levels(int peak) { return peak + 1; }", "static inline int wide_stack_levels(int peak) { return peak; }"),
    "levels = peak + 2 (stack sizing)": ("static inline int wide_stack_levels(int peak) { return peak + 1; }", "static inline int wide_stack_levels(int peak) { return peak + 2; }"),
    "ties to the highest slot": ("half_area(sl[k]) > best_area) {", "half_area(sl[k]) >= best_area) {"),
}
if __name__ == "__main__":
    what = sys.argv[1]
    if what == "steps":
        for name, m in STEP_MUT.items():
            wd = tempfile.mkdtemp()
            try:
                exe = build_emulator(wd, m)
                print("MUT", name, "->", step_tests(exe, wd), flush=True)
            except Exception as e:
                print("MUT", name, "-> ERROR", repr(e)[:300], flush=True)
    else:
        for name, m in COLLAPSE_MUT.items():
            print("MUT", name, "->", collapse_tests(m), flush=True)
