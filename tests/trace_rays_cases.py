"""The host checker, scenes and ray sets of tests/test_trace_rays_abi.py and tests/test_gpu_trace_rays.py (a helper module,
not a test file): everything here runs on the CPU.

The judge is tests/rays_host_check.cpp built with oracle/Makefile's CXXFLAGS: once as it is (f64) and once with
o2_flat_f32.cpp's four defines (the float judge, linked to liboracle.so for oracle_f32_images).  Scenes and rays are those of
tests/cast_rays_cases.py (>= 25 % hits and >= 10 % misses per scene, by the oracle alone, under the case's own t_max); a radiance
query has no t_max, so that column serves the hit mix only."""
import ctypes as C
import os
import subprocess

import numpy as np

import cast_rays_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "rays_host_check.cpp")
ORACLE_BUILD = os.path.join(ROOT, "oracle", "_build")
# oracle/Makefile's CXXFLAGS (the O2 checker's)
CXXFLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-pthread"]
HOST_SOURCES = [os.path.join(ROOT, "ray-tracing-series-rust_amd", "csrc", "host", f)
                for f in ("scene_graph.cpp", "flatten.cpp", "bvh_build.cpp", "scenes.cpp")]
SANFLAGS = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-omit-frame-pointer",
            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-pthread"]

RAYS, SPP, DEPTH = 2000, 4, 8   # every GPU case: 2000 rays x 4 spp x depth 8
BACKGROUND = (0.7, 0.8, 1.0)
SEED = 1

_D = C.POINTER(C.c_double)
_ARGS = [C.c_void_p, C.c_int64, _D, _D, _D, C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, _D, C.c_int32, _D, _D]
_checkers = {}


def checkers(tmp_path_factory):
    """{False: the f64 judge's entry, True: the float judge's}, built once per session (needs liboracle.so: the orc fixture)."""
    if not _checkers:
        d = tmp_path_factory.mktemp("rays_host")
        out64, out32 = str(d / "rays_host_check.so"), str(d / "rays_host_check_f32.so")
        subprocess.run(["g++"] + CXXFLAGS + ["-shared", SRC, "-o", out64], check=True)
        subprocess.run(["g++"] + CXXFLAGS + ["-DRAYS_HOST_F32", "-shared", SRC, os.path.join(ORACLE_BUILD, "liboracle.so"),
                        "-Wl,-rpath," + ORACLE_BUILD, "-o", out32], check=True)
        for f32, path, name in ((False, out64, "rays_host_trace"), (True, out32, "rays_host_trace_f32")):
            fn = getattr(C.CDLL(path), name)
            fn.restype, fn.argtypes = C.c_int, _ARGS
            _checkers[f32] = fn
    return _checkers


def host_trace(chk, flat, o, d, time=None, *, spp=SPP, max_depth=DEPTH, background=BACKGROUND, seed=SEED, first_sample=0,
               first_ray=0, light_sampling=False, f32=False, into=None):
    """The judge's (sum, sumsq) of a batch; into=(S, Q): continue those sums in place (accumulate)."""
    n = len(o)
    o, d = np.ascontiguousarray(o, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
    time = None if time is None else np.ascontiguousarray(time, dtype=np.float64)
    S, Q = into if into is not None else (np.zeros((n, 3)), np.zeros((n, 3)))
    bg = np.array(background, dtype=np.float64)
    p = lambda a: a.ctypes.data_as(_D) if a is not None else None
    rc = chk[f32](flat.arrays_ptr(), n, p(o), p(d), p(time), first_ray, first_sample, spp, max_depth, 1 if into is not None else 0,
                  seed, p(bg), 1 if light_sampling else 0, p(S), p(Q))
    assert rc == 0, rc
    return S, Q


def same_bits(a, b):
    """cast_rays_cases.same_bits over whole arrays -> one boolean per ray."""
    return cc.same_bits(np.asarray(a).reshape(len(a), -1), np.asarray(b).reshape(len(b), -1))


# ---- scenes.  A case is a cast_rays_cases.Case: flat, o, d, time (2000 rays).  Boxes fitted on the CPU; check_mix holds them.
CASES = dict(cc.F64_CASES)
CASES.pop("gravity_t6.2")  # scene 8 once
# a sphere light beside a rectangle light (light sampling), and a world with an empty light table
CASES["simple_light"] = lambda r: cc._catalogue(r, "simple_light", r.SCENE_SIMPLE_LIGHT, (-6.0, -1.0, -6.0), (6.0, 9.0, 6.0), 1.0, seed=9)
CASES["book1"] = lambda r: cc._catalogue(r, "book1", r.SCENE_BOOK1_CANONICAL, (-12.0, -1.0, -12.0), (12.0, 14.0, 12.0), 1.0, seed=8)
CASES.update(cc.F32_CASES)
F64_CHECKED = ("cornell_smoke", "book2", "moving_test", "gravity_t0.37", "mesh_room", "zoo_middle", "zoo_two")
_built = {}


def case(rtsr, orc, name):
    """The named case with its rays and the oracle's first-hit records (built once); no device is touched."""
    if name not in _built:
        c = CASES[name](rtsr).build_rays(orc)
        # under the case's own t_max (Book-2's fog holds every unbounded ray): the records cast_rays_cases' guarantee is about
        c.first_hits = cc.records(orc, c, c.o, c.d, c.time, c.t_max, 1, 0)
        assert c.n == RAYS
        _built[name] = c
    return _built[name]


def gravity_time_limit():
    """table_len * 0.001 + 10 with the table of GravitySphere::new (time0 = 0 for every sphere of scene 8), rebuilt here."""
    t, table_len = 0.0, 1
    while t < 100.0:
        t += 0.001
        table_len += 1
    return table_len * 0.001 + 10.0


def batch_mean_and_se(S, Q, spp):
    """Per channel: the batch-mean radiance of a ray set and its standard error, from the per-ray sums and sums of squares
    (per-ray variance of the mean (Q - S^2 / spp) / (spp - 1) / spp; the rays are independent)."""
    S, Q = np.asarray(S, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    var_of_mean = np.maximum(Q - S * S / spp, 0.0) / (spp - 1) / spp
    return (S / spp).mean(axis=0), np.sqrt(var_of_mean.sum(axis=0)) / len(S)
