"""What deforming a mesh costs on a resident scene (rtx_scene_set_triangles*), and what the refitted BVH costs a render.

    python scripts/bench_set_triangles.py [--sizes 8192,871200] [--out profiles/deform/bench_set_triangles.json]

The mesh is the procedural mesh of the dragon room (rtx_get_world_cam scene 11, bench.py's C4; mesh_triangles = N), taken out of its flattened scene and put
into a world of its own -- the mesh in a BvhNode over a ground sphere, one material -- so that the same function builds the
scene at rest and from scratch with displaced vertices.  Every vertex is displaced by a seeded smooth field of about one mean
edge length, new for every run.  Device work is timed with torch events on the stream the update is enqueued on
(RtxRenderStats.trace_ms for a render), host work with the wall clock.  Every figure is the median of 7 timed runs after 2
warm-up runs, with the min and max beside it; everything runs in one process and one call.

Measurement 1, per N: one update of EVERY triangle --
  update_device_ms          rtx_scene_set_triangles_device (vertices already on the device): the copy of the index lists,
                            k_set_prims, k_refit_bvh (and k_refit_wide where the scene has a wide tree), between two events;
  update_call_ms            wall time of that call itself (checks, plan, staging, enqueue; it does not wait);
  update_host_device_ms     the same between events for rtx_scene_set_triangles (vertices staged from the host: 72 B a triangle);
beside what the same change costs without the feature, wall time, the device idle before and after --
  rebuild_mesh_ms           rtx_triangle_mesh and the BvhNode over it;
  rebuild_flatten_sah_ms    rtx_flatten with the host SAH builder;      rebuild_flatten_gpu_ms   with gpu_builder = 1;
  rebuild_upload_ms         rtx_scene_upload of the SAH scene (the collapse of the wide tree and the plans included);
  upload_shadow_ms          the part of every f64 upload that is new with this feature: building the shadow set_triangles needs
                            (host/set_triangles.hpp), host wall time.
Measurement 2, per N: one render at 256 x 256 x 16 spp of the last displaced mesh --
  render_refit_ms           trace time on the tree REFITTED to those vertices;
  render_fresh_ms           trace time on the tree BUILT for them (host SAH);
and whether the two frames are the same bits (they must be).
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, RUNS = 2, 7
MESH_SCENE = 11  # the dragon room of the catalogue (bench.py's C4): without a PLY file its mesh is the procedural one
TRIANGLE = np.dtype([("v", np.float64, (3, 3)), ("normal", np.float64, (3,)), ("mat", np.int32), ("pad", np.int32)])


def stat(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def displaced(tris, edge, seed):
    """Every vertex moved by a smooth field of about one mean edge length (a function of position: shared corners stay shared)."""
    rng = np.random.default_rng(seed)
    k = rng.uniform(0.5, 1.5, (3, 3)) / (20.0 * edge)
    ph = rng.uniform(0.0, 6.28, 3)
    out = tris.copy()
    for a in range(3):
        out[..., a] += edge * np.sin(tris @ k[a] + ph[a])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,871200")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")

    def world_of(tris, lo):
        """lo: the lowest corner of the mesh AT REST (the ground does not move with the mesh)."""
        b = rtsr.Builder(1)
        grey, red = b.lambertian((0.5, 0.5, 0.5)), b.lambertian((0.7, 0.35, 0.3))
        mesh = b.triangle_mesh(tris.reshape(-1, 3), np.arange(3 * len(tris), dtype=np.int64).reshape(-1, 3), red)
        bvh = b.bvh_from_list(mesh, 0.0, 1.0)
        return b, b.hittable_list([b.sphere((0.0, lo[1] - 5000.0, 0.0), 5000.0, grey), bvh]), mesh

    rows = []
    stream = torch.cuda.Stream()
    for n in [int(x) for x in args.sizes.split(",")]:
        b10 = rtsr.Builder(1)
        w10, cam, _ = b10.get_world_cam(MESH_SCENE, camera_aspect=1.0, mesh_triangles=n)
        f10 = b10.flatten(w10)
        rec = f10.array("triangles").view(TRIANGLE)
        rest = rec["v"][np.argsort(f10.array("triangle_id").view(np.int32), kind="stable")].copy()
        del f10, b10
        edge = float(np.mean(np.linalg.norm(rest[:, 1] - rest[:, 0], axis=1)))
        lo = rest.reshape(-1, 3).min(axis=0) - 2.0 * edge
        b, w, mesh = world_of(rest, lo)
        flat = b.flatten(w)
        scene = flat.upload()
        ids = flat.triangle_ids(b, mesh)
        assert len(ids) == len(rest)
        ids_p = ids.ctypes.data_as(C.POINTER(C.c_int32))
        cfg = rtsr.Config.new(1.0, 256, 16, 30, 4, seed=11, background=(0.35, 0.4, 0.55))
        assert rtsr.image_height(cfg) == 256
        # what the shadow an f64 upload now keeps for set_triangles costs that upload: a refused rtx_flat_set_triangles (an id out
        # of range) builds exactly the two shadows and stops
        shadow = []
        bad_id, nine = (C.c_int32 * 1)(-1), (C.c_double * 9)()
        for k in range(WARMUP + RUNS):
            t0 = time.perf_counter()
            st = rtsr.lib.rtx_flat_set_triangles(flat.ptr, bad_id, 1, nine)
            t1 = time.perf_counter()
            assert st == rtsr.RTX_EINVAL
            if k >= WARMUP:
                shadow.append(1e3 * (t1 - t0))
        dev, call, hostdev, mesh_ms, sah, gpu, up = [], [], [], [], [], [], []
        for k in range(WARMUP + RUNS):
            moved = displaced(rest, edge, 100 + k)
            flatv = np.ascontiguousarray(moved.reshape(-1, 9))
            d_v = torch.from_numpy(flatv).cuda()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            torch.cuda.synchronize()
            e[0].record(stream)
            t0 = time.perf_counter()
            st = rtsr.lib.rtx_scene_set_triangles_device(scene.ptr, ids_p, len(ids), C.c_void_p(d_v.data_ptr()), C.c_void_p(stream.cuda_stream))
            t1 = time.perf_counter()
            e[1].record(stream)
            assert st == rtsr.RTX_OK, rtsr.last_error()
            stream.synchronize()
            e[2].record(stream)
            st = rtsr.lib.rtx_scene_set_triangles(scene.ptr, ids_p, len(ids), flatv.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(stream.cuda_stream))
            e[3].record(stream)
            assert st == rtsr.RTX_OK, rtsr.last_error()
            stream.synchronize()
            # the way to the same scene without the feature: the mesh built anew, flattened (both builders) and uploaded
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            bf, wf, _ = world_of(moved, lo)
            t3 = time.perf_counter()
            fresh_flat = bf.flatten(wf)
            t4 = time.perf_counter()
            fresh = fresh_flat.upload()
            torch.cuda.synchronize()
            t5 = time.perf_counter()
            gpu_flat = bf.flatten(wf, gpu_builder=True)
            torch.cuda.synchronize()
            t6 = time.perf_counter()
            del gpu_flat
            if k >= WARMUP:
                dev.append(e[0].elapsed_time(e[1])); call.append(1e3 * (t1 - t0)); hostdev.append(e[2].elapsed_time(e[3]))
                mesh_ms.append(1e3 * (t3 - t2)); sah.append(1e3 * (t4 - t3)); up.append(1e3 * (t5 - t4)); gpu.append(1e3 * (t6 - t5))
        refit, built = [], []
        for k in range(WARMUP + RUNS):
            a = scene.render(cam, cfg, want_stats=True)
            f = fresh.render(cam, cfg, want_stats=True)
            if k >= WARMUP:
                refit.append(a.stats.trace_ms); built.append(f.stats.trace_ms)
        row = {"triangles": len(rest), "nodes": flat.info()["n_nodes"], "wide_levels": scene.wide_levels(), "mean_edge": round(edge, 6),
               "update_device_ms": stat(dev), "update_call_ms": stat(call), "update_host_device_ms": stat(hostdev),
               "rebuild_mesh_ms": stat(mesh_ms), "rebuild_flatten_sah_ms": stat(sah), "rebuild_flatten_gpu_ms": stat(gpu), "rebuild_upload_ms": stat(up),
               "upload_shadow_ms": stat(shadow), "render": "256x256x16spp", "kernel": rtsr.trace_kernel_name(a.stats.trace_kernel),
               "render_refit_ms": stat(refit), "render_fresh_ms": stat(built), "same_frame": bool(np.array_equal(a.accum, f.accum))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del scene, fresh
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            json.dump({"warmup": WARMUP, "runs": RUNS, "rows": rows}, fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main()
