"""Timing of the denoiser on the Book-2 final scene: the feature pass and one a-trous level, at 1920x1080 and 3840x2160.

    python scripts/bench_denoise.py [--reps N]

Prints one JSON line.  Every time is taken with HIP events on the null stream (the stream the blocking denoise entries run
on) after a warm-up call, as the median of --reps calls:
  feature_ms    rtx_progressive_features with a feature_spp the handle does not hold yet (4 and 5 alternating), so the
                pass runs every call;
  denoise_ms[K] rtx_progressive_denoise with K levels and no host output (features cached, nothing copied back): the
                prepare kernel and K levels;
  level_ms      (denoise_ms[8] - denoise_ms[1]) / 7, the cost of one level (steps 2 .. 128; every level reads the same taps);
  prepare_ms    denoise_ms[1] - level_ms.
The byte and tap counts behind the estimates in DESIGN.md ("Denoising") come along: per level and pixel 64 B of compulsory
HBM traffic (three 16-B inputs, one 16-B output) and 25 taps x 3 16-B loads = 1200 B through the caches.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch  # first: the library then shares torch's HIP runtime (tests/conftest.py)
    torch.cuda.init()
    rtsr = importlib.import_module("ray-tracing-series-rust_amd")

    def check(status):
        if status != rtsr.RTX_OK:
            raise rtsr.RtxError(status, rtsr.last_error())

    def timed(fn):
        fn()  # warm-up
        out = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return statistics.median(out)

    b = rtsr.Builder(1)
    world, cam, bg = b.get_world_cam(rtsr.SCENE_BOOK2_FINAL)
    scene = b.flatten(world).upload()
    result = {"scene": "book2_final", "reps": args.reps, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for w, h in ((1920, 1080), (3840, 2160)):
        cfg = rtsr.Config.new(w / h, w, 2, 50, 10, seed=1, background=bg)
        prog = scene.progressive(cam, cfg)
        prog.add(2)
        flip = [4]

        def features():
            flip[0] = 9 - flip[0]  # 4, 5, 4, ...: never the feature_spp the handle holds
            check(rtsr.lib.rtx_progressive_features(prog._p, flip[0], None, None))

        feature_ms = timed(features)
        check(rtsr.lib.rtx_progressive_features(prog._p, 4, None, None))
        den = {}
        for k in (1, 2, 5, 8):
            prm = rtsr.denoise_params(iterations=k)
            den[k] = timed(lambda: check(rtsr.lib.rtx_progressive_denoise(prog._p, C.byref(prm), None, None)))
        level = (den[8] - den[1]) / 7.0
        npix = w * h
        result["sizes"]["%dx%d" % (w, h)] = {
            "feature_ms_4spp_avg_of_4_and_5": round(feature_ms, 4), "denoise_ms": {str(k): round(v, 4) for k, v in den.items()},
            "level_ms": round(level, 4), "prepare_ms": round(den[1] - level, 4),
            "hbm_bytes_per_level": 64 * npix, "cache_bytes_per_level": 1200 * npix, "taps_per_level": 25 * npix,
            "level_at_6p3_TBps_ms": round(64 * npix / 6.3e12 * 1e3, 4)}
        del prog
    print(json.dumps(result))


if __name__ == "__main__":
    main()
