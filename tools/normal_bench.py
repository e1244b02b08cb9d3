"""Time Sampler.normal_equations (olpe_normal_batch) beside Sampler.chi_squared
(olpe_chi2_batch) in EXACT mode over the same vectors in the same process.

    python tools/normal_bench.py [--vectors W] [--reps N] [--shapes 64x2,64x3,128x3]

Per shape: a synthetic cutout, W vectors scattered 1e-3 (relative) about the step-1 guess,
both calls once to warm up, then N repetitions of the two calls one after the other, the
order reversed every other repetition.  Each call is timed by the host clock from a
synchronised start to its return (it ends in a stream synchronise): upload of the vectors,
kernel, and the copy back -- W x (1 + P + P^2) doubles for the normal equations (11.8 MB at
4,096 x 19 parameters), W for chi^2 -- so the ratio is the ratio of the calls, not of the
kernels.  Prints one JSON line per call: ms, vectors/s, the FP64 lane-operations it counts
over the 39.3e12 lane-ops/s peak.  The counts per pixel: chi^2 is DESIGN.md §4's EXACT model,
21 G + G + 3; the normal equations' are read off the kernel's ISA (the pixel loop of
normal_kernel<NSRC>: 269 / 380 FP64 VALU instructions for 2 / 3 sources, all 64 lanes a
pixel each) plus the matrix core's 16 lane-FMAs per lane and v_mfma_f64_16x16x4_f64: 16 of
them per 64 pixels for 2 sources, 32 for 3 -- 256 / 512 per pixel, of which 136 / 184 entries
of the symmetric matrix are unique.  With three sources the variant that takes the 3 x 3
corner by a third MFMA (OLPE_NORMAL_CORNER=mfma, 48 per step) is timed as well.  No GPU, no
number: it fails without one.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 39.3e12                                  # FP64 lane-ops/s
VALU_PER_PIXEL = {2: 269, 3: 380}               # FP64 VALU instructions of the pixel loop
MFMA_PER_STEP = {2: 16, 3: 32}                  # per 64 pixels, 16 lane-FMAs per lane each


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="64x2,64x3,128x3")
    args = ap.parse_args(argv)
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    W = args.vectors
    for shape in args.shapes.split(","):
        n, nsrc = (int(v) for v in shape.split("x"))
        G = 2 * nsrc
        img, _ = synth.make_image(n, nsrc, 0)
        p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
        rng = np.random.RandomState(n + nsrc)
        vecs = np.tile(p0, (W, 1))
        vecs[:, :-1] *= 1.0 + 1e-3 * rng.normal(size=(W, p0.size - 1))
        ops = {"chi2": n * n * (21 * G + G + 3),
               "normal": n * n * (VALU_PER_PIXEL[nsrc] + 16 * MFMA_PER_STEP[nsrc])}
        with Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc) as s:
            s.set_eval_mode("exact")
            def corner_mfma(v):
                os.environ["OLPE_NORMAL_CORNER"] = "mfma"
                try:
                    return s.normal_equations(v)
                finally:
                    del os.environ["OLPE_NORMAL_CORNER"]
            calls = {"chi2": s.chi_squared, "normal": s.normal_equations}
            if nsrc == 3:                       # the 3 x 3 corner by a third MFMA (A/B)
                calls["normal_corner_mfma"] = corner_mfma
                ops["normal_corner_mfma"] = ops["normal"] + n * n * 16 * 16
                corner_mfma(vecs)
            chi = calls["chi2"](vecs)
            got = calls["normal"](vecs)
            assert np.isfinite(got[2]).all()
            assert np.abs(got[0] - chi).max() <= 1e-12 * np.abs(chi).max()
            for rep in range(args.reps):
                order = list(calls) if rep % 2 == 0 else list(calls)[::-1]
                ms = {}
                for kind in order:
                    s.sync()
                    t0 = time.perf_counter()
                    calls[kind](vecs)
                    ms[kind] = 1e3 * (time.perf_counter() - t0)
                for kind in calls:
                    print(json.dumps({
                        "call": kind, "side": n, "nsrc": nsrc, "vectors": W, "rep": rep,
                        "ms": round(ms[kind], 3),
                        "vectors_per_s": round(W / (ms[kind] * 1e-3), 1),
                        "fp64_lane_ops_per_pixel": ops[kind] // (n * n),
                        "fp64_fraction_of_peak": round(W * ops[kind] / (ms[kind] * 1e-3) / PEAK, 4),
                        "ratio_to_chi2": round(ms[kind] / ms["chi2"], 4),
                    }), flush=True)


if __name__ == "__main__":
    main()
