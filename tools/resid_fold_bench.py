"""Time olpe_resid's fold of a sampler launch's device chain.

    python tools/resid_fold_bench.py [--config 2|4] [--walkers W] [--rows R] [--stride S]
        [--thin T] [--reps N] [--heights 8,16]

A bench.py-style ensemble (synthetic cutout, step-1 start) runs rows x stride iterations
in the default (FAST) mode, recording every stride-th row; then, per tile height and
repetition (the heights alternate), a fresh Residuals folds that launch behind a device
synchronise and the fold is timed by the host clock up to the next synchronise (folds take
0.1-20 s).  Prints one JSON line per fold: ms, samples/s, the FP64 lane-operations it
counts (DESIGN.md §4's EXACT model, n^2 (21 G + G + 3), plus 3 per pixel for the sums) over
the 39.3e12 lane-ops/s peak, and the fold's cost as a share of the launch's kernel time.
No GPU, no number: it fails without one.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {2: (65536, 64, 2), 4: (16384, 128, 3)}     # bench.py's CONFIGS
PEAK = 39.3e12                                       # FP64 lane-ops/s


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, choices=sorted(SHAPES))
    ap.add_argument("--walkers", type=int, default=0)
    ap.add_argument("--rows", type=int, default=10, help="rows recorded per walker")
    ap.add_argument("--stride", type=int, default=10, help="iterations per recorded row")
    ap.add_argument("--thin", type=int, default=1, help="row_step of the fold")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--heights", default="8,16")
    args = ap.parse_args(argv)
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    from olpefit_amd.residuals import Residuals
    W, n, nsrc = SHAPES[args.config]
    W = args.walkers or W
    G = 2 * nsrc
    ops_per_sample = n * n * (21 * G + G + 3 + 3)
    img, _ = synth.make_image(n, nsrc, 0)
    with Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc) as s:
        p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
        p0[-1] = s.chi_squared(p0)
        s.seed(np.arange(1000, 1000 + W))
        s.set_state(np.tile(p0, (W, 1)))
        s.run(args.rows * args.stride, 0, args.stride, read_chain=False)      # warm-up
        with Residuals(s) as r:                                                # code objects
            r.fold(s, row_step=args.rows)
            r.state()
        planes = {}
        for rep in range(args.reps):
            nrec = s.run_async(args.rows * args.stride, 0, args.stride)
            s.sync()
            launch_ms = s.last_kernel_ms()
            for h in args.heights.split(","):                  # the same launch, each height
                os.environ["OLPE_RESID_ROWS"] = h
                with Residuals(s) as r:
                    t0 = time.perf_counter()
                    r.fold(s, row_step=args.thin)
                    s.sync()
                    ms = 1e3 * (time.perf_counter() - t0)
                    st = r.state()
                    planes.setdefault(rep, []).append(r.finalize()[0])
                S = st["n"]
                print(json.dumps({
                    "config": args.config, "side": n, "nsrc": nsrc, "walkers": W, "rows": nrec,
                    "stride": args.stride, "thin": args.thin, "tile_rows": int(h), "rep": rep,
                    "samples": S, "n_bad": st["n_bad"], "fold_ms": round(ms, 3),
                    "samples_per_s": round(S / (ms * 1e-3), 1),
                    "fp64_lane_ops": S * ops_per_sample,
                    "fp64_fraction_of_peak": round(S * ops_per_sample / (ms * 1e-3) / PEAK, 4),
                    "launch_ms": round(launch_ms, 3),
                    "fold_share_of_launch": round(ms / launch_ms, 4),
                    "thin_for_5_percent": int(np.ceil(ms / launch_ms * args.thin / 0.05)),
                }), flush=True)
        same = all(np.array_equal(p[0], q, equal_nan=True) for p in planes.values() for q in p[1:])
        print(json.dumps({"tile_heights_give_identical_planes": bool(same)}), flush=True)


if __name__ == "__main__":
    main()
