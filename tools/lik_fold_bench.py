"""Time olpe_lik's fold of a sampler launch's device chain beside olpe_resid's fold of the
same launch.

    python tools/lik_fold_bench.py [--config 2|4] [--walkers W] [--rows R] [--stride S]
        [--thin T] [--reps N] [--heights 4,8]

A bench.py-style ensemble (synthetic cutout, step-1 start) runs rows x stride iterations
in the default (FAST) mode, recording every stride-th row; then, per repetition, a fresh
Residuals (the yardstick) and a fresh Predictive per tile height fold that launch one after
the other (the order alternates from repetition to repetition), each behind a device
synchronise and timed by the host clock up to the next synchronise.  Prints one JSON line
per fold: ms, samples/s, the FP64 lane-operations it counts over the 39.3e12 lane-ops/s
peak, its time over the residual fold's of the same repetition, and its cost as a share of
the launch's kernel time.  The count per pixel and sample: DESIGN.md §4's EXACT model,
21 G + G + 3, plus for olpe_resid the 3 of its sums and for olpe_lik 26: t (2), x (1),
x - c, A1, A2 (3), x - m, its half, the compare and L's update (4), and the 16 of the one
more exp_neg.  No GPU, no number: it fails without one.
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
RESID_EXTRA, LIK_EXTRA = 3, 26


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, choices=sorted(SHAPES))
    ap.add_argument("--walkers", type=int, default=0)
    ap.add_argument("--rows", type=int, default=10, help="rows recorded per walker")
    ap.add_argument("--stride", type=int, default=10, help="iterations per recorded row")
    ap.add_argument("--thin", type=int, default=1, help="row_step of the fold")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--heights", default="4,8")
    args = ap.parse_args(argv)
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    from olpefit_amd.predictive import Predictive
    from olpefit_amd.residuals import Residuals
    W, n, nsrc = SHAPES[args.config]
    W = args.walkers or W
    G = 2 * nsrc
    model_ops = n * n * (21 * G + G + 3)
    img, _ = synth.make_image(n, nsrc, 0)

    def timed(obj, s):
        t0 = time.perf_counter()
        obj.fold(s, row_step=args.thin)
        s.sync()
        return 1e3 * (time.perf_counter() - t0)

    with Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc) as s:
        p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
        p0[-1] = s.chi_squared(p0)
        s.seed(np.arange(1000, 1000 + W))
        s.set_state(np.tile(p0, (W, 1)))
        s.run(args.rows * args.stride, 0, args.stride, read_chain=False)      # warm-up
        with Residuals(s) as r, Predictive(s) as p:                            # code objects
            r.fold(s, row_step=args.rows)
            p.fold(s, row_step=args.rows)
            r.state(), p.state()
        states = {}
        for rep in range(args.reps):
            nrec = s.run_async(args.rows * args.stride, 0, args.stride)
            s.sync()
            launch_ms = s.last_kernel_ms()
            jobs = [("resid", "")] + [("lik", h) for h in args.heights.split(",")]
            if rep % 2:
                jobs.reverse()
            got = {}
            for kind, h in jobs:                               # the same launch, each object
                if kind == "resid":
                    with Residuals(s) as r:
                        ms = timed(r, s)
                        st = r.state()
                else:
                    os.environ["OLPE_LIK_ROWS"] = h
                    with Predictive(s) as p:
                        ms = timed(p, s)
                        st = p.state()
                        states.setdefault(rep, []).append(st)
                got[(kind, h)] = (ms, st["n"], st["n_bad"])
            base = got[("resid", "")][0]
            for (kind, h), (ms, S, bad) in got.items():
                ops = S * (model_ops + n * n * (RESID_EXTRA if kind == "resid" else LIK_EXTRA))
                print(json.dumps({
                    "fold": kind, "config": args.config, "side": n, "nsrc": nsrc, "walkers": W,
                    "rows": nrec, "stride": args.stride, "thin": args.thin,
                    "tile_rows": int(h) if h else None, "rep": rep, "samples": S, "n_bad": bad,
                    "fold_ms": round(ms, 3), "samples_per_s": round(S / (ms * 1e-3), 1),
                    "fp64_lane_ops": ops,
                    "fp64_fraction_of_peak": round(ops / (ms * 1e-3) / PEAK, 4),
                    "ratio_to_resid_fold": round(ms / base, 4),
                    "launch_ms": round(launch_ms, 3),
                    "fold_share_of_launch": round(ms / launch_ms, 4),
                    "thin_for_5_percent": int(np.ceil(ms / launch_ms * args.thin / 0.05)),
                }), flush=True)
        keys = ("a1", "a2", "m", "l")
        same = all(np.array_equal(q[0][k], x[k], equal_nan=True)
                   for q in states.values() for x in q[1:] for k in keys)
        print(json.dumps({"tile_heights_give_identical_states": bool(same)}), flush=True)


if __name__ == "__main__":
    main()
