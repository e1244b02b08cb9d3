"""Time olpe_cov's fold of a sampler launch's device chain, with the
photometry fold of the same launch beside it as the yardstick (§7f).

    python tools/cov_fold_bench.py [--walkers W] [--rows R] [--stride S] [--reps N]
        [--tiles 0,64,128] [--pooled]
    python tools/cov_fold_bench.py --numpy [--walkers W] [--rows R]

A bench.py-style configs[2] ensemble (synthetic 64x64 cutout, 2 sources, step-1 start) runs
rows x stride iterations in the default (FAST) mode, recording every stride-th row; then,
per repetition (and per OLPE_COV_TILE setting, 0 = the default), a fresh Covariance (with the
walkers' sums unless --pooled) folds that launch behind a device synchronise, and the fold
is timed by the host clock up to the next synchronise; a fresh Photometry folds the same
launch the same way.  Prints one JSON line per fold: ms, the bytes of chain read over the
time (TB/s), that rate over the 6.29 TB/s a float4 copy reaches, and the time over the
photometry fold's; then one line saying whether the repeated folds gave identical bits, with
the multivariate R-hat and the smallest conditional efficiency of the run.  No GPU, no
number: it fails without one.

--numpy times the float64 NumPy form of the same S2 (d^T d over all rows) on the host
instead, without a GPU, on synthetic rows.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY = 6.29e12                                       # bytes/s of a float4 copy


def numpy_form(W, N, ncols):
    rng = np.random.RandomState(0)
    chunk = max(1, min(W, (1 << 27) // (N * ncols)))  # 1 GiB of rows at a time
    S1, S2, secs = np.zeros(ncols), np.zeros((ncols, ncols)), 0.0
    p = None
    for w0 in range(0, W, chunk):
        x = 512.3 + 1e-2 * rng.normal(size=(min(chunk, W - w0) * N, ncols))
        p = x[0].copy() if p is None else p
        t0 = time.perf_counter()
        d = x - p
        S1 += d.sum(axis=0)
        S2 += d.T @ d
        secs += time.perf_counter() - t0
    print(json.dumps({"numpy_form": "d.T @ d", "walkers": W, "rows": N, "ncols": ncols,
                      "seconds": round(secs, 3), "threads": os.cpu_count(),
                      "gb_per_s": round(W * N * ncols * 8 / secs / 1e9, 2)}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=2000, help="rows recorded per walker")
    ap.add_argument("--stride", type=int, default=10, help="iterations per recorded row")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiles", default="0", help="OLPE_COV_TILE settings, 0 = the default")
    ap.add_argument("--pooled", action="store_true", help="walkers = 0: no per-walker sums")
    ap.add_argument("--numpy", action="store_true")
    args = ap.parse_args(argv)
    if args.numpy:
        numpy_form(args.walkers, args.rows, 17)
        return
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.covariance import Covariance
    from olpefit_amd.photometry import Photometry
    from olpefit_amd.pipeline import initial_parameters
    from olpefit_amd.step3 import NAMES_2
    W, n, nsrc = args.walkers, 64, 2
    keep = 0 if args.pooled else W
    img, _ = synth.make_image(n, nsrc, 0)
    with Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc) as s:
        p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
        p0[-1] = s.chi_squared(p0)
        s.seed(np.arange(1000, 1000 + W))
        s.set_state(np.tile(p0, (W, 1)))
        s.run(10 * args.stride, 0, args.stride, read_chain=False)                # warm-up
        with Covariance(s.ps, keep) as c, Photometry(W, 10, variant=nsrc, pixscale=9.952,
                                                     ps=s.ps) as p:              # code objects
            c.fold(s)
            p.fold(s)
            c.state()
            p.finalize()
        nrec = s.run_async(args.rows * args.stride, 0, args.stride)
        s.sync()
        launch_ms = s.last_kernel_ms()
        nbytes = W * nrec * s.ps * 8
        states, phot_ms, res = [], [], None
        for rep in range(args.reps):
            with Photometry(W, nrec, variant=nsrc, pixscale=9.952, ps=s.ps) as p:
                t0 = time.perf_counter()
                p.fold(s)
                s.sync()
                phot_ms.append(1e3 * (time.perf_counter() - t0))
            print(json.dumps({"fold": "photometry", "walkers": W, "rows": nrec, "rep": rep,
                              "fold_ms": round(phot_ms[-1], 3)}), flush=True)
            for tile in args.tiles.split(","):
                if int(tile):
                    os.environ["OLPE_COV_TILE"] = tile
                else:
                    os.environ.pop("OLPE_COV_TILE", None)
                with Covariance(s.ps, keep, labels=NAMES_2) as c:
                    t0 = time.perf_counter()
                    c.fold(s)
                    s.sync()
                    ms = 1e3 * (time.perf_counter() - t0)
                    st = c.state()
                    if res is None:
                        res = c.result(param_cols=range(s.ps - 1))
                if not int(tile):
                    states.append(st)
                rate = nbytes / (ms * 1e-3)
                print(json.dumps({
                    "fold": "covariance", "walkers": W, "rows": nrec, "stride": args.stride,
                    "ncols": s.ps, "per_walker_sums": bool(keep), "tile": int(tile), "rep": rep,
                    "n": st["n"], "skipped": st["skipped"], "fold_ms": round(ms, 3),
                    "chain_bytes": nbytes, "tb_per_s": round(rate / 1e12, 3),
                    "fraction_of_copy_rate": round(rate / COPY, 3),
                    "over_photometry_fold": round(ms / phot_ms[-1], 3),
                    "launch_ms": round(launch_ms, 3)}), flush=True)
        same = all(np.array_equal(states[0][k], t[k]) for t in states[1:]
                   for k in ("S1", "S2") + (("S1w", "nw") if keep else ()))
        eff = res["conditional"]["efficiency"]
        print(json.dumps({
            "repeated_folds_give_identical_bits": bool(same) if len(states) > 1 else None,
            "mpsrf": res["mpsrf"]["mpsrf"], "mpsrf_note": res["mpsrf"]["note"],
            "condition": res["conditional"]["condition"],
            "efficiency": {k: (round(float(v), 4) if np.isfinite(v) else None)
                           for k, v in zip(NAMES_2, eff)},
            "largest_correlations": res["pairs"][:5]}), flush=True)


if __name__ == "__main__":
    main()
