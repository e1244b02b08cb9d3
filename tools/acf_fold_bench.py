"""Time olpe_acf's fold of a sampler launch's device chain.

    python tools/acf_fold_bench.py [--walkers W] [--rows R] [--stride S] [--max-lag L]
        [--reps N] [--tiles 0,256]
    python tools/acf_fold_bench.py --numpy [--walkers W] [--rows R] [--max-lag L]

A bench.py-style configs[2] ensemble (synthetic 64x64 cutout, 2 sources, step-1 start) runs
rows x stride iterations in the default (FAST) mode, recording every stride-th row; then,
per repetition (and per OLPE_ACF_TILE setting, 0 = the default), a fresh Autocorr folds that
launch behind a device synchronise and the fold is timed by the host clock up to the next
synchronise.  Prints one JSON line per fold: ms, the FP64 FMAs it counts, series x ncols x
sum_{k=0..L} (N - k), over the 39.3e12 lane-ops/s peak, and the fold's cost as a share of the
launch's kernel time; then one line with the per-column tau of the run and the smallest
effective sample size per second of sampling.  No GPU, no number: it fails without one.

--numpy times the float64 NumPy forms of the same sums on the host instead (the direct
products and an np.fft form), without a GPU: the chains are synthetic AR(1) rows.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 39.3e12                                       # FP64 lane-ops/s


def fmas(series, ncols, N, L):
    return series * ncols * sum(max(N - k, 0) for k in range(L + 1))


def numpy_forms(W, N, ncols, L):
    """The lag sums of [W][N][ncols] AR(1) rows in float64: direct products, then np.fft."""
    rng = np.random.RandomState(0)
    phi = np.linspace(0.0, 0.97, ncols)
    z = np.empty((N, W, ncols))
    z[0] = rng.normal(size=(W, ncols))
    for t in range(1, N):
        z[t] = phi * z[t - 1] + rng.normal(size=(W, ncols))
    x = 512.3 + 1e-2 * np.ascontiguousarray(np.swapaxes(z, 0, 1))
    t0 = time.perf_counter()
    d = x - x[:, :1, :]
    y = d - d.mean(axis=1, keepdims=True)
    C1 = np.stack([(y[:, :N - k, :] * y[:, k:, :]).sum(axis=(0, 1)) for k in range(L + 1)], axis=1)
    t1 = time.perf_counter()
    d = x - x[:, :1, :]
    y = d - d.mean(axis=1, keepdims=True)
    nfft = 1 << int(np.ceil(np.log2(2 * N)))
    F = np.fft.rfft(y, n=nfft, axis=1)
    C2 = np.fft.irfft(F * np.conj(F), n=nfft, axis=1)[:, :L + 1, :].sum(axis=0).T
    t2 = time.perf_counter()
    dev = float(np.abs(C1 - C2).max() / np.abs(C1[:, 0]).max())
    for form, s in (("direct", t1 - t0), ("fft", t2 - t1)):
        print(json.dumps({"numpy_form": form, "walkers": W, "rows": N, "ncols": ncols,
                          "max_lag": L, "seconds": round(s, 3),
                          "fmas_per_s": round(fmas(W, ncols, N, L) / s, 1),
                          "forms_agree_to": dev}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=2000, help="rows recorded per walker")
    ap.add_argument("--stride", type=int, default=10, help="iterations per recorded row")
    ap.add_argument("--max-lag", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiles", default="0", help="OLPE_ACF_TILE settings, 0 = the default")
    ap.add_argument("--numpy", action="store_true")
    args = ap.parse_args(argv)
    if args.numpy:
        numpy_forms(args.walkers, args.rows, 17, args.max_lag)
        return
    from olpefit_amd import synth
    from olpefit_amd.autocorr import Autocorr
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    from olpefit_amd.step3 import NAMES_2
    W, n, nsrc, L = args.walkers, 64, 2, args.max_lag
    img, _ = synth.make_image(n, nsrc, 0)
    with Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc) as s:
        p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
        p0[-1] = s.chi_squared(p0)
        s.seed(np.arange(1000, 1000 + W))
        s.set_state(np.tile(p0, (W, 1)))
        s.run(10 * args.stride, 0, args.stride, read_chain=False)                # warm-up
        with Autocorr(s.ps, L) as a:                                              # code objects
            a.fold(s)
            a.state()
        t0 = time.perf_counter()
        nrec = s.run_async(args.rows * args.stride, 0, args.stride)
        s.sync()
        wall = time.perf_counter() - t0
        launch_ms = s.last_kernel_ms()
        ops = fmas(W, s.ps, nrec, L)
        states = []
        for rep in range(args.reps):
            for tile in args.tiles.split(","):
                if int(tile):
                    os.environ["OLPE_ACF_TILE"] = tile
                else:
                    os.environ.pop("OLPE_ACF_TILE", None)
                with Autocorr(s.ps, L, labels=NAMES_2) as a:
                    t0 = time.perf_counter()
                    a.fold(s)
                    s.sync()
                    ms = 1e3 * (time.perf_counter() - t0)
                    st = a.state()
                    res = a.result()
                states.append(st["C"])
                print(json.dumps({
                    "walkers": W, "rows": nrec, "stride": args.stride, "ncols": s.ps,
                    "max_lag": L, "tile": int(tile), "rep": rep, "series": st["series"],
                    "skipped": st["skipped"], "fold_ms": round(ms, 3), "fp64_fmas": ops,
                    "fp64_fraction_of_peak": round(ops / (ms * 1e-3) / PEAK, 4),
                    "launch_ms": round(launch_ms, 3),
                    "fold_share_of_launch": round(ms / launch_ms, 5)}), flush=True)
        same = all(np.array_equal(states[0], c) for c in states[1:])
        print(json.dumps({
            "repeated_folds_give_identical_bits": bool(same) if args.tiles == "0" else None,
            "sampling_wall_s": round(wall, 3), "sampling_kernel_ms": round(launch_ms, 3),
            "walker_steps_per_s": round(W * nrec * args.stride / (launch_ms * 1e-3), 1),
            "tau_rows": {k: round(float(v), 3) for k, v in zip(NAMES_2, res["tau"])},
            "windowed": [bool(v) for v in res["windowed"]],
            "reliable": [bool(v) for v in res["reliable"]],
            "min_ess": round(res["min_ess"], 1),
            "min_ess_per_s_of_sampling": round(res["min_ess"] / (launch_ms * 1e-3), 1)}),
            flush=True)


if __name__ == "__main__":
    main()
