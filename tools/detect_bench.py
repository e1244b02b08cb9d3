"""What the companion detection map costs.

    python tools/detect_bench.py [--samples 4096 65536] [--big 1024] [--repeats 5]

Folds host rows (relative scatter 1e-3 about the truth of synth.make_image's frame) with
detect.Detect and, for scale, with residuals.Residuals in the same process, alternating the
two after a warm-up fold of each; the times are wall clock around fold_rows + a state read,
uploads included.  Cases: the 64x64 2-source frame at oversample 1 for each --samples count,
and the 128x128 3-source frame for --big samples.  Prints one JSON line per case: the median
and the fastest time of each fold, the detection fold's FP64 rate from 2 G n^2 lane-FMAs per
sample and plane (N and Q: 4 G n^2 flop-pairs) as a fraction of the 2.4 GHz vector peak
(256 CUs x 4 SIMDs x 16 lanes), the ratio to the residual fold, and the time of one sample's
K @ z in NumPy on the host.  No GPU, no number: it fails without one.

    python tools/detect_bench.py --null [--repeats 5]

The false-alarm calibration: detect_null.DetectNull.run(R) beside
Detect.fold_rows of S samples at the same shape, alternating, for 64x64 2-source oversample 1
(R = 4096), 128x128 3-source oversample 1 (R = 1024) and 64x64 oversample 4 (R = 1024).  One
JSON line per case: the time per realisation and per sample, their ratio (a realisation does
half a sample's FMAs and builds no table: the bound is 0.5), the realisations' FP64 rate from
G n^2 lane-FMAs each as a fraction of the vector peak (the whole run: noise, weighting,
correlation, reductions and the results' copy), and the time per realisation of the same maps
as one dense product in NumPy on the host.  The kernels' shares of a batch come from a kernel
trace of this run (rocprofv3 --kernel-trace --stats).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FMA = 256 * 4 * 16 * 2.4e9          # FP64 vector FMAs per second


def rows_about(base, S, seed):
    rng = np.random.RandomState(seed)
    P = base.size
    rows = np.empty((S, P + 1))
    rows[:, :P] = base * (1.0 + 1e-3 * rng.normal(size=(S, P)))
    rows[:, P] = rng.uniform(1e3, 2e3, size=S)
    return rows


def timed(obj, rows):
    obj.reset()
    t = time.perf_counter()
    obj.fold_rows(rows)
    obj.state()
    return time.perf_counter() - t


def host_one(n):
    """One sample's two correlations as a dense product on the host."""
    rng = np.random.RandomState(0)
    K, z = rng.uniform(size=(n * n, n * n)), rng.normal(size=n * n)
    t = time.perf_counter()
    (K @ z, (K * K) @ z)
    return time.perf_counter() - t


def host_null(n, R=32):
    """R realisations' correlations as one dense product on the host, per realisation."""
    rng = np.random.RandomState(0)
    K, y = rng.uniform(size=(n * n, n * n)), rng.normal(size=(n * n, R))
    t = time.perf_counter()
    K @ y
    return (time.perf_counter() - t) / R


def null_bench(repeats):
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.detect import Detect
    from olpefit_amd.detect_null import DetectNull

    def timed_null(h, R):
        h.reset()
        t = time.perf_counter()
        h.run(R)
        h.results()
        return time.perf_counter() - t
    for n, nsrc, os_, R, S in ((64, 2, 1, 4096, 4096), (128, 3, 1, 1024, 512),
                               (64, 2, 4, 1024, 512)):
        img, truth = synth.make_image(n, nsrc, 0)
        rows = rows_about(truth, S, 1)
        with Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc) as s, \
                Detect(s, pivot=truth, oversample=os_) as d, DetectNull(d, truth) as h:
            timed(d, rows[:256]), timed_null(h, 64)
            td, tn = [], []
            for _ in range(repeats):
                td.append(timed(d, rows))
                tn.append(timed_null(h, R))
        G = float(os_ * (n - 1) + 1) ** 2
        per_r, per_s = float(np.median(tn)) / R, float(np.median(td)) / S
        print(json.dumps({
            "null": True, "side": n, "nsrc": nsrc, "oversample": os_, "realisations": R,
            "samples": S, "repeats": repeats, "null_s_median": float(np.median(tn)),
            "null_s_min": float(min(tn)), "detect_s_median": float(np.median(td)),
            "s_per_realisation": per_r, "s_per_sample": per_s,
            "ratio_realisation_to_sample": per_r / per_s,
            "fp64_peak_fraction": G * n * n / per_r / PEAK_FMA,
            "host_numpy_s_per_realisation": host_null(n) if n <= 64 and os_ == 1 else None}),
            flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--null", action="store_true",
                    help="the false-alarm calibration beside the detection fold")
    ap.add_argument("--samples", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--big", type=int, default=1024, help="samples of the 128x128 case (0: skip)")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args(argv)
    if args.null:
        return null_bench(args.repeats)
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.detect import Detect
    from olpefit_amd.residuals import Residuals
    cases = [(64, 2, S) for S in args.samples] + ([(128, 3, args.big)] if args.big else [])
    for n, nsrc, S in cases:
        img, truth = synth.make_image(n, nsrc, 0)
        rows = rows_about(truth, S, 1)
        with Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc) as s, Detect(s, pivot=truth) as d, \
                Residuals(s, pivot=truth) as r:
            warm = rows[:min(S, 1024)]
            timed(d, warm), timed(r, warm)
            td, tr = [], []
            for _ in range(args.repeats):          # alternating: drift hits both alike
                td.append(timed(d, rows))
                tr.append(timed(r, rows))
        G = float((n - 1) + 1) ** 2
        fma = 2.0 * G * n * n * S
        print(json.dumps({
            "side": n, "nsrc": nsrc, "samples": S, "oversample": 1, "repeats": args.repeats,
            "detect_s_median": float(np.median(td)), "detect_s_min": float(min(td)),
            "resid_s_median": float(np.median(tr)), "resid_s_min": float(min(tr)),
            "detect_fma_per_s": fma / float(np.median(td)),
            "fp64_peak_fraction": fma / float(np.median(td)) / PEAK_FMA,
            "ratio_to_resid": float(np.median(td)) / float(np.median(tr)),
            "host_numpy_one_sample_s": host_one(n) if n <= 64 else None}), flush=True)


if __name__ == "__main__":
    main()
