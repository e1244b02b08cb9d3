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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--big", type=int, default=1024, help="samples of the 128x128 case (0: skip)")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args(argv)
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
