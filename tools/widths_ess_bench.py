"""What the proposal widths are worth in effective samples per second.

    python tools/widths_ess_bench.py [--walkers W] [--rows R] [--stride S] [--burn B]
        [--tune-every N] [--target A] [--gain G] [--max-lag L]

The configs[2]-like ensemble of §7e / §7g (synthetic 64x64 cutout, 2 sources, step-1 start,
FAST mode, seeds 1000 + w) runs three times with the same seeds and the same number of
iterations, B unrecorded ones and then R rows at stride S in one launch:

  default      the reference's widths throughout;
  tuned        the tuner (Sampler.tune_*) adapts the widths over the B burn-in iterations,
               a step behind every launch of N, and they are frozen for the recorded launch;
  covariance   covariance.proposal_widths of the default run's recorded launch, from the
               first iteration on.

Each recorded launch is folded on the device by Autocorr and Covariance.  Prints one JSON
line per run: the widths as factors of the defaults, the acceptance rate per parameter over
the recorded launch, tau per column in recorded rows, the smallest ESS, the recorded
launch's kernel time and the smallest ESS per second of it, the smallest conditional
efficiency; then one line comparing the three.  No GPU, no number: it fails without one.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=65536)
    ap.add_argument("--rows", type=int, default=2000, help="rows recorded per walker")
    ap.add_argument("--stride", type=int, default=10, help="iterations per recorded row")
    ap.add_argument("--burn", type=int, default=4800, help="unrecorded iterations first")
    ap.add_argument("--tune-every", type=int, default=240)
    ap.add_argument("--target", type=float, default=0.44)
    ap.add_argument("--gain", type=float, default=2.0)
    ap.add_argument("--max-lag", type=int, default=1024)
    args = ap.parse_args(argv)
    if args.burn % args.tune_every:
        ap.error("--tune-every must divide --burn")
    from olpefit_amd import covariance as cv, synth, tune
    from olpefit_amd.autocorr import Autocorr
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    from olpefit_amd.step3 import NAMES_2
    W, n, nsrc = args.walkers, 64, 2
    img, _ = synth.make_image(n, nsrc, 0)
    d = tune.default_widths(nsrc)
    names = NAMES_2[:-1]

    def one(kind, widths=None):
        with Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc) as s:
            p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
            p0[-1] = s.chi_squared(p0)
            s.seed(np.arange(1000, 1000 + W))
            s.set_state(np.tile(p0, (W, 1)))
            if widths is not None:
                s.set_widths(widths)
            steps = 0
            if kind == "tuned":
                s.tune_begin(args.target, args.gain)
                for _ in range(args.burn // args.tune_every):
                    s.run_async(args.tune_every)
                    s.tune_step()
                steps = len(s.tune_history()[0])
                s.tune_end()
            elif args.burn:
                s.run_async(args.burn)
            w = s.get_widths()
            _, t0, a0 = s.get_state()
            total = args.burn + args.rows * args.stride
            nrec = s.run_async(args.rows * args.stride, args.burn, args.stride)
            with Autocorr(s.ps, args.max_lag, labels=NAMES_2) as ac, \
                    cv.Covariance(s.ps, W, labels=NAMES_2) as c:
                ac.fold(s)
                c.fold(s)
                s.sync()
                ms = s.last_kernel_ms()
                res = ac.result()
                cst = c.state()
                cres = c.result(param_cols=range(s.ps - 1), state=cst)
            _, t1, a1 = s.get_state()
            assert s.count == total
        rate = (a1 - a0).sum(0) / np.maximum((t1 - t0).sum(0), 1.0)
        fin = np.isfinite(res["ess"][:-1])
        worst = int(np.nanargmin(np.where(fin, res["ess"][:-1], np.nan)))
        eff = cres["conditional"]["efficiency"]
        out = {"run": kind, "walkers": W, "rows": nrec, "stride": args.stride, "burn": args.burn,
               "iterations": total, "tuner_steps": steps,
               "width_over_default": {k: round(float(v), 4) for k, v in zip(names, w / d)},
               "acceptance": {k: round(float(v), 4) for k, v in zip(names, rate)},
               "tau_rows": {k: (round(float(v), 2) if np.isfinite(v) else None)
                            for k, v in zip(NAMES_2, res["tau"])},
               "unwindowed": [k for k, ok in zip(NAMES_2, res["windowed"]) if not ok],
               "min_ess": res["min_ess"], "min_ess_parameters": float(res["ess"][worst]),
               "min_ess_column": names[worst], "values_per_column": res["n"],
               "recorded_launch_ms": round(ms, 3),
               "min_ess_per_second": res["min_ess"] / (ms * 1e-3),
               "walker_steps_per_second": W * args.rows * args.stride / (ms * 1e-3),
               "min_efficiency": float(np.nanmin(eff)),
               "mpsrf": cres["mpsrf"]["mpsrf"]}
        print(json.dumps(out), flush=True)
        return out, cst

    base, cst = one("default")
    tuned, _ = one("tuned")
    covw, _ = one("covariance", cv.proposal_widths(cst, nsrc))
    print(json.dumps({"min_ess_per_second_over_default": {
        "tuned": tuned["min_ess_per_second"] / base["min_ess_per_second"],
        "covariance": covw["min_ess_per_second"] / base["min_ess_per_second"]},
        "min_ess_over_default": {"tuned": tuned["min_ess"] / base["min_ess"],
                                 "covariance": covw["min_ess"] / base["min_ess"]}}), flush=True)


if __name__ == "__main__":
    main()
