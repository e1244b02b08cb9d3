"""The worked example of README's "Best fit and Laplace approximation" on the WAIC section's
frame (64 x 64, 2 sources, synth seed 0), and the wall times of the fit.

    python tools/map_example.py [--walkers 64] [--dir DIR]

1. Wall time, in this process, of ``apf_map.py`` with 1 start and with 64 starts beside the
   5,000-iteration ``apf_step2a.py`` on the same frame (each from its ``main``: staging the
   frame, the work, the files), and of ``mapfit.fit`` alone on a live context.
2. The 60,000-iteration run of the WAIC example (step-1 start, default widths, burn-in
   50,000, stride 10): the posterior sigma per parameter from the covariance fold beside the
   Laplace sigma, its multivariate R-hat and acceptance rates.
3. 2,000 recorded rows at stride 10 with no burn-in, from the step-1 start with the default
   widths and from ``laplace_draws`` (inflate 1) with ``map_widths.json``'s widths: R-hat and
   acceptance rates side by side.
One run's figures.  No GPU, no number: it fails without one.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


REST = [k for k in range(16) if k not in (6, 7, 9)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=64)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args(argv)
    from olpefit_amd import mapcli, mapfit, step2, step3, synth, tune
    from olpefit_amd.core import Sampler
    from olpefit_amd.covariance import Covariance, error_ellipse
    from olpefit_amd.pipeline import initial_parameters
    W, nsrc, n = args.walkers, 2, 64
    d = args.dir or tempfile.mkdtemp()
    path = synth.write_case(d, n, nsrc)
    names = tune.param_names(nsrc)

    def wall(fn):
        t0 = time.perf_counter()
        out = fn()
        return out, time.perf_counter() - t0

    mapcli.main([path, "-q"])                                       # code objects, page cache
    out, t1 = wall(lambda: mapcli.main([path, "-q"]))
    _, t64 = wall(lambda: mapcli.main([path, "-q", "--starts", "64"]))
    with open(out + "map_fit.json") as f:
        doc64 = json.load(f)
    _, t1b = wall(lambda: mapcli.main([path, "-q"]))
    _, t2a = wall(lambda: step2.main([path, "--seed", "1", "-q"], nsrc=nsrc, variant="2a"))
    fit = mapfit.load_map(out + "map_fit.json", nsrc, 0, n)
    widths = tune.load_widths(out + "map_widths.json", nsrc)
    print(json.dumps({"apf_map_1_start_s": round(t1, 4), "apf_map_1_start_again_s": round(t1b, 4),
                      "apf_map_64_starts_s": round(t64, 4), "minima_of_64": doc64["minima"],
                      "apf_step2a_5000_iterations_s": round(t2a, 4),
                      "steps": fit["steps"], "evals": fit["evals"], "chi2": fit["chi2"]}))

    img, _ = synth.make_image(n, nsrc, 0)
    p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
    seeds = np.arange(1, 1 + W)

    def ensemble(s, start, w, iters, burn):
        s.seed(seeds)
        s.set_widths(w)
        st = np.tile(np.append(fit["theta_hat"], 0.0), (W, 1)) if start is None else start
        st = np.array(st, dtype=np.float64)
        st[:, -1] = s.chi_squared(st)
        s.set_state(st)
        _, t = wall(lambda: s.run(iters, burn_in=burn, record_stride=10, read_chain=False))
        with Covariance(s.ps, walkers=W, labels=step3.NAMES_2) as cv:
            cv.fold(s)
            res = cv.result(nsrc=nsrc, pixscale=9.95, param_cols=range(s.np_))
            # ... and without the exactly flat direction's members (amps, ampc, bkgd)
            res["mpsrf_rest"] = cv.result(param_cols=REST)["mpsrf"]
        _, tries, acc = s.get_state()
        return res, acc.sum(axis=0) / tries.sum(axis=0), t

    with Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc) as s:
        s.normal_equations(p0)                                      # warm
        res, tfit = wall(lambda: mapfit.fit(s.normal_equations, p0[:-1], nsrc))
        ms, tms = wall(lambda: mapfit.multi_start(s.normal_equations, p0[:-1], nsrc, 64, 1.0, 0))
        print(json.dumps({"mapfit_fit_s": round(tfit, 5), "evals": int(res.evals[0]),
                          "multi_start_64_s": round(tms, 5), "evals_64": int(ms.evals.sum()),
                          "iterations_64": int(ms.evals.max()), "minima": ms.minima}))
        guess = np.tile(p0, (W, 1))
        long, acc_long, t_long = ensemble(s, guess, None, 60000, 50000)
        short, acc_short, t_short = ensemble(s, guess, None, 20000, 0)
        draws = np.hstack([mapfit.laplace_draws(fit, seeds, 1.0), np.zeros((W, 1))])
        lap, acc_lap, t_lap = ensemble(s, draws, widths, 20000, 0)
        mapd, acc_mapd, t_mapd = ensemble(s, draws, None, 20000, 0)
    sig_post = np.sqrt(np.diag(long["cov"]))[:16]
    print(f"{'parameter':>10} {'theta_hat':>14} {'Laplace sigma':>14} {'posterior sigma':>16} "
          f"{'ratio':>7} | acceptance: {'default':>8} {'map widths':>10} | {'width / default':>15}")
    for k, name in enumerate(names):
        r = fit["sigma"][k] / sig_post[k] if sig_post[k] > 0 else float("nan")
        print(f"{name:>10} {fit['theta_hat'][k]:14.7g} {fit['sigma'][k]:14.5g} {sig_post[k]:16.5g} "
              f"{r:7.3f} | {acc_short[k]:20.3f} {acc_lap[k]:10.3f} | "
              f"{widths[k] / tune.default_widths(nsrc)[k]:15.3f}")
    for label, r, t in (("step-1 start, 60,000 iterations, burn-in 50,000, default widths", long, t_long),
                        ("step-1 start, 2,000 rows from iteration 0, default widths", short, t_short),
                        ("laplace_draws x 1, 2,000 rows from iteration 0, default widths", mapd, t_mapd),
                        ("laplace_draws x 1, 2,000 rows from iteration 0, map widths", lap, t_lap)):
        mp, mr = r["mpsrf"], r["mpsrf_rest"]
        worst = int(np.nanargmax(mp["rhat"]))
        print(f"{label}: R-hat^p {mp['mpsrf']:.4f} (largest univariate {np.nanmax(mp['rhat']):.4f}, "
              f"{names[worst]}; {mp['m']} walkers x {mp['n']} rows); without amps, ampc, bkgd "
              f"{mr['mpsrf']:.4f} (largest univariate {np.nanmax(mr['rhat']):.4f}, "
              f"{names[REST[int(np.nanargmax(mr['rhat']))]]}); {t:.3f} s")
        print("   univariate:", " ".join(f"{n} {v:.3f}" for n, v in zip(names, mp["rhat"])))
    e, le = long["ellipses"][0], error_ellipse(fit["cov"], (0, 1), (2, 3))
    print(f"offset ellipse, posterior: {e['semi_major']:.5g} x {e['semi_minor']:.5g} px angle "
          f"{e['angle']:.2f}; Laplace: {le['semi_major']:.5g} x {le['semi_minor']:.5g} px angle "
          f"{le['angle']:.2f}")


if __name__ == "__main__":
    main()
