"""apf_map command line: the best fit of a frame and its Laplace approximation.

    python apf_map.py <dir>/N2.<date>.<frame>.LDIF.fits [--starts N] [--scatter X] [--seed S]
                      [--fixed-bkgd] [--fix NAME ...] [--max-steps K]

The reference has no optimiser; this stages the frame as step 2 does (``Sampler``: the noise
model of apf_step2.py:176-210), takes the step-1 guess (apf_step2.py:264-273) and runs
``mapfit.fit`` on the device's Gauss-Newton sums (``Sampler.normal_equations``), with
``--starts`` N > 1 ``mapfit.multi_start``.  It prints the chi^2 history, theta_hat +- sigma
per parameter, the companions' separation and position angle in the detector frame with
their Laplace sigma, the flat directions and the number of distinct minima, and writes into
``<dir>/<frame>_apf_results/``

  map_fit.json      theta_hat, chi^2, status, steps, the free mask, F, the covariance, sigma,
                    correlation, eigenvalues, the run's settings (``apf_step2.py -i map``)
  map_widths.json   ``tune.save_widths`` of ``mapfit.proposal_widths``, source "laplace"
                    (``apf_step2.py --widths``)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

from . import fitsio, mapfit, pipeline, tune
from .core import Sampler

PIXSCALE_MAS = 9.95        # apf_step2.py:242-245


def parse(argv, nsrc):
    ap = argparse.ArgumentParser(prog="apf_map" + ("" if nsrc == 2 else "_3body"))
    ap.add_argument("image", type=str)
    ap.add_argument("--starts", type=int, default=1,
                    help="fits from this many starts: the step-1 guess and N - 1 scattered "
                         "about it")
    ap.add_argument("--scatter", type=float, default=1.0,
                    help="the scatter of the starts, in default proposal widths")
    ap.add_argument("--seed", type=int, default=0, help="RandomState seed of the scatter")
    ap.add_argument("--fixed-bkgd", action="store_true",
                    help="background = p[9] instead of the reference's p[12] (2-source)")
    ap.add_argument("--fix", type=str, nargs="+", default=[], metavar="NAME",
                    help="parameters held at the guess (names as step 3 prints them)")
    ap.add_argument("--max-steps", type=int, default=50, help="accepted steps per start")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("-q", "--quiet", action="store_true")
    args = ap.parse_args(argv)
    if args.starts < 1 or args.max_steps < 1 or not args.scatter >= 0.0:
        ap.error("--starts and --max-steps must be >= 1, --scatter >= 0")
    return args


def main(argv=None, nsrc=2):
    args = parse(sys.argv[1:] if argv is None else argv, nsrc)
    say = (lambda *a: None) if args.quiet else print
    image, hdr = fitsio.getdata_header(args.image)
    directory, frame, outdir = pipeline.image_paths(args.image)
    say(outdir)
    os.makedirs(outdir, exist_ok=True)
    bkgd_mode = 1 if args.fixed_bkgd else 0
    free = mapfit.free_mask(nsrc, bkgd_mode, fix=args.fix)
    guess = pipeline.read_guess(directory + frame + "_initialguess")
    p0 = pipeline.initial_parameters(image, guess, nsrc)[:-1]
    names = tune.param_names(nsrc)
    t0 = time.perf_counter()
    with Sampler(image, hdr["ITIME"], hdr["COADDS"], hdr["MULTISAM"], hdr["SAMPMODE"], nsrc=nsrc,
                 bkgd_mode=bkgd_mode, device=args.device) as s:
        normal = s.normal_equations
        if args.starts > 1:
            res = mapfit.multi_start(normal, p0, nsrc, args.starts, args.scatter, args.seed,
                                     bkgd_mode, free, max_steps=args.max_steps)
        else:
            res = mapfit.fit(normal, p0, nsrc, bkgd_mode, free, max_steps=args.max_steps)
        if not np.isfinite(res.chi2[0]):
            raise RuntimeError("no start has a finite chi^2")
        theta = mapfit.canonical(res.theta[0], nsrc, bkgd_mode, free)
        lap = mapfit.laplace(normal, theta, nsrc, bkgd_mode, free, PIXSCALE_MAS)
    wall = time.perf_counter() - t0
    say(f"chi^2 history ({res.status[0]}, {int(res.steps[0])} accepted steps, "
        f"{int(res.evals[0])} evaluations):", " ".join(f"{c:.6g}" for c in res.history[0]))
    for k, name in enumerate(names):
        say(f"  {name:9s} {lap.theta_hat[k]: .9g} +- {lap.sigma[k]:.3g}"
            + ("" if free[k] else "  (fixed)"))
    say("  A - off  ", " ".join(f"{v:.9g}" for v in lap.amp_minus_off))
    for k, (sp, pa) in enumerate(zip(lap.separation, lap.position_angle)):
        say(f"companion {k + 1}: separation {sp['px']:.5f} +- {sp['sigma_px']:.5f} px "
            f"({sp['mas']:.3f} +- {sp['sigma_mas']:.3f} mas), position angle {pa['deg']:.4f} +- "
            f"{pa['sigma_deg']:.4f} deg (detector frame, +x towards +y)")
    fnames = [n for n, f in zip(names, free) if f]
    say(f"flat directions: {len(lap.flat_directions)}")
    for v in lap.flat_directions:
        say("  " + " ".join(f"{n} {c:+.3f}" for n, c in zip(fnames, v) if abs(c) > 1e-3))
    if args.starts > 1:
        say(f"{res.minima} distinct minima among {args.starts} starts; chi^2",
            " ".join(f"{c:.6g}" for c in res.chi2))
    settings = {"image": os.path.abspath(args.image), "starts": args.starts,
                "scatter": args.scatter, "seed": args.seed, "fixed_bkgd": args.fixed_bkgd,
                "fix": list(args.fix), "max_steps": args.max_steps, "seconds": wall}
    with open(outdir + "map_fit.json", "w") as f:
        json.dump(mapfit.map_doc(lap, res, int(image.shape[1]), settings), f, indent=1)
        f.write("\n")
    tune.save_widths(outdir + "map_widths.json", nsrc,
                     mapfit.proposal_widths(lap.F, lap.theta_hat, nsrc, free), "laplace")
    say(f"best fit in {wall:.3f} s")
    return outdir
