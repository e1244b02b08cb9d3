"""Step-3 read contract and convergence summary.

apf_step3.py reads the step-2 chain files (:169-186), drops ``additional_burnin`` rows
(:81-84, :190-205; default 1 = the NaN seed row) and computes Gelman-Rubin statistics
with d = 16 (:258-278) before its distortion / refraction / plotting stages.  This
module is that read + statistics front end, usable on the build's output; with
``--astrometry`` it goes on to the separation / position-angle summary (:211-256,
:283-343, :401-450), reduced on the GPU (olpefit_amd/astrometry.py).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

NAMES_2 = ["xcs", "ycs", "xcc", "ycc", "dx", "dy", "amps", "ampc", "ampratio", "bkgd",
           "sigmax", "sigmay", "sigmax2", "sigmay2", "theta", "theta2", "chisquare"]
NAMES_3 = ["xca", "yca", "xcb", "ycb", "xcc", "ycc", "dx", "dy", "ampa", "ampb", "ampc",
           "ampratio", "bkgd", "sigmax", "sigmay", "sigmax2", "sigmay2", "theta", "theta2",
           "chisquare"]


def load_chains(input_directory: str, ncor: int, additional_burnin: int = 1,
                source: str = "csv", threads: int = 0):
    """apf_step3.py:169-205: returns an array [length - additional_burnin, ncor, PS].

    The chain length is taken from walker 0 and every walker file must have it (the
    reference assigns columns into [length, ncor] arrays, :174-186).  ``source="csv"``
    parses the ``{i}_finalarray_mpi.csv`` files natively from a pool of threads
    (olpe_csv_read_chains: the values np.genfromtxt returns, bit for bit);
    ``source="npy"`` reads the ``{i}_chain.npy`` sidecars step 2 writes with ``--npy``
    (the same rows without the NaN seed row, which counts as one burn-in row)."""
    from . import _lib
    if source == "npy":
        paths = [os.path.join(input_directory, f"{i}_chain.npy") for i in range(ncor)]
        first = np.load(paths[0], mmap_mode="r")
        length, ps = first.shape[0] + 1, first.shape[1]
        burn = min(max(0, int(additional_burnin)), length)
        out = np.empty((length - burn, ncor, ps))
        if burn == 0:
            out[0] = np.nan                     # the seed row the CSV files start with
        lo, o = max(0, burn - 1), 1 if burn == 0 else 0
        for i, p in enumerate(paths):
            a = np.load(p, mmap_mode="r")
            if a.shape != first.shape:
                raise ValueError(f"walker {i}: chain shape {a.shape} != walker 0's {first.shape}")
            out[o:, i, :] = a[lo:]
        return out
    if source != "csv":
        raise ValueError("source must be 'csv' or 'npy'")
    lib = _lib.load()
    paths = [os.fsencode(os.path.join(input_directory, f"{i}_finalarray_mpi.csv"))
             for i in range(ncor)]
    rows, cols = C.c_longlong(0), C.c_int(0)
    _lib.check(lib.olpe_csv_shape(paths[0], C.byref(rows), C.byref(cols)))
    length, ps = rows.value, cols.value
    skip = min(max(0, int(additional_burnin)), length)
    out = np.empty((length - skip, ncor, ps))
    arr = (C.c_char_p * ncor)(*paths)
    rc = lib.olpe_csv_read_chains(arr, ncor, length, ps, skip,
                                  out.ctypes.data_as(C.POINTER(C.c_double)), int(threads))
    if rc == _lib.EINVAL:
        raise ValueError(lib.olpe_last_error().decode(errors="replace"))
    _lib.check(rc)
    return out


def gelman_rubin(p, d: int = 16):
    """apf_step3.py:260-276 (3body/apf_step3_3body.py:294-310) for one parameter:
    p [N, M] (rows, walkers) -> (PSRF, RC).

    The reference is Python 2 without ``from __future__ import division``, so its
    ``RC = np.sqrt(((d+3)/(d+1))*PSRF)`` with the int ``d = 16`` (:264, :276) divides
    19 by 17 as integers: the factor is 1 and RC = sqrt(PSRF).  Integer ``d`` keeps
    that floor division here; a float ``d`` divides as floats, as it would there."""
    p = np.asarray(p, dtype=np.float64)
    # (NumPy floats: one walker gives NaN, as summary_from_moments does, not a raise)
    N, M = np.float64(p.shape[0]), np.float64(p.shape[1])
    overall_mean = np.mean(p)
    # the reference's per-column loop (np.mean / np.std of p[:, i]) as row reductions of
    # the transpose: the same pairwise sums over the same values, so the same bits
    # (a Python loop over 65,536 walkers took 45 s of step 3)
    pt = np.ascontiguousarray(p.T)
    chain_mean = np.mean(pt, axis=1)
    w = np.std(pt, axis=1) ** 2
    b = (chain_mean - overall_mean) ** 2
    w = (1. / M) * np.sum(w)
    b = (N / (M - 1)) * np.sum(b)
    pooled = ((N - 1) / N) * w + ((M + 1) / (M * N)) * b
    psrf = pooled / w
    factor = (d + 3) // (d + 1) if isinstance(d, (int, np.integer)) else (d + 3) / (d + 1)
    return psrf, np.sqrt(factor * psrf)


def summary(chains, nsrc: int = 2):
    """Per-parameter mean, median, std and Gelman-Rubin PSRF / RC over [N, M, PS]
    chains (the chi^2 column is not a GR parameter: apf_step3.py:260,
    3body/apf_step3_3body.py:294)."""
    names = NAMES_2 if nsrc == 2 else NAMES_3
    out = {}
    for k, name in enumerate(names[:-1]):
        x = chains[:, :, k]
        psrf, rc = gelman_rubin(x)
        out[name] = {"mean": float(np.mean(x)), "median": float(np.median(x)),
                     "std": float(np.std(x)), "gr_psrf": float(psrf), "gr_rc": float(rc)}
    return out


def summary_from_moments(m, nsrc: int = 2, d: int = 16):
    """The statistics of ``summary`` (minus the median, which no moment gives) from the
    device-accumulated whole-run moments -- ``Sampler.allreduce_moments()``, the
    olpe_moments_summary layout with the centre at the pooled mean -- without reading a
    chain.  Over N rows per walker (all recorded rows: step 3's default
    additional_burnin = 1) and M walkers, as apf_step3.py:258-278 computes them:

    * mean = sum_w mean_w / M (= np.mean over all rows: every walker has N rows);
    * std = sqrt((sum_w M2_w + N sum_w (mean_w - mean)^2) / (N M)) (np.std over all rows);
    * w = (1/M) sum_w M2_w / N, b = N/(M-1) sum_w (mean_w - mean)^2, PSRF =
      ((N-1)/N w + (M+1)/(M N) b) / w, RC = sqrt(((d+3)//(d+1)) PSRF) (Python 2's
      integer division, see gelman_rubin);
    * acceptance = whole-run accepts / tries per parameter (apf_step2.py:362-365)."""
    names = NAMES_2 if nsrc == 2 else NAMES_3
    m = np.asarray(m, dtype=np.float64)
    ps = len(names)
    np_ = ps - 1
    if m.shape != (2 + 3 * ps + 2 * np_,):
        raise ValueError(f"moments vector of length {m.size}, expected {2 + 3 * ps + 2 * np_}")
    N, M = np.float64(m[0]), np.float64(m[1])      # NumPy floats: M = 1 gives NaN, not a raise
    sums, m2, dev = m[2:2 + ps], m[2 + ps:2 + 2 * ps], m[2 + 2 * ps:2 + 3 * ps]
    tries, acc = m[2 + 3 * ps:2 + 3 * ps + np_], m[2 + 3 * ps + np_:]
    factor = (d + 3) // (d + 1) if isinstance(d, (int, np.integer)) else (d + 3) / (d + 1)
    out = {}
    with np.errstate(all="ignore"):
        for k, name in enumerate(names):
            mean = sums[k] / M
            std = np.sqrt((m2[k] + N * dev[k]) / (N * M))
            ent = {"mean": float(mean), "std": float(std)}
            if k < np_:
                w = (1. / M) * (m2[k] / N)
                b = (N / (M - 1)) * dev[k]
                psrf = (((N - 1) / N) * w + ((M + 1) / (M * N)) * b) / w
                ent.update(gr_psrf=float(psrf), gr_rc=float(np.sqrt(factor * psrf)),
                           acceptance=float(acc[k] / tries[k]), tries=float(tries[k]),
                           accepts=float(acc[k]))
            out[name] = ent
    out["_rows_per_walker"] = int(N)
    out["_walkers"] = int(M)
    return out


def combine_moments(parts, centre_parts):
    """One summary vector from several contexts of one process (step 2's ``--gpus``
    shards): ``parts`` = each context's ``moments_summary()`` (no centre),
    ``centre_parts`` = each context's ``moments_summary(centre)`` about the pooled mean
    of ``parts`` (``pooled_mean(parts)``)."""
    parts = np.asarray(parts)
    out = parts.sum(axis=0)
    out[0] = parts[0][0]
    if not np.all(parts[:, 0] == parts[0][0]):
        raise ValueError("contexts folded different numbers of rows")
    ps = out.size // 5                 # OLPE_MOMENTS_LEN = 2 + 3 PS + 2 (PS - 1)
    out[2 + 2 * ps:2 + 3 * ps] = np.asarray(centre_parts)[:, 2 + 2 * ps:2 + 3 * ps].sum(axis=0)
    return out


def pooled_mean(parts):
    parts = np.asarray(parts)
    ps = parts.shape[1] // 5
    return parts[:, 2:2 + ps].sum(axis=0) / parts[:, 1].sum()


def main(argv=None, nsrc: int = 2):
    """The step-3 command line up to the statistics this build covers: apf_step3.py's
    arguments (positional ``image`` and ``system``, ``-s/--size`` walkers,
    ``-a/--additional_burnin``, :64-84), its read of the chain files (:160-186, native
    loader), its burn-in slice (:190-205) and its Gelman-Rubin statistics (:258-278),
    printed as the reference prints them, then per-parameter mean / median / sigma and
    the acceptance (``posterior_summary.json`` when step 2 wrote one), written to
    ``<frame>_apf_results/step3_summary.json``.
    ``--from-moments`` skips the chain files and uses step 2's device moments.
    ``--astrometry`` adds the separation / position-angle stages after :278 (``astrometry``
    below); without it nothing past the statistics runs and the outputs are unchanged.
    ``--corner`` and ``--residuals`` add the corner plot's counts and the posterior's model
    / residual images (``corner``, ``residuals`` below) in the same way, ``--autocorr`` the
    chains' integrated autocorrelation times and effective sample sizes (``autocorr``),
    ``--photometry`` the flux ratio, delta magnitude, FWHM and S/N (``photometry``),
    ``--covariance`` the parameter covariance, the companions' error ellipses, the conditional
    widths and the multivariate Gelman-Rubin statistic (``covariance``), ``--waic`` every
    pixel's posterior deviance, WAIC and DIC (``waic``), ``--detect`` the companion detection
    map, its candidates and the contrast curve (``detect``)."""
    import argparse
    import json
    import sys
    from . import pipeline
    ap = argparse.ArgumentParser(prog="apf_step3" + ("" if nsrc == 2 else "_3body"))
    ap.add_argument("image", help="the path to the image under study", type=str)
    ap.add_argument("system", help="name of the system (Simbad look-up: not used here)",
                    type=str)
    ap.add_argument("-s", "--size", help="Number of processes", type=str, required=True)
    ap.add_argument("-a", "--additional_burnin", type=int,
                    help="Additional burn in to apply to chains")
    ap.add_argument("--from-moments", action="store_true",
                    help="statistics from step 2's posterior_summary.json (device moments; "
                         "additional_burnin 1) instead of the chain files")
    ap.add_argument("--npy", action="store_true", help="read the {i}_chain.npy sidecars")
    ap.add_argument("-q", "--quiet", action="store_true")
    ap.add_argument("--astrometry", action="store_true",
                    help="separation / position angle / RA / Dec of the chains (GPU); appends "
                         "to epoch_grand_pasep and epoch_grand_radec beside the image")
    ap.add_argument("--distortion", nargs=2, metavar=("X.fits", "Y.fits"),
                    help="the NIRC2 distortion look-up tables (not shipped; without them no "
                         "distortion correction is applied)")
    ap.add_argument("--delta-r", type=float, default=0.0, metavar="MAS",
                    help="differential refraction deltaR in mas (apf_step3.py:391; default 0)")
    ap.add_argument("--prepost", choices=("pre", "post"),
                    help="distortion epoch (default: from the year the image's directory "
                         "name starts with, apf_step3.py:149-153)")
    ap.add_argument("--corner", action="store_true",
                    help="the corner plot's 1-D / 2-D histograms and 16/50/84 %% quantile "
                         "brackets of the chains (GPU); writes <frame>_corner.npz")
    ap.add_argument("--corner-bins", type=int, default=20, metavar="N",
                    help="bins per axis of the 2-D histograms (corner's default 20)")
    ap.add_argument("--corner-fine-bins", type=int, default=2048, metavar="N",
                    help="bins of the 1-D histograms the quantile brackets are read from")
    ap.add_argument("--residuals", action="store_true",
                    help="posterior mean / scatter of the model and the best sample's "
                         "residual images of the chains (GPU); writes <frame>_residuals.npz "
                         "and four FITS files")
    ap.add_argument("--residuals-thin", type=int, default=1, metavar="N",
                    help="fold every N-th row after the burn-in (a full fold costs about "
                         "what sampling the rows did)")
    ap.add_argument("--bkgd-mode", type=int, choices=(0, 1), default=0,
                    help="the background parameter of the models --residuals evaluates: 0 as "
                         "step 2's default, 1 as its --fixed-bkgd")
    ap.add_argument("--waic", action="store_true",
                    help="posterior mean / scatter of every pixel's deviance, WAIC and DIC of "
                         "the chains (GPU); writes <frame>_waic.npz and three FITS files")
    ap.add_argument("--waic-thin", type=int, default=1, metavar="N",
                    help="fold every N-th row after the burn-in (a full fold costs more "
                         "than sampling the rows did)")
    ap.add_argument("--waic-against", type=str, default=None, metavar="FILE",
                    help="with --waic: compare pixel by pixel with another run's "
                         "<frame>_waic.npz of the same cutout (2 against 3 sources, "
                         "--bkgd-mode 0 against 1)")
    ap.add_argument("--autocorr", action="store_true",
                    help="integrated autocorrelation time and effective sample size per "
                         "parameter of the chains (GPU); writes <frame>_autocorr.npz")
    ap.add_argument("--autocorr-max-lag", type=int, default=512, metavar="N",
                    help="largest lag in recorded rows (a multiple of 64, 64 to 1024)")
    ap.add_argument("--autocorr-c", type=float, default=5.0, metavar="X",
                    help="the window is the smallest M with M >= X tau(M) (emcee's c = 5)")
    ap.add_argument("--photometry", action="store_true",
                    help="flux ratio, delta magnitude, primary flux, FWHM and core fraction of "
                         "every chain row (GPU), the reference's aperture S/N and FWHM (host); "
                         "writes <frame>_photometry.npz and, with --astrometry, the S/N and "
                         "FWHM fields of the epoch_grand_pasep line")
    ap.add_argument("--photometry-thin", type=int, default=1, metavar="N",
                    help="fold every N-th row after the burn-in")
    ap.add_argument("--covariance", action="store_true",
                    help="parameter covariance and correlations, the companions' error "
                         "ellipses (detector frame), conditional widths and the multivariate "
                         "Gelman-Rubin statistic of the chains (GPU); writes "
                         "<frame>_covariance.npz")
    ap.add_argument("--covariance-thin", type=int, default=1, metavar="N",
                    help="fold every N-th row after the burn-in")
    ap.add_argument("--widths-out", type=str, default=None, metavar="FILE",
                    help="with --covariance: write the proposal widths the fold implies "
                         "(covariance.proposal_widths) as a widths file for step 2's --widths")
    ap.add_argument("--detect", action="store_true",
                    help="companion detection map and contrast curve of the chains (GPU): the "
                         "matched filter of every folded row's residual with its own PSF at "
                         "every candidate position; writes <frame>_detect.npz and three FITS "
                         "files")
    ap.add_argument("--detect-thin", type=int, default=1, metavar="N",
                    help="fold every N-th row after the burn-in (a row costs 2 G n^2 FMAs: "
                         "thin generously)")
    ap.add_argument("--detect-oversample", type=int, choices=(1, 2, 4), default=1,
                    help="candidate positions per pixel and axis")
    ap.add_argument("--detect-threshold", type=float, default=5.0, metavar="X",
                    help="candidates are the local maxima of the S/N map at or above X")
    ap.add_argument("--detect-k", type=float, default=5.0, metavar="K",
                    help="the contrast curve is K sigma over the primary's flux")
    ap.add_argument("--detect-null", type=int, default=0, metavar="R",
                    help="with --detect: calibrate the map's false-alarm rate on R noise "
                         "realisations drawn and matched-filtered on the GPU at the column "
                         "means; writes <frame>_detect_null.npz")
    ap.add_argument("--detect-null-seed", type=int, default=0, metavar="S",
                    help="realisation r draws from RandomState((S + r) mod 2^32)")
    ap.add_argument("--detect-fap", type=float, default=0.01, metavar="P",
                    help="the per-map (and per-ring) false-alarm probability the calibrated "
                         "threshold and contrast curve are quoted for")
    args = ap.parse_args(sys.argv[1:] if argv is None else argv)
    say = (lambda *a: None) if args.quiet else print
    ncor = int(np.int_(args.size))                                  # :76-77
    additional_burnin = args.additional_burnin or 1                 # :81-84
    _, _, input_directory = pipeline.image_paths(args.image)       # :138-143
    names = NAMES_2 if nsrc == 2 else NAMES_3
    if args.from_moments and additional_burnin != 1:
        # the device moments fold every recorded row (additional_burnin = 1): a larger
        # burn-in cannot be taken out of them afterwards
        ap.error(f"--from-moments covers every recorded row (additional_burnin 1); "
                 f"-a {additional_burnin} needs the chain files")
    if args.from_moments and args.covariance:
        ap.error("--covariance needs the chain rows (per-column moments hold no cross "
                 "terms): drop --from-moments")
    if args.covariance and args.covariance_thin < 1:
        ap.error(f"--covariance-thin {args.covariance_thin}: must be >= 1")
    if args.widths_out and not args.covariance:
        ap.error("--widths-out writes the widths of the --covariance fold: give --covariance")
    for flag, why in (("astrometry", "a median is not a moment"),
                      ("corner", "a histogram is not a moment"),
                      ("residuals", "moments are not samples"),
                      ("waic", "moments are not samples"),
                      ("detect", "moments are not samples"),
                      ("autocorr", "moments hold no order"),
                      ("photometry", "a percentile is not a moment")):
        if args.from_moments and getattr(args, flag):
            ap.error(f"--{flag} needs the chain rows ({why}): drop --from-moments")
    if args.autocorr and (args.autocorr_max_lag < 64 or args.autocorr_max_lag > 1024
                          or args.autocorr_max_lag % 64):
        ap.error(f"--autocorr-max-lag {args.autocorr_max_lag}: a multiple of 64 from 64 to 1024")
    if args.residuals_thin < 1:
        ap.error(f"--residuals-thin {args.residuals_thin}: must be >= 1")
    if args.waic_thin < 1:
        ap.error(f"--waic-thin {args.waic_thin}: must be >= 1")
    if args.detect_thin < 1:
        ap.error(f"--detect-thin {args.detect_thin}: must be >= 1")
    if args.detect_null and not args.detect:
        ap.error("--detect-null calibrates the --detect map: give --detect")
    if args.detect_null < 0 or args.detect_null_seed < 0:
        ap.error(f"--detect-null {args.detect_null}, --detect-null-seed "
                 f"{args.detect_null_seed}: must be >= 0")
    if not 0.0 < args.detect_fap < 1.0:
        ap.error(f"--detect-fap {args.detect_fap}: between 0 and 1")
    if args.waic_against and not args.waic:
        ap.error("--waic-against compares the --waic fold: give --waic")
    if args.photometry_thin < 1:
        ap.error(f"--photometry-thin {args.photometry_thin}: must be >= 1")
    if args.from_moments:
        with open(input_directory + "posterior_summary.json") as f:
            summ = json.load(f)
        if summ.get("_walkers") != ncor:
            raise ValueError(f"posterior_summary.json holds {summ.get('_walkers')} walkers, "
                             f"-s gives {ncor}")
        stats = {k: summ[k] for k in names[:-1]}
        length = summ["_rows_per_walker"] + 1
    else:
        say('Importing parameter arrays...')                        # :167
        chains = load_chains(input_directory, ncor, 0, source="npy" if args.npy else "csv")
        length = chains.shape[0]
        if length - additional_burnin < 1:
            raise ValueError(f"{input_directory}: {length} rows per walker file, none left "
                             f"after additional_burnin = {additional_burnin} (step 2's "
                             f"burn-in may exceed its run)")
        say('Parameter array shape:', length)                       # :172
        chains = chains[additional_burnin:length]                   # :190-205
        stats = summary(chains, nsrc)
    N = length - additional_burnin
    say("Number of total jumps per walker:", length)                # :202-204
    say("Number of jumps after additional burn in:", N)
    say("Number of total samples after burn-in: ", N * ncor)
    rc = np.array([stats[k]["gr_rc"] for k in names[:-1]])
    say('Mean and stdev Gelman-Rubin stat for parameter chains:', np.mean(rc), np.std(rc))
    say('GR for positions:', *rc[:4])                               # :277-278
    if not args.from_moments:
        try:
            with open(input_directory + "posterior_summary.json") as f:
                moments = json.load(f)
            for k in names[:-1]:
                for key in ("acceptance", "tries", "accepts"):
                    if key in moments.get(k, {}):
                        stats[k][key] = moments[k][key]
        except (OSError, ValueError):
            pass
    for k in names[:-1]:
        s = stats[k]
        say(f"{k:>9} mean {s['mean']:.10g} median {s.get('median', float('nan')):.10g} "
            f"std {s['std']:.6g} GR {s['gr_rc']:.6f}")
    out = {"walkers": ncor, "rows_per_walker": N, "additional_burnin": additional_burnin,
           "source": "moments" if args.from_moments else ("npy" if args.npy else "csv"),
           "gr_rc_mean": float(np.mean(rc)), "gr_rc_std": float(np.std(rc)),
           "parameters": stats}
    phot, phot_ref = (photometry(args, chains, nsrc, input_directory, say) if args.photometry
                      else (None, None))
    if args.astrometry:
        out["astrometry"] = astrometry(args, chains, nsrc, float(np.mean(rc)),
                                       float(np.std(rc)), say, photometry=phot_ref)
    if args.corner:
        out["corner"] = corner(args, chains, nsrc, input_directory, say)
    if args.residuals:
        out["residuals"] = residuals(args, chains, nsrc, input_directory, say)
    if args.autocorr:
        out["autocorr"] = autocorr(args, chains, nsrc, input_directory, say)
    if phot:
        out["photometry"] = phot
    if args.covariance:
        out["covariance"] = covariance(args, chains, nsrc, stats, input_directory, say)
    if args.waic:
        out["waic"] = waic(args, chains, nsrc, stats, input_directory, say)
    if args.detect:
        out["detect"] = detect(args, chains, nsrc, stats, input_directory, say)
    with open(input_directory + "step3_summary.json", "w") as f:
        json.dump(out, f, indent=1)
    return out


def results_prefix(args, input_directory):
    """The results directory and the frame's name: what the stages' file names begin with."""
    return input_directory + args.image.split('/')[-1].split('.')[-3]


def autocorr(args, chains, nsrc, input_directory, say=print):
    """The numbers behind the reference's chain plot (apf_step3.py:582-601;
    3body/apf_step3_3body.py likewise), which is read by eye: an integrated autocorrelation
    time and an effective sample size per column of the chains [N, M, PS] already read, each
    walker's file one series, the lag sums folded on the GPU (autocorr.Autocorr) from the
    rows as they lie (time-major).  Writes ``<frame>_autocorr.npz`` beside the chain files
    and returns what ``step3_summary.json`` records.  tau is in recorded rows."""
    from . import autocorr as ac
    labels = NAMES_2 if nsrc == 2 else NAMES_3
    say('Computing autocorrelation times...')
    path = results_prefix(args, input_directory) + '_autocorr.npz'
    with ac.Autocorr(chains.shape[2], args.autocorr_max_lag, labels=labels) as a:
        a.fold_rows(chains, time_major=True)
        st, res = a.save(path, c=args.autocorr_c)
    for line in ac.table_lines(res):
        say(line)
    say("Smallest effective sample size:", res["min_ess"])

    def num(v):                                   # JSON has no NaN
        return float(v) if np.isfinite(v) else None
    return {"file": path, "max_lag": args.autocorr_max_lag, "c": args.autocorr_c,
            "tol": res["tol"], "n": st["n"], "series": st["series"], "skipped": st["skipped"],
            "min_ess": num(res["min_ess"]),
            "columns": {name: {"tau": num(res["tau"][k]), "window": int(res["window"][k]),
                               "windowed": bool(res["windowed"][k]),
                               "reliable": bool(res["reliable"][k]), "ess": num(res["ess"][k]),
                               "suggested_stride": int(res["suggested_stride"][k]),
                               "note": res["notes"][k]}
                        for k, name in enumerate(labels)}}


def covariance(args, chains, nsrc, stats, input_directory, say=print):
    """What the per-column statistics above cannot say (the reference's corner figure,
    apf_step3.py:603-643, shows the pair scatter and gives no number for it): the covariance
    and correlation matrix of the chains [N, M, PS] already read, the error ellipse of each
    companion's offset from the primary (detector frame; pixscale the header's, as
    ``photometry`` takes it), each parameter's conditional width given all the others, and
    Brooks & Gelman's multivariate R-hat over the walkers.  The cross-column sums are folded
    on the GPU (covariance.Covariance) from every ``--covariance-thin``-th row as the rows
    lie (time-major), one walker per chain file, about the column means just computed.  The
    conditional widths and R-hat run over the parameters; chi^2 is left out.  Writes
    ``<frame>_covariance.npz`` beside the chain files and returns what
    ``step3_summary.json`` records."""
    from . import astrometry as am, covariance as cv, fitsio
    labels = NAMES_2 if nsrc == 2 else NAMES_3
    _, hdr = fitsio.getdata_header(args.image)
    prepost = resolve_prepost(args)
    pixscale = am.header_scalars(hdr, prepost)["pixscale"]
    say('Computing parameter covariance...')
    thinned = chains[::args.covariance_thin]
    # the pivot: the column means (chi^2's, which summary leaves out, from the rows folded)
    pivot = np.array([stats[k]["mean"] for k in labels[:-1]]
                     + [float(np.mean(thinned[..., -1]))])
    pivot = np.where(np.isfinite(pivot), pivot, 0.0)
    path = results_prefix(args, input_directory) + '_covariance.npz'
    with cv.Covariance(chains.shape[2], walkers=chains.shape[1], pivot=pivot,
                       labels=labels) as c:
        c.fold_rows(thinned, time_major=True)
        st, res = c.save(path, nsrc=nsrc, pixscale=pixscale,
                         param_cols=range(chains.shape[2] - 1))
    for line in cv.table_lines(res):
        say(line)
    if getattr(args, "widths_out", None):
        # the loop's closing edge: this fold -> step 2's --widths
        from . import tune
        tune.save_widths(args.widths_out, nsrc, cv.proposal_widths(st, nsrc), "covariance")
        say("Proposal widths written to", args.widths_out)

    def num(v):                                   # JSON has no NaN
        return float(v) if v is not None and np.isfinite(v) else None
    cs, mp = res["conditional"], res["mpsrf"]
    return {"file": path, "thin": args.covariance_thin, "prepost": prepost,
            "pixscale": pixscale, "n": st["n"], "skipped": st["skipped"],
            "walkers": st["walkers"],
            "largest_correlations": [{"a": a, "b": b, "r": num(r)} for a, b, r in res["pairs"]],
            "ellipses": {e["name"]: {"semi_major_px": num(e["semi_major"]),
                                     "semi_minor_px": num(e["semi_minor"]),
                                     "semi_major_mas": num(e["semi_major_mas"]),
                                     "semi_minor_mas": num(e["semi_minor_mas"]),
                                     "angle_deg": num(e["angle"]), "rho": num(e["rho"])}
                         for e in res["ellipses"]},
            "condition": num(cs["condition"]),
            "columns": {labels[k]: {"sigma": num(cs["sigma_marginal"][i]),
                                    "sigma_conditional": num(cs["sigma_cond"][i]),
                                    "efficiency": num(cs["efficiency"][i]),
                                    "rhat": num(mp["rhat"][i]), "note": res["notes"][k]}
                        for i, k in enumerate(cs["cols"])},
            "mpsrf": num(mp["mpsrf"]), "mpsrf_note": mp["note"]}


def corner(args, chains, nsrc, input_directory, say=print):
    """apf_step3.py:603-643 (3body/apf_step3_3body.py:680-726) without the drawing: the
    1-D and 2-D histograms ``corner.corner`` would compute over the chains [N, M, PS]
    already read, and its titles' quantiles as brackets, counted on the GPU
    (corner.Corner) over corner's default range (each column's min / max).  Writes
    ``<frame>_corner.npz`` beside the chain files and returns what ``step3_summary.json``
    records.  The columns are the chain files' (chi^2 included); the reference's sep / pa
    columns are not added here."""
    from . import corner as cn
    labels = cn.LABELS_2 if nsrc == 2 else cn.LABELS_3
    say('Creating a corner plot...')                                    # :605
    path = results_prefix(args, input_directory) + '_corner.npz'        # :643
    with cn.Corner(cn.Corner.ranges_of(chains), bins=args.corner_bins,
                   fine_bins=args.corner_fine_bins, labels=labels) as c:
        c.fold_rows(chains)
        counts, table = c.save(path)
    for k, name in enumerate(labels):
        say(f"{name:>10} " + "  ".join(
            f"{100 * q:g}%: {e:.10g} [{lo:.10g}, {hi:.10g}]" for q, e, lo, hi in
            zip(table["q"], table["estimate"][k], table["lo"][k], table["hi"][k])))
    return {"file": path, "samples": counts["n"], "bins": args.corner_bins,
            "fine_bins": args.corner_fine_bins, "labels": labels, "q": table["q"],
            "quantiles": {name: {"lo": [float(v) for v in table["lo"][k]],
                                 "hi": [float(v) for v in table["hi"][k]],
                                 "estimate": [float(v) for v in table["estimate"][k]]}
                          for k, name in enumerate(labels)},
            "outside": [int(v) for v in counts["outside1"]]}


def residuals(args, chains, nsrc, input_directory, say=print):
    """The picture the reference's README opens with (data, model, residual) over the
    chains [N, M, PS] already read, without the drawing: every ``--residuals-thin``-th row's
    ``build_analytical_model`` (apf_step2.py:106-124; 3body :106-125) folded on the GPU
    (residuals.Residuals) on the frame as step 2 staged it (apf_step2.py:160-161,
    :176-210).  Writes ``<frame>_residuals.npz`` and ``<frame>_model.fits``,
    ``_meanmodel.fits``, ``_resid.fits``, ``_nresid.fits`` beside the chain files and
    returns what ``step3_summary.json`` records."""
    from . import fitsio, residuals as rs
    from .core import Sampler
    image, hdr = fitsio.getdata_header(args.image)
    say('Building model and residual images...')
    prefix = results_prefix(args, input_directory)
    with Sampler(image, hdr["ITIME"], hdr["COADDS"], hdr["MULTISAM"], hdr["SAMPMODE"],
                 nsrc=nsrc, bkgd_mode=args.bkgd_mode) as s, rs.Residuals(s) as r:
        r.fold_rows(chains[::args.residuals_thin])
        _, scal = r.save(prefix + "_residuals.npz")
        files = r.write_fits(prefix)
    for k, v in scal.items():
        say(f"{k:>18} {v:.10g}")
    return {"file": prefix + "_residuals.npz", "fits": files, "thin": args.residuals_thin,
            "bkgd_mode": args.bkgd_mode, **scal}


def waic(args, chains, nsrc, stats, input_directory, say=print):
    """What the reference's chi^2 column (apf_step2.py:134-148; 3body :134-148), which is
    only plotted, cannot say: how well the model predicts every pixel over the chains
    [N, M, PS] already read, and which of two runs predicts the image better.  Every
    ``--waic-thin``-th row's ``build_analytical_model`` (apf_step2.py:106-124; 3body
    :106-125) is evaluated on the GPU (predictive.Predictive) on the frame as step 2 staged
    it (apf_step2.py:160-161, :176-210; ``--bkgd-mode`` as ``--residuals``) and its
    per-pixel deviance folded; theta_hat of DIC is the column means just computed.  Writes
    ``<frame>_waic.npz`` and ``<frame>_meandev.fits``, ``_elpd.fits``, ``_pwaic.fits``
    beside the chain files and returns what ``step3_summary.json`` records.
    ``--waic-against`` adds ``predictive.compare`` of this run against another's npz."""
    from . import fitsio, predictive as pr
    from .core import Sampler
    labels = NAMES_2 if nsrc == 2 else NAMES_3
    image, hdr = fitsio.getdata_header(args.image)
    say('Folding pointwise deviance (WAIC, DIC)...')
    prefix = results_prefix(args, input_directory)
    theta_hat = np.array([stats[k]["mean"] for k in labels[:-1]])
    if not np.isfinite(theta_hat).all():
        raise ValueError("a column mean is not finite: --waic needs an additional_burnin "
                         "that drops the NaN seed row")
    with Sampler(image, hdr["ITIME"], hdr["COADDS"], hdr["MULTISAM"], hdr["SAMPMODE"],
                 nsrc=nsrc, bkgd_mode=args.bkgd_mode) as s, pr.Predictive(s) as p:
        p.fold_rows(chains[::args.waic_thin])
        _, scal = p.save(prefix + "_waic.npz", theta_hat=theta_hat, thin=args.waic_thin)
        files = p.write_fits(prefix, theta_hat=theta_hat)
    cmp_ = None
    if args.waic_against:
        cmp_ = pr.compare(prefix + "_waic.npz", args.waic_against)
        cmp_["file"] = args.waic_against
    for line in pr.table_lines(scal, cmp_):
        say(line)

    def num(v):                                   # JSON has no NaN
        return v if isinstance(v, int) else (float(v) if np.isfinite(v) else None)
    out = {"file": prefix + "_waic.npz", "fits": files, "thin": args.waic_thin,
           "bkgd_mode": args.bkgd_mode, **{k: num(v) for k, v in scal.items()}}
    if cmp_ is not None:
        out["against"] = {k: (v if isinstance(v, str) else num(v)) for k, v in cmp_.items()}
    return out


def detect(args, chains, nsrc, stats, input_directory, say=print):
    """Is there another source in the frame, and how faint a one would have been seen?  Over
    the chains [N, M, PS] already read, every ``--detect-thin``-th row's residual
    (``build_analytical_model``, apf_step2.py:106-124; 3body :106-125) is matched-filtered
    with that row's own unit PSF (apf_step2.py:78-103) at every candidate position on the GPU
    (detect.Detect) on the frame as step 2 staged it (apf_step2.py:160-161, :176-210;
    ``--bkgd-mode`` as ``--residuals``), about theta_hat, the column means just computed.
    Prints the scalars, the candidates above ``--detect-threshold`` and the ``--detect-k``
    sigma contrast curve; writes ``<frame>_detect.npz`` and ``<frame>_snr.fits``,
    ``_sigma.fits``, ``_contrast.fits`` beside the chain files and returns what
    ``step3_summary.json`` records."""
    from . import astrometry as am, detect as dt, fitsio
    from .core import Sampler
    labels = NAMES_2 if nsrc == 2 else NAMES_3
    image, hdr = fitsio.getdata_header(args.image)
    pixscale = am.PIXSCALE[resolve_prepost(args)]    # the scale alone: no pointing cards needed
    say('Folding the companion detection map...')
    prefix = results_prefix(args, input_directory)
    theta_hat = np.array([stats[k]["mean"] for k in labels[:-1]])
    if not np.isfinite(theta_hat).all():
        raise ValueError("a column mean is not finite: --detect needs an additional_burnin "
                         "that drops the NaN seed row")
    os_ = args.detect_oversample
    flux0, known = dt.flux0_of(theta_hat, nsrc), dt.known_of(theta_hat, nsrc)
    with Sampler(image, hdr["ITIME"], hdr["COADDS"], hdr["MULTISAM"], hdr["SAMPMODE"],
                 nsrc=nsrc, bkgd_mode=args.bkgd_mode) as s, \
            dt.Detect(s, pivot=theta_hat, oversample=os_) as d:
        d.fold_rows(chains[::args.detect_thin])
        img, scal = d.finalize()
        img, scal = dict(zip(dt.PLANES, img)), d._scalars(scal)
        curve = dt.contrast_curve(img["sigma_total"], known[0], flux0, pixscale,
                                  k=args.detect_k, oversample=os_)
        cands = dt.candidates(img["snr_marg"], img["amp_mean"], img["sigma_total"], known,
                              threshold=args.detect_threshold,
                              exclude_px=dt.default_exclude_px(theta_hat, nsrc),
                              oversample=os_, flux0=flux0, pixscale=pixscale)
        keys = ("x", "y", "snr", "amp", "sigma", "contrast", "dmag", "sep_px", "pa_deg")
        d.save(prefix + "_detect.npz", thin=np.int64(args.detect_thin),
               bkgd_mode=np.int64(args.bkgd_mode), theta_hat=theta_hat,
               flux0=np.float64(flux0), pixscale=np.float64(pixscale),
               k=np.float64(args.detect_k), threshold=np.float64(args.detect_threshold),
               candidates=np.array([[c[k] for k in keys] for c in cands]).reshape(-1, len(keys)),
               candidates_flagged=np.array([c["flagged"] for c in cands], dtype=bool),
               **{"curve_" + k: v for k, v in curve.items()})
        files = d.write_fits(prefix, flux0=flux0, k=args.detect_k)
        null = (detect_null(args, d, theta_hat, img, cands, curve, known, flux0, prefix)
                if args.detect_null else None)
    for line in dt.table_lines(scal, cands, curve):
        say(line)
    if null:
        for line in null.pop("lines"):
            say(line)

    def num(v):                                   # JSON has no NaN
        if isinstance(v, (bool, int, str)):
            return v
        return float(v) if np.isfinite(v) else None
    out = {"file": prefix + "_detect.npz", "fits": files, "thin": args.detect_thin,
           "oversample": os_, "bkgd_mode": args.bkgd_mode, "threshold": args.detect_threshold,
           "k": args.detect_k, "flux0": num(flux0), **{k: num(v) for k, v in scal.items()},
           "candidates": [{k: num(v) for k, v in c.items()} for c in cands],
           "curve": {k: [num(x) for x in np.asarray(v).tolist()] for k, v in curve.items()}}
    if null:
        def clean(v):
            if isinstance(v, (list, tuple)):
                return [clean(x) for x in v]
            return v if v is None else num(v)
        out["detect_null"] = {k: clean(v) for k, v in null.items()}
    return out


def detect_null(args, d, theta_hat, img, cands, curve, known, flux0, prefix):
    """What does ``--detect-threshold`` mean?  ``--detect-null`` R noise realisations of the
    frame's own err (apf_step2.py:210) are drawn and matched-filtered on the GPU at theta_hat
    (detect_null.DetectNull) with the denominator of ``snr_marg``, the map the candidates are
    taken from: scale = sigma_A(theta_hat) / sigma_total.  Writes ``<frame>_detect_null.npz``
    and returns the scalars ``step3_summary.json`` records, with the ``lines`` to print."""
    from . import detect as dt, detect_null as dn
    os_ = args.detect_oversample
    with np.errstate(all="ignore"):
        scale = d.point(theta_hat)[1] / img["sigma_total"]
    scale = np.where(np.isfinite(scale) & (scale > 0.0), scale, 1.0)
    ex = dt.default_exclude_px(theta_hat, d.nsrc)
    with dn.DetectNull(d, theta_hat, scale=scale, known=known, exclude_px=ex, centre=known[0],
                       threshold=args.detect_threshold, seed=args.detect_null_seed) as h:
        h.run(args.detect_null)
        res = h.results()
    summ = dn.summarise(res, args.detect_threshold, args.detect_fap, cands=cands)
    ring_k = dn.ring_thresholds(res["ring_max"], args.detect_fap)
    cal = dn.calibrated_curve(curve, img["sigma_total"], ring_k, known[0], flux0, oversample=os_)
    with open(prefix + "_detect_null.npz", "wb") as f:
        np.savez(f, **{k: np.asarray(v) for k, v in res.items()}, scale=scale, ring_k=ring_k,
                 fap=np.float64(args.detect_fap), seed=np.int64(args.detect_null_seed),
                 **{"curve_" + k: cal[k] for k in ("k", "contrast_median_cal", "contrast_min_cal",
                                                   "dmag_median_cal", "dmag_min_cal")})
    return {"file": prefix + "_detect_null.npz", "seed": args.detect_null_seed, **summ,
            "curve_k": cal["k"].tolist(), "curve_dmag_median_cal": cal["dmag_median_cal"].tolist(),
            "lines": dn.table_lines(summ, cands, cal)}


def resolve_prepost(args):
    """--prepost, or apf_step3.py:149-153's choice by the year the image's directory name
    starts with."""
    from . import astrometry as am
    if args.prepost is not None:
        return args.prepost
    try:
        return am.prepost_of(am.epoch_of(args.image))                   # :149-153
    except (ValueError, IndexError):
        raise ValueError(f"{args.image}: the directory name does not start with the "
                         f"epoch's year (apf_step3.py:149); give --prepost") from None


def photometry(args, chains, nsrc, input_directory, say=print):
    """The photometry of the chains [N, M, PS] already read.  On the GPU
    (photometry.Photometry): every ``--photometry-thin``-th row's flux ratio and delta
    magnitude per companion, the primary's integrated flux, the FWHM of the narrow and the
    wide Gaussian and the core fraction (the model of apf_step2.py:78-124; 3body :78-125),
    summarised by median, 16 / 84 % percentiles, mean and np.std.  On the host: what the
    reference's own block computes (apf_step3.py:452-511; 3body :520-569), FWHMmean /
    FWHMstd over the last 100 rows and the sources' aperture S/N, which fill the pasep
    line's fields under ``--astrometry``.  pixscale is the header's (apf_step3.py:224 /
    :231, by ``--prepost`` or the epoch).  Writes ``<frame>_photometry.npz`` beside the
    chain files and returns what ``step3_summary.json`` records, then the host numbers as
    ``photometry.reference_numbers`` gives them (for ``astrometry``'s pasep line)."""
    from . import astrometry as am, fitsio, photometry as ph
    image, hdr = fitsio.getdata_header(args.image)
    prepost = resolve_prepost(args)
    pixscale = am.header_scalars(hdr, prepost)["pixscale"]
    say('Computing photometry...')
    thinned = chains[::args.photometry_thin]
    with ph.Photometry(chains.shape[1], thinned.shape[0], variant=nsrc, ps=chains.shape[2],
                       pixscale=pixscale) as p:
        p.fold_rows(thinned)
        res = p.finalize(ph.DEFAULT_PROBS)
        unusable, planes = p.unusable, p.planes
    ref = ph.reference_numbers(image, chains, pixscale, nsrc)
    table = np.array([[res[k]["percentiles"][1], res[k]["percentiles"][0],
                       res[k]["percentiles"][2], res[k]["mean"], res[k]["std"], res[k]["min"],
                       res[k]["max"]] for k in planes])
    for k, t in zip(planes, table):
        say(f"{k:>16} median {t[0]:.10g} -{t[0] - t[1]:.6g} +{t[2] - t[0]:.6g} "
            f"mean {t[3]:.10g} std {t[4]:.6g}")
    say("Unusable rows:", unusable)
    say("FWHM (reference, last 100 rows):", ref["fwhm_mean"], ref["fwhm_std"])
    say("S/N (reference apertures):", *ref["snr"])
    path = results_prefix(args, input_directory) + '_photometry.npz'
    np.savez(path, planes=np.array(planes), table=table,
             columns=np.array(["median", "p16", "p84", "mean", "std", "min", "max"]),
             probs=np.array(ph.DEFAULT_PROBS), counts=np.array([res[k]["n"] for k in planes]),
             unusable=np.int64(unusable), thin=np.int64(args.photometry_thin),
             pixscale=np.float64(pixscale), snr=np.array(ref["snr"]),
             fwhm_mean=np.float64(ref["fwhm_mean"]), fwhm_std=np.float64(ref["fwhm_std"]),
             positions=np.array(ref["positions"]))

    def num(v):                                   # JSON has no NaN
        return float(v) if np.isfinite(v) else None
    return {"file": path, "thin": args.photometry_thin, "prepost": prepost,
            "pixscale": pixscale, "rows": int(thinned.shape[0]), "unusable": unusable,
            "probs": list(ph.DEFAULT_PROBS),
            "planes": {k: {"n": res[k]["n"], "median": num(res[k]["percentiles"][1]),
                           "p16": num(res[k]["percentiles"][0]),
                           "p84": num(res[k]["percentiles"][2]), "mean": num(res[k]["mean"]),
                           "std": num(res[k]["std"]), "min": num(res[k]["min"]),
                           "max": num(res[k]["max"])} for k in planes},
            "reference": {"positions": ref["positions"], "snr": [num(v) for v in ref["snr"]],
                          "fwhm_mean": num(ref["fwhm_mean"]),
                          "fwhm_std": num(ref["fwhm_std"])}}, ref


def astrometry(args, chains, nsrc, rc_mean, rc_std, say=print, photometry=None):
    """apf_step3.py:211-256, :283-343, :401-450 and the two result lines of :517-546
    (3body/apf_step3_3body.py:247-288, :315-390, :450-518, :575-613) for the chains
    [N, M, PS] already read: the per-sample work and every reduction on the GPU
    (astrometry.Astrometry), the header's scalars on the host.  Appends to
    ``epoch_grand_pasep`` / ``epoch_grand_radec`` beside the image and returns what
    ``step3_summary.json`` records.  deltaR is ``--delta-r`` (computing it needs a network
    name resolver: not covered); the S/N and FWHM fields are ``photometry``'s (what
    ``photometry()`` below returns under ``"reference"``), ``nan`` without it."""
    from . import astrometry as am, fitsio, pipeline
    image, hdr = fitsio.getdata_header(args.image)
    directory, _, _ = pipeline.image_paths(args.image)
    prepost = resolve_prepost(args)
    x_dist = y_dist = None
    if args.distortion:
        x_dist = np.asarray(fitsio.getdata_header(args.distortion[0])[0], dtype=np.float64)
        y_dist = np.asarray(fitsio.getdata_header(args.distortion[1])[0], dtype=np.float64)
        say('Correcting plate scale distortion...')                     # :217
    else:
        say('No distortion tables given (--distortion): no distortion correction applied')
    say('Computing separation and position angle...')                   # :282
    with am.Astrometry.from_header(hdr, chains.shape[1], chains.shape[0], prepost=prepost,
                                   variant=nsrc, image_shape=image.shape, x_dist=x_dist,
                                   y_dist=y_dist) as a:
        a.fold_rows(chains)
        scal = a.scalars
        res = a.finalize(delta_r=args.delta_r)
    say('Computing median values...')                                   # :435
    for r in res:
        say("r%s = " % r["pair"], r["sep_median"], "pa%s = " % r["pair"], r["pa_median"])
    koaid = hdr.get('KOAID', '')
    pasep = am.pasep_line(koaid, res, rc_mean, rc_std, nsrc, photometry=photometry)
    radec = am.radec_line(koaid, res)
    with open(directory + 'epoch_grand_pasep', 'a') as f:               # :529-533
        f.write(pasep + "\n")
    with open(directory + 'epoch_grand_radec', 'a') as f:               # :536-546
        f.write(radec + "\n")
    return {"pairs": res, "delta_r_mas": args.delta_r, "parantel": scal["parantel"],
            "prepost": prepost, "pixscale": scal["pixscale"],
            "rotation_angle": scal["rotation_angle"],
            "vertical_angle_mode": scal["vertical_angle_mode"], "rotcorr": scal["rotcorr"],
            "distortion": list(args.distortion) if args.distortion else None,
            "pasep_line": pasep, "radec_line": radec}
