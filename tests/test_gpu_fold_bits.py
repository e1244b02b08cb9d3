"""The step-3 folds' summaries, bit for bit, against a recording of the library before the
block reductions, the stage-2 kernel, the sample store and the order-statistic bracket got one
home each (olpe_reduce.h, olpe_store.h, olpe_select.h; tests/golden/fold_bits_parent.npz,
written by tools/record_fold_bits_golden.py).

Every case is the smallest shape that reaches a place where shared code can go wrong: dead
lanes' zeros through block_sum, a ragged second stage-1 partial, 257 partials for the 256
threads of the stage-2 kernels, second trips of the grid-stride kernels, the median's upper
neighbour (n even) and the single-rank median (n odd), NaN-skipping reductions with live
count / min / max words, idle threads in cov_between_kernel.  Inputs come from fixed
RandomState seeds; outputs are compared as 64-bit words.

The two 257-partial cases print a host clock around finalize (it ends in a read-back, which
synchronises): toy-sized, mostly launch and copy overhead.
"""
import time

import numpy as np
import pytest

import fold_scale_cases as fc
import moments_restatement as mr
import test_gpu_astrometry as ta
import test_gpu_moments as tm
import test_gpu_photometry as tp
from olpefit_amd.astrometry import Astrometry
from olpefit_amd.autocorr import Autocorr
from olpefit_amd.covariance import Covariance
from olpefit_amd.photometry import Photometry

pytestmark = pytest.mark.gpu

GOLDEN = "fold_bits_parent"
ASTROM_KEYS = ("sep_median", "sep_std", "pa_median", "pa_std", "ra", "ra_std", "dec", "dec_std",
               "pa_mean_uncorrected", "branch_code", "samples", "added_360")
PHOT_KEYS = ("n", "mean", "std", "min", "max", "passes")


def words(x):
    """x as 64-bit words: the bits of doubles, the values of integers."""
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x.astype(np.uint64)


def clocked(what, fn):
    t0 = time.perf_counter()
    out = fn()
    print(f"{what}: finalize {1e3 * (time.perf_counter() - t0):.3f} ms (host clock, toy size)")
    return out


# ------------------------------------------------------------------------------ astrometry
def astrom(W, rows, variant, seed, clock=None):
    """finalize's whole output per pair, [npairs][16], with the tables and delta_r = 35."""
    chain = ta.make_chain(W, rows, variant, seed=seed)
    s = ta.scalars(rotation_angle=10.0)
    with Astrometry(W, rows, variant=variant, pixscale=s["pixscale"],
                    rotation_angle=s["rotation_angle"], rotcorr=s["rotcorr"],
                    use_rotcorr=s["use_rotcorr"], parantel=s["parantel"], x_dist=ta.XD,
                    y_dist=ta.YD, xdiff=ta.XDIFF, ydiff=ta.YDIFF) as a:
        a.fold_rows(chain)
        fin = lambda: a.finalize(delta_r=35.0)
        res = clocked(clock, fin) if clock else fin()
    assert res[0]["samples"] == W * rows
    return {"out": np.array([[float(r[k]) for k in ASTROM_KEYS] + r["position_means"]
                             for r in res])}


# ------------------------------------------------------------------------------ photometry
def phot_chain(variant, rows, W):
    """tests/test_gpu_photometry.py's plane_chain recipe at [rows][W]: a few rows unusable (a
    NaN column, A_0 - b <= 0) and one companion at or below the offset."""
    ps = 17 if variant == 2 else 20
    c0, ns = tp.columns(variant)
    rng = np.random.RandomState(60 + variant)
    c = rng.normal(size=(rows, W, ps)) * 3.0 + 50.0
    c[:, :, c0] = 3.0e4 + 500.0 * rng.normal(size=(rows, W))
    for k in range(1, ns):
        c[:, :, c0 + k] = 2.0e3 / k + 60.0 * rng.normal(size=(rows, W))
    c[:, :, c0 + ns] = 0.2 + 0.02 * rng.normal(size=(rows, W))
    c[:, :, c0 + ns + 1] = 30.0 + rng.normal(size=(rows, W))
    for i, s0 in enumerate((1.5, 1.5, 4.5, 4.5)):
        c[:, :, c0 + ns + 2 + i] = s0 + 0.2 * rng.normal(size=(rows, W))
    b = c0 + ns + 1
    c[0, :, c0 + ns] = np.nan                               # a NaN column: a whole row of walkers
    c[5, 1, c0] = c[5, 1, b] - 1.0                          # A_0 - b < 0
    c[40, 69, c0] = c[40, 69, b]                            # A_0 - b = 0, in the ragged tile
    c[6, 0, c0 + 1] = c[6, 0, b] - 2.0                      # d_1 < 0: ratio kept, dmag NaN
    return c


def phot_out(res, names):
    return np.array([[float(res[n][k]) for k in PHOT_KEYS]
                     + [v for br in res[n]["brackets"] for v in br] for n in names])


def phot(variant):
    chain = phot_chain(variant, 61, 70)
    with Photometry(70, 61, variant=variant, pixscale=tp.PIXSCALE) as p:
        p.fold_rows(chain)
        res = p.finalize(tp.PROBS)
        bad = p.unusable
    assert bad == 72 and res[p.planes[1]]["n"] == 70 * 61 - 73        # dmag of companion 1
    return {"out": phot_out(res, p.planes), "unusable": np.array([bad])}


def phot_partials257():
    n, W = fc.PHOT["partials257"]
    chain = tp.ratio_chain(tp.scale_values(n), W)
    with Photometry(W, chain.shape[0], pixscale=tp.PIXSCALE) as p:
        p.fold_rows(chain)
        res = clocked("phot partials257", lambda: p.finalize(tp.PROBS))
    return {"out": phot_out(res, ("flux_ratio", "core_fraction"))}


# ------------------------------------------------------------ covariance, autocorrelation
def cov(W, N):
    """Per-walker form with between, 17 columns, one row non-finite."""
    rng = np.random.RandomState(1000 * W + N)
    rows = rng.normal(size=(W, N, 17)) * np.linspace(0.1, 3.0, 17) + np.arange(17.0)
    rows[W // 2, N // 2, 5] = np.inf
    with Covariance(17, walkers=W) as c:
        c.fold_rows(rows)
        st, bt = c.state(), c.between()
    assert st["skipped"] == 1 and st["n"] == W * N - 1
    out = {k: np.asarray(st[k]) for k in ("n", "skipped", "S1", "S2", "S1w", "nw")}
    out.update({k: np.asarray(bt[k]) for k in ("B", "m", "nw_min", "nw_max")})
    return {k: np.atleast_1d(v) for k, v in out.items()}


def acf():
    """300 series x 130 rows, 3 columns, max_lag 64, one series unusable."""
    rng = np.random.RandomState(300130)
    rows = np.cumsum(rng.normal(size=(300, 130, 3)), axis=1) * 0.1 + rng.normal(size=(300, 130, 3))
    rows[271, 64, 1] = np.nan
    with Autocorr(3, 64) as a:
        a.fold_rows(rows)
        st = a.state()
    assert (st["skipped"], st["series"], st["n"]) == (1, 299, 299 * 130)
    return {"C": st["C"], "counters": np.array([st["n"], st["series"], st["skipped"]])}


# --------------------------------------------------------------------------------- moments
def moments():
    """olpe_moments_summary over 300 walkers (two stage-1 blocks of 256, the second ragged)
    after two small launches, with a centre and without."""
    rows = mr.chain_rows(300, 12, 17, seed=23)
    s = tm.make_sampler(2, 300)
    tm.fold(s, rows, (3, 9))
    out = {"centre": s.moments_summary(rows[0, 0].copy()), "bare": s.moments_summary()}
    assert out["centre"].shape == (s.moments_len,)
    s.close()
    return out


CASES = {
    "astrom-v2-300x15": lambda: astrom(300, 15, 2, 51),
    "astrom-v3-300x15": lambda: astrom(300, 15, 3, 52),
    "astrom-v2-1025x1024": lambda: astrom(*fc.ASTROM["1025x1024"][:2], 2, 53,
                                          clock="astrom 1025x1024"),
    "astrom-v2-3x3": lambda: astrom(3, 3, 2, 54),
    "phot-v2-70x61": lambda: phot(2),
    "phot-v3-70x61": lambda: phot(3),
    "phot-v2-partials257": phot_partials257,
    "cov-5x300": lambda: cov(5, 300),
    "cov-300x3": lambda: cov(300, 3),
    "acf-300x130": acf,
    "moments-300": moments,
}


def differing(got, want):
    """The names of a case's arrays that differ from the recording in any bit."""
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    return [k for k in got if not np.array_equal(words(got[k]), words(want[k]))]


@pytest.mark.parametrize("case", list(CASES))
def test_summaries_equal_the_recording(lib_loaded, golden, case):
    rec = golden(GOLDEN)
    want = {k.split("/", 1)[1]: v for k, v in rec.items() if k.startswith(case + "/")}
    assert want, f"{case} is not in tests/golden/{GOLDEN}.npz"
    got = CASES[case]()
    assert differing(got, want) == []
