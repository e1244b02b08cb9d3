"""The definitions of the pointwise-deviance fold (olpe_lik.hip, olpefit_amd/predictive.py)
restated in np.longdouble over the oracle's build_analytical_model and core.noise_model's
err and mask:  x = ((D - M) / err)^2 per unmasked pixel and sample, and from x the planes
and scalars of olpe_lik_finalize.  Also the error bounds the GPU tests hold the device to,
derived in test_gpu_predictive's docstring.  No GPU, nothing of the library.
"""
import numpy as np

from olpefit_amd import core
from oracle import olpe_oracle

LD = np.longdouble
U = 2.0 ** -53


def frame(img):
    """(D, err, mask) of an image as olpe_create stages it (ITIME 1, one coadd, SAMPMODE 2)."""
    mask, pois2, rn2, _, _ = core.noise_model(img, 1.0, 1, 1, 2)
    with np.errstate(invalid="ignore"):
        err = np.sqrt(rn2 + pois2.astype(np.float64))
    return np.asarray(img, dtype=np.float64), err, np.asarray(mask, dtype=bool)


def models(rows, n, nsrc, bkgd_mode=0):
    return np.stack([olpe_oracle.build_analytical_model(r, n, nsrc, bkgd_mode)
                     for r in np.atleast_2d(rows)])


def deviance(M, D, err, mask):
    """(t, x) [S][n][n] in long double; 0 at masked pixels."""
    with np.errstate(all="ignore"):
        t = (D.astype(LD) - M.astype(LD)) / np.where(mask, 1.0, err).astype(LD)
    t = np.where(mask, LD(0), t)
    return t, t * t


def planes(x, mask):
    """The five sample planes of olpe_lik_finalize from x [S][n][n], NaN at masked pixels."""
    S = x.shape[0]
    mean = x.mean(axis=0)
    std = x.std(axis=0)
    m = x.min(axis=0)
    L = np.exp(-(x - m) / 2).sum(axis=0)
    lppd = np.log(L / S) - m / 2
    pw = (-x / 2).var(axis=0, ddof=1) if S > 1 else np.zeros(mean.shape, LD)
    out = {"mean_dev": mean, "std_dev": std, "lppd": lppd, "p_waic": pw, "elpd": lppd - pw}
    return {k: np.where(mask, LD("nan"), v) for k, v in out.items()}


def scalars(pl, ok, nparams, dev_best=None, dev_at=None, err=None):
    """The totals over the pixels `ok` ([n][n] bool)."""
    N = int(ok.sum())
    e = pl["elpd"][ok]
    sc = {"pixels_counted": N, "lppd": pl["lppd"][ok].sum(), "p_waic": pl["p_waic"][ok].sum(),
          "elpd_waic": e.sum(), "waic": -2 * e.sum(),
          "se_elpd": np.sqrt(N * e.var(ddof=1)) if N > 1 else LD("nan"),
          "p_waic_high": int((pl["p_waic"][ok] > 0.4).sum()),
          "mean_deviance": pl["mean_dev"][ok].sum()}
    sc["reduced"] = sc["mean_deviance"] / (N - nparams)
    if dev_best is not None:
        sc["deviance_best"] = dev_best[ok].sum()
    if dev_at is not None:
        sc["deviance_at"] = dev_at[ok].sum()
        sc["p_d"] = sc["mean_deviance"] - sc["deviance_at"]
        sc["dic"] = sc["deviance_at"] + 2 * sc["p_d"]
    if err is not None:
        sc["log_norm"] = (-np.log(err[ok].astype(LD)) - np.log(2 * LD(np.pi)) / 2).sum()
    return sc


def eps(t, M, err, mask):
    """eps_i = max_s (2 |t| dt + dt^2) with dt = delta w_i + 4 u |t|, delta = 1e-13 max|M|:
    how far x may lie from the restatement's when the model is within the project's EXACT
    tolerance; [n][n] (or [S][n][n] with per_sample)."""
    delta = 1e-13 * float(np.abs(M).max())
    w = np.where(mask, 0.0, 1.0 / np.where(mask, 1.0, err))
    with np.errstate(over="ignore", invalid="ignore"):
        at = np.abs(t).astype(np.float64)
        dt = delta * w + 4 * U * at
        return 2 * at * dt + dt * dt


def bounds(t, x, M, err, mask, c):
    """Per-pixel bounds of the planes for S samples about the pivot plane c."""
    S = x.shape[0]
    e = eps(t, M, err, mask).max(axis=0)
    spread = 2 * S * U * np.abs(x - c).max(axis=0).astype(np.float64)
    b_mean = e + spread
    b_std = 2 * e + spread
    sig = x.std(axis=0).astype(np.float64)
    b_pw = (2 * sig * b_std + b_std ** 2) * (S / (S - 1.0) / 4.0) if S > 1 else np.zeros(e.shape)
    b_lppd = e / 2 + (S + 32) * U
    return {"mean_dev": b_mean, "std_dev": b_std, "p_waic": b_pw, "lppd": b_lppd,
            "elpd": b_lppd + b_pw}


def total_bound(b, values, ok):
    """A total's bound: the sum of its pixels' bounds plus N u sum|.|."""
    N = int(ok.sum())
    return float(b[ok].sum() + N * U * np.abs(values[ok]).sum())
