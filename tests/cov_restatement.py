"""The cross-column sums of include/olpe.h (olpe_cov_*) restated in NumPy, every sum in
np.longdouble: the reference of test_covariance_cpu.py and test_gpu_covariance.py.

About a pivot p, with d = x - p per row: S1[j] = sum d_j, S2[j][k] = sum d_j d_k, per walker
w its row count nw[w], S1w[w][j] and (for the bounds) its own sum of squares S2w[w][j]; the
between-walker term sum_w S1w S1w^T / nw over the walkers with rows.  A row with a non-finite
value in any column is left out whole and counted in ``skipped``.  With no pivot given it is
the first row (walker 0, row 0), a non-finite entry replaced by 0.0.
"""
import numpy as np

LD = np.longdouble


def sums(rows, pivot=None, time_major=False):
    """rows [W][N][C] (or [N][W][C] with time_major) -> dict of longdouble sums."""
    x = np.asarray(rows, dtype=np.float64)
    if time_major:
        x = np.swapaxes(x, 0, 1)
    W, N, ncols = x.shape
    if pivot is None:
        p = np.where(np.isfinite(x[0, 0]), x[0, 0], 0.0)
    else:
        p = np.asarray(pivot, dtype=np.float64)
    ok = np.isfinite(x).all(axis=2)
    d = np.where(ok[:, :, None], x, p).astype(LD) - p.astype(LD)
    S1w = d.sum(axis=1, dtype=LD)
    S2w = (d * d).sum(axis=1, dtype=LD)
    S2 = np.zeros((ncols, ncols), dtype=LD)
    for j in range(ncols):
        S2[j] = (d[:, :, j:j + 1] * d).sum(axis=(0, 1), dtype=LD)
    nw = ok.sum(axis=1).astype(np.uint64)
    on = nw > 0
    B = np.zeros((ncols, ncols), dtype=LD)
    for w in np.flatnonzero(on):
        B += np.outer(S1w[w], S1w[w]) / LD(int(nw[w]))
    return {"pivot": p, "n": int(nw.sum()), "skipped": int(W * N - nw.sum()),
            "S1": S1w.sum(axis=0, dtype=LD), "S2": S2, "nw": nw, "S1w": S1w, "S2w": S2w,
            "between": B, "m": int(on.sum()),
            "nw_min": int(nw[on].min()) if on.any() else 0,
            "nw_max": int(nw[on].max()) if on.any() else 0}


def cov(rows):
    """np.cov of the rows [W][N][C] pooled, in longdouble (ddof 1)."""
    x = np.asarray(rows, dtype=np.float64).reshape(-1, np.shape(rows)[-1]).astype(LD)
    xm = x - x.sum(axis=0, dtype=LD) / LD(x.shape[0])
    out = np.zeros((x.shape[1], x.shape[1]), dtype=LD)
    for j in range(x.shape[1]):
        out[j] = (xm[:, j:j + 1] * xm).sum(axis=0, dtype=LD)
    return out / LD(x.shape[0] - 1)


def mpsrf(rows, cols=None):
    """Brooks & Gelman's multivariate R-hat and the per-column values of m walkers of n rows,
    rows [m][n][C], straight from the definition: W the mean of the walkers' covariance
    matrices (divisor n - 1), B / n the covariance of the walker means (divisor m - 1), the
    moments in longdouble, the eigenvalues of W^-1 B / n in double.  Returns (Rp, rhat[C])."""
    x = np.asarray(rows, dtype=np.float64).astype(LD)
    if cols is not None:
        x = x[:, :, list(cols)]
    m, n, ncols = x.shape
    mu_w = x.sum(axis=1, dtype=LD) / LD(n)
    dev = x - mu_w[:, None, :]
    Wm = np.zeros((ncols, ncols), dtype=LD)
    for j in range(ncols):
        Wm[j] = (dev[:, :, j:j + 1] * dev).sum(axis=(0, 1), dtype=LD)
    Wm /= LD(m * (n - 1))
    dm = mu_w - mu_w.sum(axis=0, dtype=LD) / LD(m)
    Bn = (dm[:, :, None] * dm[:, None, :]).sum(axis=0, dtype=LD) / LD(m - 1)
    lam = np.linalg.eigvals(np.linalg.solve(Wm.astype(np.float64), Bn.astype(np.float64)))
    f0, f1 = (n - 1.0) / n, (m + 1.0) / m
    rhat = f0 + f1 * (np.diag(Bn) / np.diag(Wm)).astype(np.float64)
    return f0 + f1 * float(lam.real.max()), rhat
