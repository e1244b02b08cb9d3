"""The autocorrelation estimator of include/olpe.h (olpe_acf_*) restated in NumPy, every sum
in np.longdouble: the reference of test_acf_cpu.py and test_gpu_acf.py.

A series is one walker's values of one column over one contiguous run of rows x[0 .. N-1];
p = x[0]; y[t] = (x[t] - p) - mean_t(x[t] - p).  Per column c and lag k = 0 .. L,

    C[c][k] = sum over series  sum_{t=0}^{N-k-1} y[t] y[t+k]

(biased, no 1 / (N - k) factor, pooled over the series; a lag k >= N adds exactly 0).  A
series with a non-finite value in any column is left out whole and counted in ``skipped``;
``n`` = usable series x N, ``series`` = usable series.  Then f[k] = C[k] / C[0],
tau(M) = 2 sum_{k<=M} f[k] - 1, and the window is the smallest M with M >= c tau(M).
"""
import numpy as np

LD = np.longdouble


def lag_sums(rows, max_lag, time_major=False):
    """rows [W][N][C] (or [N][W][C] with time_major) -> {"C" [C][L + 1] longdouble, "n",
    "series", "skipped"}."""
    x = np.asarray(rows, dtype=np.float64)
    if time_major:
        x = np.swapaxes(x, 0, 1)
    W, N, ncols = x.shape
    ok = np.isfinite(x).all(axis=(1, 2))
    x = x[ok].astype(LD)
    d = x - x[:, :1, :]
    y = d - d.sum(axis=1, keepdims=True, dtype=LD) / LD(N)
    Cm = np.zeros((ncols, max_lag + 1), dtype=LD)
    for k in range(min(max_lag, N - 1) + 1):
        Cm[:, k] = (y[:, :N - k, :] * y[:, k:, :]).sum(axis=(0, 1), dtype=LD)
    used = int(ok.sum())
    return {"C": Cm, "n": used * N, "series": used, "skipped": int(W - used)}


def integrated_time(C, n, series, c=5.0, tol=50.0):
    """One column's (tau, window, windowed, reliable, ess) from its lag sums C[0 .. L], in
    longdouble; tau(L), a lower bound, with windowed False when no M <= L qualifies."""
    C = np.asarray(C, dtype=LD)
    L = C.size - 1
    f = C / C[0]
    taus = LD(2) * np.cumsum(f) - LD(1)
    ok = np.arange(L + 1) >= LD(c) * taus
    windowed = bool(ok.any())
    m = int(np.argmax(ok)) if windowed else L
    tau = taus[m]
    reliable = windowed and LD(n) / LD(series) >= LD(tol) * tau
    return float(tau), m, windowed, bool(reliable), float(LD(n) / tau)


def ar1(phi, W, N, seed):
    """W x N x len(phi) stationary AR(1) series of unit innovations, column c with
    coefficient phi[c], from np.random.RandomState(seed)."""
    phi = np.atleast_1d(np.asarray(phi, dtype=np.float64))
    rng = np.random.RandomState(seed)
    e = rng.normal(size=(N, W, phi.size))
    z = np.empty((N, W, phi.size))
    z[0] = e[0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, N):
        z[t] = phi * z[t - 1] + e[t]
    return np.ascontiguousarray(np.swapaxes(z, 0, 1))


def chain_like(W, N, ncols, seed):
    """The GPU tests' data: AR(1) with phi spread over 0 .. 0.97 by column, as a chain whose
    scatter is small beside its value, 512.3 + 1e-2 z; [W][N][ncols]."""
    phi = np.linspace(0.0, 0.97, ncols)
    return 512.3 + 1e-2 * ar1(phi, W, N, seed)
