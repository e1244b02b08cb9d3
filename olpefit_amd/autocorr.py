"""Integrated autocorrelation times and effective sample sizes of the chains, summed on the
device (include/olpe.h, olpe_acf_*).

The reference judges its chains by eye: apf_step3.py:582-601 draws every walker's trace of
every parameter, and ``additional_burnin``, ``accept_min`` and the record stride are chosen
from the picture.  ``Autocorr`` is the quantitative counterpart, in emcee's
``get_autocorr_time`` form: per column the pooled lag sums

    C[k] = sum over series  sum_{t=0}^{N-k-1} y[t] y[t+k],   k = 0 .. max_lag,

of the series' deviations y (a series is one walker's values of one column over one
contiguous run of recorded rows; y[t] = (x[t] - x[0]) - mean_t(x[t] - x[0])), folded on the
GPU from a sampler's device chain or from host rows.  The state is additive (``state`` /
``add``), so launches, ranks and checkpoints merge on the host, and everything after the
sums is host arithmetic: ``integrated_time`` needs no GPU.

Not covered: lags across launch boundaries in ``fold(sampler)`` (each launch's rows of a
walker are a series of their own), per-walker tau, an FFT form, a collective over the state.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._handle import Handle, _pd, _u64, load_npz  # noqa: F401  (load_npz: Autocorr.save's reader)
from ._lib import check

MAX_COLS, MIN_LAG, MAX_LAG = 24, 64, 1024


def integrated_time(C, n, series, c: float = 5.0, tol: float = 50.0):
    """tau and the effective sample size per column from the lag sums (plain NumPy).

    ``C`` [ncols][L + 1] (or [L + 1]), ``n`` values per column, ``series`` series folded.
    With f[k] = C[k] / C[0] and tau(M) = 2 sum_{k<=M} f[k] - 1, the window is the smallest
    M with M >= c tau(M) (emcee's automatic windowing, c = 5 its default).  Returns a dict of
    per-column arrays:

    * ``tau`` (recorded rows), ``window``, ``windowed`` -- False if no M <= L qualifies; tau
      is then tau(L), a lower bound, and ``window`` is L;
    * ``reliable`` -- windowed and the mean series length n / series >= tol tau (emcee's
      ``tol``);
    * ``ess`` = n / tau, ``suggested_stride`` = ceil(tau) recorded rows (at least 1; 0 where
      tau is NaN), ``f`` [ncols][L + 1];
    * ``notes`` -- "constant column" where C[0] == 0 (tau NaN), "no samples", "max_lag too
      small", or "";
    * ``min_ess`` -- the smallest finite ess (NaN if there is none).
    """
    Cm = np.atleast_2d(np.asarray(C, dtype=np.float64))
    ncols, L = Cm.shape[0], Cm.shape[1] - 1
    n, series = int(n), int(series)
    tau = np.full(ncols, np.nan)
    window = np.zeros(ncols, dtype=np.int64)
    windowed = np.zeros(ncols, dtype=bool)
    reliable = np.zeros(ncols, dtype=bool)
    f = np.full((ncols, L + 1), np.nan)
    notes = []
    lags = np.arange(L + 1)
    for k in range(ncols):
        if n == 0 or series == 0:
            notes.append("no samples")
            continue
        if not Cm[k, 0] > 0.0:                      # 0 (or a NaN merged in): no scatter
            notes.append("constant column")
            continue
        f[k] = Cm[k] / Cm[k, 0]
        taus = 2.0 * np.cumsum(f[k]) - 1.0
        ok = lags >= c * taus
        if ok.any():
            m = int(np.argmax(ok))
            windowed[k] = True
            notes.append("")
        else:
            m = L
            notes.append("max_lag too small")
        window[k] = m
        tau[k] = taus[m]
        reliable[k] = bool(windowed[k] and n / series >= tol * tau[k])
    with np.errstate(all="ignore"):
        ess = n / tau
        stride = np.where(np.isfinite(tau), np.ceil(np.maximum(tau, 1.0)), 0).astype(np.int64)
    fin = ess[np.isfinite(ess)]
    return {"tau": tau, "window": window, "windowed": windowed, "reliable": reliable,
            "ess": ess, "suggested_stride": stride, "f": f, "notes": notes,
            "min_ess": float(fin.min()) if fin.size else float("nan"),
            "n": n, "series": series, "c": float(c), "tol": float(tol)}


class Autocorr(Handle):
    """One ``olpe_acf``: the pooled lag sums of [..., ncols] chains on one GPU.
    ``max_lag`` is a multiple of 64 from 64 to 1024; 1 <= ncols <= 24."""

    _destroy = "olpe_acf_destroy"

    def __init__(self, ncols: int, max_lag: int = 512, labels=None, device: int = 0):
        self.ncols, self.max_lag = int(ncols), int(max_lag)
        self.labels = ([f"c{i}" for i in range(self.ncols)] if labels is None
                       else [str(s) for s in labels])
        if len(self.labels) != self.ncols:
            raise ValueError(f"{len(self.labels)} labels for {self.ncols} columns")
        #: iterations per recorded row of the sampler launches folded (None: host rows, or
        #: launches of different strides)
        self.record_stride = None
        self._strides = set()
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.olpe_acf_create(int(device), self.ncols, self.max_lag, C.byref(h)))
        self._h = h

    # -- folding ------------------------------------------------------------------
    def _stride_seen(self, s):
        self._strides.add(s)
        only = next(iter(self._strides)) if len(self._strides) == 1 else None
        self.record_stride = only if only else None

    def fold(self, sampler):
        """Fold the sampler's last launch from its device chain: each walker's recorded rows
        of that launch are one series (once per launch; async on the sampler's stream, no
        host copy)."""
        check(self._lib.olpe_acf_fold_ctx(self._h, sampler._ctx))
        self._stride_seen(int(getattr(sampler, "_record_stride", 0) or 0))

    def fold_rows(self, rows, time_major: bool = False):
        """Fold host rows: [walkers][rows][ncols], or with ``time_major`` [rows][walkers]
        [ncols] as step 3's chains lie.  Each walker's rows are one series.  No transposition
        on the host."""
        r = np.ascontiguousarray(rows, dtype=np.float64)
        if r.ndim != 3 or r.shape[2] != self.ncols:
            raise ValueError(f"rows of shape {r.shape}, expected [walkers][rows][{self.ncols}] "
                             f"(or [rows][walkers][{self.ncols}] with time_major)")
        nw, nr = (r.shape[1], r.shape[0]) if time_major else (r.shape[0], r.shape[1])
        check(self._lib.olpe_acf_fold_rows(self._h, _pd(r), nw, nr,
                                           int(bool(time_major))))
        self._stride_seen(0)

    def state(self):
        """``{"ncols", "max_lag", "n", "series", "skipped", "C" [ncols][max_lag + 1]}``."""
        n, ser, sk = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
        Cm = np.zeros((self.ncols, self.max_lag + 1))
        check(self._lib.olpe_acf_get(self._h, C.byref(n), C.byref(ser), C.byref(sk),
                                     _pd(Cm)))
        return {"ncols": self.ncols, "max_lag": self.max_lag, "n": int(n.value),
                "series": int(ser.value), "skipped": int(sk.value), "C": Cm}

    def add(self, state):
        """Merge another object's, rank's or checkpoint's ``state()`` (the same ncols and
        max_lag; anything else is refused)."""
        Cm = np.ascontiguousarray(state["C"], dtype=np.float64)
        if Cm.ndim != 2:
            raise ValueError(f"C of shape {Cm.shape}")
        check(self._lib.olpe_acf_add(self._h, int(Cm.shape[0]), int(Cm.shape[1]) - 1,
                                     int(state["n"]), int(state["series"]),
                                     int(state["skipped"]), _pd(Cm)))

    def reset(self):
        check(self._lib.olpe_acf_reset(self._h))
        self._strides.clear()
        self.record_stride = None

    # -- results ------------------------------------------------------------------
    def result(self, c: float = 5.0, tol: float = 50.0, state=None):
        """``integrated_time`` of the state, with ``labels``, ``skipped`` and, when every
        fold came from sampler launches of one record stride, ``record_stride`` and
        ``tau_iterations`` = tau x stride."""
        st = self.state() if state is None else state
        res = integrated_time(st["C"], st["n"], st["series"], c, tol)
        res["labels"] = list(self.labels)
        res["skipped"] = st["skipped"]
        res["max_lag"] = self.max_lag
        res["record_stride"] = self.record_stride
        res["tau_iterations"] = (res["tau"] * self.record_stride if self.record_stride
                                 else None)
        return res

    def save(self, path, c: float = 5.0, tol: float = 50.0):
        """One ``.npz`` with the state and the table; returns ``(state, result)``."""
        st = self.state()
        res = self.result(c, tol, st)
        save_npz(path, st, res)
        return st, res


def save_npz(path, state, res):
    with open(path, "wb") as f:
        np.savez(f, labels=np.asarray(res["labels"], dtype="U"), max_lag=np.int64(res["max_lag"]),
                 C=state["C"], n=np.uint64(state["n"]), series=np.uint64(state["series"]),
                 skipped=np.uint64(state["skipped"]), tau=res["tau"], window=res["window"],
                 windowed=res["windowed"], reliable=res["reliable"], ess=res["ess"],
                 suggested_stride=res["suggested_stride"], f=res["f"],
                 notes=np.asarray(res["notes"], dtype="U"), c=np.float64(res["c"]),
                 tol=np.float64(res["tol"]), min_ess=np.float64(res["min_ess"]),
                 record_stride=np.int64(res["record_stride"] or 0))


def table_lines(res):
    """One line per label: tau, window, ESS and flags."""
    out = []
    for k, name in enumerate(res["labels"]):
        flags = ("windowed" if res["windowed"][k] else "lower-bound") + (
            " reliable" if res["reliable"][k] else " short")
        note = f" ({res['notes'][k]})" if res["notes"][k] else ""
        out.append(f"{name:>10} tau {res['tau'][k]:.6g} window {int(res['window'][k])} "
                   f"ESS {res['ess'][k]:.6g} {flags}{note}")
    return out
