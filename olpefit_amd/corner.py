"""The data behind the reference's corner plot, counted on the device (include/olpe.h,
olpe_corner_*).

The reference ends (apf_step3.py:603-643; 3body/apf_step3_3body.py likewise) by flattening
every parameter chain into ``corner.corner(..., show_titles=True, plot_contours=True)``: a
1-D histogram per parameter, a 2-D histogram per pair and each title's 16 / 50 / 84 %
quantiles.  ``Corner`` keeps both sets of integer counts on the GPU, streams a sampler's
launches (or host rows) into them, and reads quantile brackets off the fine 1-D counts.
Counts merge by addition (``add``), so ranks, contexts and checkpoints combine on the host.

Not covered: the drawing, contour levels and exact quantiles (they need a sample store).
Nothing here imports matplotlib, corner or the oracle.
"""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import numpy as np

from . import _lib
from ._handle import Handle, _pd, _u64, load_npz  # noqa: F401  (load_npz: Corner.save's reader)
from ._lib import check

MAX_COLS, MAX_BINS, MAX_FINE_BINS = 24, 64, 4096
#: the reference's labels (apf_step3.py:586-587; 3body/apf_step3_3body.py:661-662)
LABELS_2 = ["xcs", "ycs", "xcc", "ycc", "dx", "dy", "amps", "ampc", "ampratio", "bkgd",
            "sigmax", "sigmay", "sigmax2", "sigmay2", "theta", "theta2", "chisquared"]
LABELS_3 = ["xca", "yca", "xcb", "ycb", "xcc", "ycc", "dx", "dy", "ampa", "ampb", "ampc",
            "ampratio", "bkgd", "sigmax", "sigmay", "sigmax2", "sigmay2", "theta", "theta2",
            "chisquared"]


def pairs_of(ncols: int):
    """The pairs (i, j), i < j, in the order of ``h2``'s first axis."""
    return [(i, j) for i in range(ncols) for j in range(i + 1, ncols)]


def quantile_table(edges, h1, n, q=(0.16, 0.5, 0.84)):
    """Quantile brackets from 1-D counts (host arithmetic only).

    ``edges`` [C][nb + 1], ``h1`` [C][nb], ``n`` samples folded.  Returns a dict with
    ``q``, ``lo`` / ``hi`` / ``estimate`` [C][len(q)] and ``notes`` [C].

    For a column whose samples all fell in a bin, ``[lo, hi]`` contains
    ``np.percentile(col, 100 q)`` (linear interpolation): with v = q (N - 1), that value
    lies between the order statistics floor(v) and ceil(v), and the bracket is the union
    of the bins that hold those two.  Where v is an integer the two coincide; where the
    float product lands within rounding of an integer m (NumPy's own product may fall on
    either side), the statistics m - 1 .. m + 1 are taken.  ``estimate`` interpolates
    linearly inside the bins and lies in the bracket.  A column with samples outside its
    edges (or none at all) gives NaN, and ``notes`` says why: the rank of a sample that
    was not counted is unknown."""
    edges = np.asarray(edges, dtype=np.float64)
    h1 = np.asarray(h1, dtype=np.uint64)
    q = [float(x) for x in q]
    if any(not 0.0 <= x <= 1.0 for x in q):
        raise ValueError("quantiles must lie in [0, 1]")
    ncols = h1.shape[0]
    lo = np.full((ncols, len(q)), np.nan)
    hi = np.full((ncols, len(q)), np.nan)
    est = np.full((ncols, len(q)), np.nan)
    notes = []
    n = int(n)
    for c in range(ncols):
        counts = [int(v) for v in h1[c]]          # Python ints: exact beyond 2^53
        inside = sum(counts)
        if n == 0:
            notes.append("no samples folded")
            continue
        if inside != n:
            notes.append(f"{n - inside} of {n} samples outside the edges "
                         f"[{edges[c][0]:.17g}, {edges[c][-1]:.17g}]: ranks unknown")
            continue
        notes.append("")
        cum = np.cumsum(np.asarray(counts, dtype=object))   # cum[b] = samples in bins <= b

        def bin_of(k):                            # the bin of order statistic k (0-based)
            a, b = 0, len(counts) - 1
            while a < b:
                m = (a + b) // 2
                if cum[m] > k:
                    b = m
                else:
                    a = m + 1
            return a

        def value(k):                             # within-bin linear position of statistic k
            b = bin_of(k)
            before = int(cum[b]) - counts[b]
            return edges[c][b] + (k - before + 0.5) / counts[b] * (edges[c][b + 1] - edges[c][b])

        for iq, x in enumerate(q):
            v = x * (n - 1)
            m = int(round(v))
            if Fraction(x) * (n - 1) == m:
                k0 = k1 = m
                f0, g = m, 0.0
            else:
                if abs(v - m) <= 1e-9 * max(1.0, float(n)):
                    k0, k1 = m - 1, m + 1
                else:
                    k0 = int(math.floor(v))
                    k1 = k0 + 1
                f0 = int(math.floor(v))
                g = v - f0
            k0, k1 = max(0, k0), min(n - 1, k1)
            f0 = min(max(0, f0), n - 1)
            b0, b1 = bin_of(k0), bin_of(k1)
            lo[c, iq], hi[c, iq] = edges[c][b0], edges[c][b1 + 1]
            e = (1.0 - g) * value(f0) + g * value(min(f0 + 1, n - 1))
            est[c, iq] = min(max(e, lo[c, iq]), hi[c, iq])
    return {"q": q, "lo": lo, "hi": hi, "estimate": est, "notes": notes}


class Corner(Handle):
    """One ``olpe_corner``: the corner plot's 1-D and 2-D counts of [..., ncols] rows on
    one GPU.  ``ranges`` [ncols][2] = (lo, hi) per column; both edge sets are
    ``np.linspace(lo, hi, n + 1)`` (``bins`` per axis of the 2-D histograms, corner's
    default 20; ``fine_bins`` for the 1-D ones the quantiles are read from)."""

    _destroy = "olpe_corner_destroy"

    def __init__(self, ranges, *, bins: int = 20, fine_bins: int = 2048, labels=None,
                 device: int = 0, edges=None, fine_edges=None):
        if edges is None or fine_edges is None:
            r = np.asarray(ranges, dtype=np.float64)
            if r.ndim != 2 or r.shape[1] != 2:
                raise ValueError("ranges must be [ncols][2]")
            edges = np.stack([np.linspace(lo, hi, int(bins) + 1) for lo, hi in r])
            fine_edges = np.stack([np.linspace(lo, hi, int(fine_bins) + 1) for lo, hi in r])
        self.edges = np.ascontiguousarray(edges, dtype=np.float64)
        self.fine_edges = np.ascontiguousarray(fine_edges, dtype=np.float64)
        if (self.edges.ndim != 2 or self.fine_edges.ndim != 2
                or self.edges.shape[0] != self.fine_edges.shape[0]):
            raise ValueError("edges must be [ncols][bins + 1] and [ncols][fine_bins + 1]")
        self.ncols = int(self.edges.shape[0])
        self.bins = int(self.edges.shape[1]) - 1
        self.fine_bins = int(self.fine_edges.shape[1]) - 1
        self.npairs = self.ncols * (self.ncols - 1) // 2
        self.labels = ([f"c{i}" for i in range(self.ncols)] if labels is None
                       else [str(s) for s in labels])
        if len(self.labels) != self.ncols:
            raise ValueError(f"{len(self.labels)} labels for {self.ncols} columns")
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.olpe_corner_create(int(device), self.ncols, _pd(self.fine_edges),
                                            self.fine_bins, _pd(self.edges), self.bins,
                                            C.byref(h)))
        self._h = h

    # -- ranges -------------------------------------------------------------------
    @staticmethod
    def ranges_of(rows):
        """Per-column (min, max) of the finite values of [..., ncols] rows: corner's
        default range.  A constant column gets +-0.5 (as np.histogram widens it)."""
        r = np.asarray(rows, dtype=np.float64)
        r = r.reshape(-1, r.shape[-1])
        out = np.empty((r.shape[1], 2))
        for c in range(r.shape[1]):
            x = r[:, c]
            x = x[np.isfinite(x)]
            if x.size == 0:
                raise ValueError(f"column {c} has no finite value")
            lo, hi = float(x.min()), float(x.max())
            if lo == hi:
                lo, hi = lo - 0.5, hi + 0.5
            out[c] = lo, hi
        return out

    @staticmethod
    def ranges_from_summary(mean, sigma, k: float = 5.0):
        """mean +- k sigma per column, for streaming from a sampler whose rows never reach
        the host (``Sampler.moments_summary``).  Samples beyond are dropped and show up in
        the outside counts."""
        mean = np.asarray(mean, dtype=np.float64).ravel()
        half = float(k) * np.abs(np.asarray(sigma, dtype=np.float64).ravel())
        half = np.where(half > 0, half, 0.5)
        return np.stack([mean - half, mean + half], axis=1)

    # -- folding ------------------------------------------------------------------
    def fold(self, sampler):
        """Fold the rows of the sampler's last launch from its device chain (once per
        launch; async on the sampler's stream, no host copy)."""
        check(self._lib.olpe_corner_fold_ctx(self._h, sampler._ctx))

    def fold_rows(self, rows):
        """Fold host rows [..., ncols] (a caller may have appended columns of its own,
        separation and position angle for instance, up to 24 in all)."""
        r = np.ascontiguousarray(rows, dtype=np.float64)
        if r.ndim < 1 or r.shape[-1] != self.ncols:
            raise ValueError(f"rows of shape {r.shape}, expected [..., {self.ncols}]")
        n = r.size // self.ncols
        check(self._lib.olpe_corner_fold_rows(self._h, _pd(r), n))

    def counts(self):
        """``{"n", "h1" [C][fine_bins], "h2" [npairs][bins][bins], "outside1" [C],
        "outside2" [npairs]}`` (uint64): a sample outside a column's edges, NaN or +-inf is
        in none of that column's bins."""
        n = C.c_ulonglong(0)
        h1 = np.zeros((self.ncols, self.fine_bins), dtype=np.uint64)
        h2 = np.zeros((self.npairs, self.bins, self.bins), dtype=np.uint64)
        check(self._lib.olpe_corner_get(self._h, C.byref(n), _u64(h1), _u64(h2)))
        nn = np.uint64(n.value)
        return {"n": int(n.value), "h1": h1, "h2": h2,
                "outside1": nn - h1.sum(axis=1, dtype=np.uint64),
                "outside2": nn - h2.sum(axis=(1, 2), dtype=np.uint64)}

    def add(self, counts):
        """Merge another object's, rank's or checkpoint's ``counts()`` (same edges)."""
        h1 = np.ascontiguousarray(counts["h1"], dtype=np.uint64)
        h2 = np.ascontiguousarray(counts["h2"], dtype=np.uint64)
        if h1.shape != (self.ncols, self.fine_bins) or h2.shape != (self.npairs, self.bins,
                                                                    self.bins):
            raise ValueError(f"counts of shapes {h1.shape}, {h2.shape} do not match this object")
        check(self._lib.olpe_corner_add(self._h, int(counts["n"]), _u64(h1), _u64(h2)))

    def reset(self):
        check(self._lib.olpe_corner_reset(self._h))

    # -- results ------------------------------------------------------------------
    quantile_table = staticmethod(quantile_table)

    def quantiles(self, q=(0.16, 0.5, 0.84), counts=None):
        """``quantile_table`` of the fine 1-D counts."""
        c = self.counts() if counts is None else counts
        return quantile_table(self.fine_edges, c["h1"], c["n"], q)

    def save(self, path, q=(0.16, 0.5, 0.84)):
        """One ``.npz`` with everything a plotting script needs: labels, both edge sets,
        ``h1``, ``h2``, ``n``, the outside counts and the quantile table."""
        c = self.counts()
        t = self.quantiles(q, c)
        save_npz(path, self.labels, self.edges, self.fine_edges, c, t)
        return c, t


def save_npz(path, labels, edges, fine_edges, counts, table):
    with open(path, "wb") as f:
        np.savez(f, labels=np.asarray(labels, dtype="U"), edges=edges, fine_edges=fine_edges,
                 h1=counts["h1"], h2=counts["h2"], n=np.uint64(counts["n"]),
                 outside1=counts["outside1"], outside2=counts["outside2"],
                 pairs=np.asarray(pairs_of(len(labels)), dtype=np.int32),
                 q=np.asarray(table["q"]), q_lo=table["lo"], q_hi=table["hi"],
                 q_estimate=table["estimate"], q_notes=np.asarray(table["notes"], dtype="U"))
