"""Pointwise deviance, WAIC and DIC of the posterior, folded on the device (include/olpe.h,
olpe_lik_*).

The reference's ``chi_squared`` (apf_step2.py:134-148; 3body/apf_step2_3body.py:134-148)
is one number per vector, and its column is only ever plotted; its 2-source and 3-source
fitters are separate scripts with no way to choose between them.  ``Predictive`` evaluates
every folded sample's ``build_analytical_model`` (apf_step2.py:106-124; 3body :106-125) on
the GPU in the EXACT operation order and folds, per pixel, the deviance ``x = ((D - M) /
err)^2``: its posterior mean and scatter, the log pointwise predictive density, the
effective parameter count, and from them WAIC and DIC.  ``compare`` sets two runs on the
same cutout against each other pixel by pixel.

The sampler's target is ``exp(-chi^2 / 2)``, so ``log p(D_i | theta) = -x_i / 2 + k_i`` with
``k_i = -log(err_i) - log(2 pi) / 2``.  The planes leave ``k_i`` out (it cancels in every
comparison on the same data); its sum is the scalar ``log_norm``.

A sample whose model overflows at a pixel is not dropped there the way ``np.ma`` would drop
it: the pixel's sums become non-finite, its planes are NaN, it is left out of every total and
counted in ``poisoned``.

The state is four images and a few numbers.  It merges (``add``) whenever the pivots are
equal, so ranks, contexts and checkpoints combine on the host; ``planes_from_state`` finishes
a merged state anywhere, in NumPy.

Not covered: PSIS-LOO, a factorised (FAST) fold, a collective over the state, priors (the
reference has none: the posterior is the likelihood), plots, comparisons across different
cutouts or masks.  Nothing here imports matplotlib or the oracle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, fitsio
from ._handle import Handle, _pd, load_npz
from ._lib import check

PLANES = ("mean_dev", "std_dev", "lppd", "p_waic", "elpd", "dev_best", "dev_at")
SCALARS = ("samples", "n_bad", "pixels", "poisoned", "lppd", "p_waic", "elpd_waic", "waic",
           "se_elpd", "p_waic_high", "mean_deviance", "reduced", "deviance_best",
           "deviance_at", "p_d", "dic", "log_norm")
_INTS = ("samples", "n_bad", "pixels", "poisoned", "p_waic_high")
P_WAIC_HIGH = 0.4        # a pixel's p_waic above this: WAIC is unreliable there


def merge_lse(ma, La, mb, Lb):
    """Two running log-sum-exp pairs (m = min x, L = sum exp(-(x - m) / 2); empty: (+inf, 0))
    into one, elementwise: m' = min(m_a, m_b), L' = L_a exp(-(m_a - m') / 2) + L_b
    exp(-(m_b - m') / 2).  The side that holds the minimum keeps the factor 1 exactly; an
    empty side is skipped.  olpe_lik_add's rule, with NumPy's exp."""
    ma, La, mb, Lb = (np.asarray(v, dtype=np.float64) for v in (ma, La, mb, Lb))
    ea, eb = (ma == np.inf) & (La == 0.0), (mb == np.inf) & (Lb == 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.exp(-np.abs(ma - mb) * 0.5)
        lower = mb < ma
        m = np.where(lower, mb, ma)
        L = np.where(lower, La * f + Lb, La + Lb * f)
    m = np.where(eb, ma, np.where(ea, mb, m))
    L = np.where(eb, La, np.where(ea, Lb, L))
    return m, L


def planes_from_state(state, c_plane, dev_best=None, dev_at=None, mask=None):
    """olpe_lik_finalize's arithmetic on a ``state()`` dict and the pivot's deviance plane
    ``c_plane`` (``point(state["pivot"])``): ``(planes, scalars)`` by name.  ``dev_best`` /
    ``dev_at``: the planes of the best row and of theta_hat (``point`` of them), NaN planes
    without; ``mask``: True at masked pixels (default: where ``c_plane`` is NaN).  The
    scalars that need the noise (``log_norm``) or the parameter count (``reduced``) are
    left out."""
    n = np.float64(state["n"])
    a1, a2, m, L = (np.asarray(state[k], dtype=np.float64) for k in ("a1", "a2", "m", "l"))
    c = np.asarray(c_plane, dtype=np.float64)
    mask = np.isnan(c) if mask is None else np.asarray(mask, dtype=bool)
    c = np.where(mask, 0.0, c)
    nanp = np.full(a1.shape, np.nan)
    dev_best = nanp if dev_best is None else np.asarray(dev_best, dtype=np.float64)
    dev_at_given = dev_at is not None
    dev_at = nanp if dev_at is None else np.asarray(dev_at, dtype=np.float64)
    with np.errstate(all="ignore"):
        m1 = a1 / n
        mean = c + m1
        vnum = a2 - a1 * m1
        var = vnum / n
        std = np.sqrt(np.maximum(var, 0.0))
        lppd = np.log(L / n) - m * 0.5
        pw = vnum / (n - 1.0) * 0.25 if n > 1 else np.zeros(a1.shape)
        elpd = lppd - pw
        bad = ~(np.isfinite(a1) & np.isfinite(a2) & np.isfinite(m) & np.isfinite(L)
                & np.isfinite(mean) & np.isfinite(vnum))
    out = mask | bad
    planes = {k: np.where(out, np.nan, v) for k, v in
              zip(PLANES, (mean, std, lppd, pw, elpd, dev_best, dev_at))}
    ok = ~out
    N = int(ok.sum())
    e = planes["elpd"][ok]
    sc = {"samples": int(state["n"]), "n_bad": int(state["n_bad"]),
          "pixels": int((~mask).sum()), "poisoned": int((bad & ~mask).sum()),
          "lppd": float(planes["lppd"][ok].sum()), "p_waic": float(planes["p_waic"][ok].sum()),
          "elpd_waic": float(e.sum()), "waic": float(-2.0 * e.sum()),
          "se_elpd": float(np.sqrt(N * e.var(ddof=1))) if N > 1 else float("nan"),
          "p_waic_high": int((planes["p_waic"][ok] > P_WAIC_HIGH).sum()),
          "mean_deviance": float(planes["mean_dev"][ok].sum()),
          "deviance_best": float(planes["dev_best"][ok].sum())}
    if dev_at_given:
        sc["deviance_at"] = float(planes["dev_at"][ok].sum())
        sc["p_d"] = sc["mean_deviance"] - sc["deviance_at"]
        sc["dic"] = sc["deviance_at"] + 2.0 * sc["p_d"]
    else:
        sc["deviance_at"] = sc["p_d"] = sc["dic"] = float("nan")
    return planes, sc


def _as_dict(x):
    return load_npz(x) if isinstance(x, (str, bytes)) or hasattr(x, "__fspath__") else x


def compare(a, b):
    """Two runs on the same cutout, pixel by pixel: ``a`` and ``b`` are files that ``save``
    wrote, or dicts of their contents (``data``, ``mask``, ``elpd``, ``scalar_waic``,
    ``scalar_dic``).  Refuses (ValueError) unless data and mask are equal arrays.  Over the
    pixels that count in both (unmasked, not poisoned in either): ``d_elpd = sum(elpd_a -
    elpd_b)`` (positive: a predicts the image better), ``se = sqrt(N var_i(elpd_a,i -
    elpd_b,i))`` (ddof 1), their ratio, and ``d_waic`` = WAIC_a - WAIC_b = -2 d_elpd and
    ``d_dic`` = DIC_a - DIC_b of the two runs' own scalars."""
    a, b = _as_dict(a), _as_dict(b)
    for k in ("data", "mask"):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or not np.array_equal(x, y, equal_nan=(k == "data")):
            raise ValueError(f"the two runs' {k} arrays differ: pointwise terms of different "
                             f"cutouts or masks do not compare")
    ea, eb = np.asarray(a["elpd"], dtype=np.float64), np.asarray(b["elpd"], dtype=np.float64)
    ok = ~(np.isnan(ea) | np.isnan(eb))
    d = ea[ok] - eb[ok]
    N = int(ok.sum())
    d_elpd = float(d.sum())
    se = float(np.sqrt(N * d.var(ddof=1))) if N > 1 else float("nan")
    with np.errstate(all="ignore"):
        ratio = float(np.float64(d_elpd) / np.float64(se))
    return {"pixels": N, "d_elpd": d_elpd, "se": se, "ratio": ratio,
            "d_waic": float(a["scalar_waic"]) - float(b["scalar_waic"]),
            "d_dic": float(a["scalar_dic"]) - float(b["scalar_dic"])}


def write_npz(path, images, scalars, state, c_plane, data, mask, nsrc, bkgd_mode=0, thin=1):
    """What ``Predictive.save`` writes: the planes by name, ``scalar_<name>``, the state
    (``n``, ``n_bad``, ``pivot``, ``a1``, ``a2``, ``m``, ``l``, ``best``) with the pivot's
    deviance plane ``c``, and data, mask, nsrc, bkgd_mode, thin."""
    with open(path, "wb") as f:
        np.savez(f, data=np.asarray(data, dtype=np.float64), mask=np.asarray(mask, dtype=bool),
                 nsrc=np.int64(nsrc), bkgd_mode=np.int64(bkgd_mode), thin=np.int64(thin),
                 c=np.asarray(c_plane, dtype=np.float64), n=np.int64(state["n"]),
                 n_bad=np.int64(state["n_bad"]),
                 **{k: np.asarray(state[k], dtype=np.float64)
                    for k in ("pivot", "a1", "a2", "m", "l", "best")},
                 **{k: np.asarray(v, dtype=np.float64) for k, v in images.items()},
                 **{"scalar_" + k: np.float64(v) for k, v in scalars.items()})


def state_of(saved):
    """The ``state()`` dict inside a saved file (a path or its dict): ``add`` takes it, and
    ``planes_from_state(state_of(z), z["c"], ...)`` finishes it."""
    z = _as_dict(saved)
    return {"n": int(z["n"]), "n_bad": int(z["n_bad"]),
            **{k: np.array(z[k], dtype=np.float64)
               for k in ("pivot", "a1", "a2", "m", "l", "best")}}


def table_lines(scalars, comparison=None):
    """The lines step 3 prints: the scalars of ``Predictive.scalars`` and, with one,
    ``compare``'s result."""
    s = scalars
    lines = [f"{'samples':>16} {s['samples']}  (unusable rows {s['n_bad']})",
             f"{'pixels':>16} {s['pixels']}  (poisoned {s['poisoned']})",
             f"{'mean deviance':>16} {s['mean_deviance']:.10g}  reduced {s['reduced']:.6g}",
             f"{'deviance best':>16} {s['deviance_best']:.10g}",
             f"{'lppd':>16} {s['lppd']:.10g}",
             f"{'p_waic':>16} {s['p_waic']:.6g}  ({s['p_waic_high']} pixels above "
             f"{P_WAIC_HIGH:g})",
             f"{'elpd_waic':>16} {s['elpd_waic']:.10g} +- {s['se_elpd']:.6g}",
             f"{'WAIC':>16} {s['waic']:.10g}",
             f"{'D(theta_hat)':>16} {s['deviance_at']:.10g}  p_D {s['p_d']:.6g}",
             f"{'DIC':>16} {s['dic']:.10g}",
             f"{'log_norm':>16} {s['log_norm']:.10g}"]
    if comparison is not None:
        c = comparison
        lines += [f"{'against':>16} {c.get('file', 'the other run')}  ({c['pixels']} pixels)",
                  f"{'d_elpd':>16} {c['d_elpd']:.10g} +- {c['se']:.6g}  (ratio {c['ratio']:.4g})",
                  f"{'d_waic':>16} {c['d_waic']:.10g}  d_dic {c['d_dic']:.10g}"]
    return lines


class Predictive(Handle):
    """One ``olpe_lik`` on the sampler's GPU: a copy of its staged cutout, independent of
    the sampler afterwards.  ``pivot``: the parameter vector whose deviance plane the sums
    are shifted by (the posterior mean, say); None takes the first usable row folded."""

    _destroy = "olpe_lik_destroy"

    def __init__(self, sampler, pivot=None):
        self.n, self.nsrc, self.np_, self.ps = sampler.n, sampler.nsrc, sampler.np_, sampler.ps
        self.bkgd_mode = int(getattr(sampler, "bkgd_mode", 0))
        self.data = np.array(sampler._img, dtype=np.float64)
        self._lib = _lib.load()
        pv = None if pivot is None else self._vec(pivot, "pivot")
        h = C.c_void_p()
        check(self._lib.olpe_lik_create(sampler._ctx, None if pv is None else _pd(pv),
                                        C.byref(h)))
        self._h = h

    def _vec(self, v, what):
        v = np.ascontiguousarray(v, dtype=np.float64).ravel()
        if v.size not in (self.np_, self.ps):
            raise ValueError(f"{what} of {v.size} entries, expected {self.np_} or {self.ps}")
        return np.ascontiguousarray(v[:self.np_])

    # -- folding ------------------------------------------------------------------
    def fold(self, sampler, row_step: int = 1, walker_step: int = 1):
        """Fold rows 0, row_step, ... of walkers 0, walker_step, ... of the sampler's last
        launch from its device chain (once per launch; async on the sampler's stream, no
        copy).  A full fold of an EXACT launch costs more than the launch did."""
        check(self._lib.olpe_lik_fold_ctx(self._h, sampler._ctx, int(row_step),
                                          int(walker_step)))

    def fold_rows(self, rows):
        """Fold host rows [..., PS], in memory order."""
        r = np.ascontiguousarray(rows, dtype=np.float64)
        if r.ndim < 1 or r.shape[-1] != self.ps:
            raise ValueError(f"rows of shape {r.shape}, expected [..., {self.ps}]")
        check(self._lib.olpe_lik_fold_rows(self._h, _pd(r), r.size // self.ps))

    def point(self, vec):
        """x = ((D - M) / err)^2 of one parameter vector, [n][n], NaN at masked pixels."""
        v = self._vec(vec, "vector")
        out = np.empty((self.n, self.n))
        check(self._lib.olpe_lik_point(self._h, _pd(v), _pd(out)))
        return out

    # -- state --------------------------------------------------------------------
    def state(self):
        """``{"n", "n_bad", "pivot" [PS], "a1", "a2", "m", "l" [n][n], "best" [PS]}``; pivot
        / best are NaN while there is none."""
        n, bad = C.c_longlong(0), C.c_longlong(0)
        pivot, best = np.empty(self.ps), np.empty(self.ps)
        img = {k: np.empty((self.n, self.n)) for k in ("a1", "a2", "m", "l")}
        check(self._lib.olpe_lik_get(self._h, C.byref(n), C.byref(bad), _pd(pivot),
                                     _pd(img["a1"]), _pd(img["a2"]), _pd(img["m"]),
                                     _pd(img["l"]), _pd(best)))
        return {"n": int(n.value), "n_bad": int(bad.value), "pivot": pivot, **img, "best": best}

    def add(self, state):
        """Merge another object's, rank's or checkpoint's ``state()`` (equal pivots, unless
        this object is still empty: it then adopts the incoming one)."""
        arr = {k: np.ascontiguousarray(state[k], dtype=np.float64)
               for k in ("pivot", "a1", "a2", "m", "l", "best")}
        if (arr["pivot"].shape != (self.ps,) or arr["best"].shape != (self.ps,)
                or any(arr[k].shape != (self.n, self.n) for k in ("a1", "a2", "m", "l"))):
            raise ValueError("state of other shapes than this object's")
        check(self._lib.olpe_lik_add(self._h, int(state["n"]), int(state["n_bad"]),
                                     _pd(arr["pivot"]), _pd(arr["a1"]), _pd(arr["a2"]),
                                     _pd(arr["m"]), _pd(arr["l"]), _pd(arr["best"])))

    def reset(self):
        check(self._lib.olpe_lik_reset(self._h))

    def best(self):
        """The folded row with the smallest chi^2 column [PS] (NaN while there is none)."""
        best = np.empty(self.ps)
        check(self._lib.olpe_lik_get(self._h, None, None, None, None, None, None, None,
                                     _pd(best)))
        return best

    # -- results ------------------------------------------------------------------
    def finalize(self, theta_hat=None):
        """(planes [7][n][n], scalars [17]) as olpe_lik_finalize returns them."""
        planes = np.empty((len(PLANES), self.n, self.n))
        scal = np.empty(len(SCALARS))
        th = None if theta_hat is None else self._vec(theta_hat, "theta_hat")
        check(self._lib.olpe_lik_finalize(self._h, None if th is None else _pd(th),
                                          _pd(planes), _pd(scal)))
        return planes, scal

    @staticmethod
    def _scalars(scal):
        out = {k: float(v) for k, v in zip(SCALARS, scal)}
        for k in _INTS:
            out[k] = int(out[k])
        return out

    def images(self, theta_hat=None):
        """The named planes: mean_dev and std_dev (ddof 0) of x over the samples, lppd =
        log mean exp(-x / 2), p_waic = var(-x / 2) (ddof 1), elpd = lppd - p_waic, dev_best
        (x of the best row), dev_at (x of ``theta_hat``; NaN without one).  NaN at masked
        and poisoned pixels."""
        planes, _ = self.finalize(theta_hat)
        return dict(zip(PLANES, planes))

    def scalars(self, theta_hat=None):
        """samples, n_bad, (unmasked) pixels, poisoned; with N = pixels - poisoned: the sums
        lppd, p_waic, elpd_waic, waic = -2 elpd_waic, se_elpd = sqrt(N var(elpd_i)) (ddof 1),
        p_waic_high (pixels with p_waic > 0.4), mean_deviance, reduced = mean_deviance /
        (N - P), deviance_best, deviance_at = D(theta_hat), p_d = mean_deviance -
        deviance_at, dic = deviance_at + 2 p_d, and log_norm = sum of k_i."""
        return self._scalars(self.finalize(theta_hat)[1])

    def save(self, path, theta_hat=None, thin=1):
        """One ``.npz`` (``write_npz``): the planes by name, the scalars
        (``scalar_<name>``), the state and its pivot plane ``c``, the data and mask used,
        nsrc, bkgd_mode and thin.  Returns (images, scalars)."""
        planes, scal = self.finalize(theta_hat)
        st = self.state()
        img, sc = dict(zip(PLANES, planes)), self._scalars(scal)
        mask = np.isnan(self.point(st["best"]))
        write_npz(path, img, sc, st, self.point(st["pivot"]), self.data, mask, self.nsrc,
                  self.bkgd_mode, thin)
        return img, sc

    def write_fits(self, prefix, theta_hat=None):
        """``<prefix>_meandev.fits`` (mean_dev), ``_elpd.fits`` and ``_pwaic.fits``
        (float64).  Returns the paths."""
        img = self.images(theta_hat)
        paths = []
        for suffix, key in (("meandev", "mean_dev"), ("elpd", "elpd"), ("pwaic", "p_waic")):
            paths.append(f"{prefix}_{suffix}.fits")
            fitsio.write(paths[-1], img[key])
        return paths
