"""The posterior's model and residual images, folded on the device (include/olpe.h,
olpe_resid_*).

The reference's README opens with ``model_residuals_all.png``: data, model, residual.
``Residuals`` takes that picture over a whole ensemble: every folded sample's
``build_analytical_model`` (apf_step2.py:106-124; 3body/apf_step2_3body.py:106-125) is
evaluated on the GPU in the EXACT operation order and folded per pixel into the mean
model, its scatter, and the best sample's model and residuals in units of sigma.  The
state is three images and a few numbers; it merges by addition (``add``) whenever the
pivots are equal, so ranks, contexts and checkpoints combine on the host.

Not covered: the drawing, a factorised (FAST) fold, a collective over the state,
photometry (per-pixel chi^2 over all samples: ``predictive.Predictive``).  Nothing here imports matplotlib or
the oracle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, fitsio
from ._handle import Handle, _pd, load_npz  # noqa: F401  (load_npz: Residuals.save's reader)
from ._lib import check

PLANES = ("mean_model", "std_model", "best_model", "resid", "nresid", "mean_resid",
          "mean_nresid")
SCALARS = ("samples", "n_bad", "pixels", "best_chi2", "chi2_best_model", "chi2_mean_model",
           "max_abs_nresid", "max_abs_nresid_at")


def mean_std(pivot_image, s1, s2, n):
    """(mean, std) of the folded models from the shifted sums about ``pivot_image``:
    mean = R + S1 / n, std = sqrt((S2 - S1^2 / n) / n) (``np.std``, ddof 0), the arithmetic
    of olpe_resid_finalize's planes 0 and 1."""
    s1 = np.asarray(s1, dtype=np.float64)
    s2 = np.asarray(s2, dtype=np.float64)
    n = np.float64(n)
    m1 = s1 / n
    var = (s2 - s1 * m1) / n
    return np.asarray(pivot_image, dtype=np.float64) + m1, np.sqrt(np.maximum(var, 0.0))


class Residuals(Handle):
    """One ``olpe_resid`` on the sampler's GPU: a copy of its staged cutout, independent of
    the sampler afterwards.  ``pivot``: the parameter vector whose model the sums are
    shifted by (the posterior mean from ``Sampler.moments_summary``, say); None takes the
    first usable row folded."""

    _destroy = "olpe_resid_destroy"

    def __init__(self, sampler, pivot=None):
        self.n, self.nsrc, self.np_, self.ps = sampler.n, sampler.nsrc, sampler.np_, sampler.ps
        self.data = np.array(sampler._img, dtype=np.float64)
        self._lib = _lib.load()
        pv = None
        if pivot is not None:
            pv = np.ascontiguousarray(pivot, dtype=np.float64).ravel()
            if pv.size not in (self.np_, self.ps):
                raise ValueError(f"pivot of {pv.size} entries, expected {self.np_} or {self.ps}")
            pv = np.ascontiguousarray(pv[:self.np_])
        h = C.c_void_p()
        check(self._lib.olpe_resid_create(sampler._ctx, None if pv is None else _pd(pv),
                                          C.byref(h)))
        self._h = h

    # -- folding ------------------------------------------------------------------
    def fold(self, sampler, row_step: int = 1, walker_step: int = 1):
        """Fold rows 0, row_step, ... of walkers 0, walker_step, ... of the sampler's last
        launch from its device chain (once per launch; async on the sampler's stream, no
        copy).  A full fold of a launch costs about what the launch did."""
        check(self._lib.olpe_resid_fold_ctx(self._h, sampler._ctx, int(row_step),
                                            int(walker_step)))

    def fold_rows(self, rows):
        """Fold host rows [..., PS], in memory order."""
        r = np.ascontiguousarray(rows, dtype=np.float64)
        if r.ndim < 1 or r.shape[-1] != self.ps:
            raise ValueError(f"rows of shape {r.shape}, expected [..., {self.ps}]")
        check(self._lib.olpe_resid_fold_rows(self._h, _pd(r), r.size // self.ps))

    # -- state --------------------------------------------------------------------
    def state(self):
        """``{"n", "n_bad", "pivot" [PS], "s1", "s2" [n][n], "best" [PS]}``; pivot / best
        are NaN while there is none."""
        n, bad = C.c_longlong(0), C.c_longlong(0)
        pivot, best = np.empty(self.ps), np.empty(self.ps)
        s1, s2 = np.empty((self.n, self.n)), np.empty((self.n, self.n))
        check(self._lib.olpe_resid_get(self._h, C.byref(n), C.byref(bad), _pd(pivot), _pd(s1),
                                       _pd(s2), _pd(best)))
        return {"n": int(n.value), "n_bad": int(bad.value), "pivot": pivot, "s1": s1, "s2": s2,
                "best": best}

    def add(self, state):
        """Merge another object's, rank's or checkpoint's ``state()`` (equal pivots, unless
        this object is still empty: it then adopts the incoming one)."""
        arr = {k: np.ascontiguousarray(state[k], dtype=np.float64)
               for k in ("pivot", "s1", "s2", "best")}
        if (arr["pivot"].shape != (self.ps,) or arr["best"].shape != (self.ps,)
                or arr["s1"].shape != (self.n, self.n) or arr["s2"].shape != (self.n, self.n)):
            raise ValueError("state of other shapes than this object's")
        check(self._lib.olpe_resid_add(self._h, int(state["n"]), int(state["n_bad"]),
                                       _pd(arr["pivot"]), _pd(arr["s1"]), _pd(arr["s2"]),
                                       _pd(arr["best"])))

    def reset(self):
        check(self._lib.olpe_resid_reset(self._h))

    def best(self):
        """The folded row with the smallest chi^2 column [PS] (NaN while there is none)."""
        best = np.empty(self.ps)
        check(self._lib.olpe_resid_get(self._h, None, None, None, None, None, _pd(best)))
        return best

    # -- results ------------------------------------------------------------------
    def finalize(self):
        """(planes [7][n][n], scalars [8]) as olpe_resid_finalize returns them."""
        planes = np.empty((len(PLANES), self.n, self.n))
        scal = np.empty(len(SCALARS))
        check(self._lib.olpe_resid_finalize(self._h, _pd(planes), _pd(scal)))
        return planes, scal

    def _scalars(self, scal):
        out = {k: float(v) for k, v in zip(SCALARS, scal)}
        for k in ("samples", "n_bad", "pixels", "max_abs_nresid_at"):
            out[k] = int(out[k])
        dof = out["pixels"] - self.np_
        out["reduced_chi2"] = out["best_chi2"] / dof if dof > 0 else float("nan")
        return out

    def images(self):
        """The named planes: mean_model, std_model (ddof 0), best_model, resid = D -
        best_model, nresid = resid / err, mean_resid = D - mean_model, mean_nresid; the
        residual planes are NaN at masked pixels."""
        planes, _ = self.finalize()
        return dict(zip(PLANES, planes))

    def scalars(self):
        """samples, n_bad, (unmasked) pixels, best_chi2 as the row stores it,
        chi2_best_model / chi2_mean_model (sum of nresid^2 / mean_nresid^2),
        max_abs_nresid and its pixel (row * n + column), and reduced_chi2 = best_chi2 /
        (pixels - P)."""
        return self._scalars(self.finalize()[1])

    def save(self, path):
        """One ``.npz``: the planes by name, the scalars, the pivot, the best row and the
        data and mask used.  Returns (images, scalars)."""
        planes, scal = self.finalize()
        st = self.state()
        img, sc = dict(zip(PLANES, planes)), self._scalars(scal)
        with open(path, "wb") as f:
            np.savez(f, data=self.data, mask=np.isnan(img["nresid"]), pivot=st["pivot"],
                     best=st["best"], **img, **{"scalar_" + k: np.float64(v) for k, v in sc.items()})
        return img, sc

    def write_fits(self, prefix):
        """``<prefix>_model.fits`` (best_model), ``_meanmodel.fits``, ``_resid.fits`` and
        ``_nresid.fits`` (float64).  Returns the paths."""
        img = self.images()
        paths = []
        for suffix, key in (("model", "best_model"), ("meanmodel", "mean_model"),
                            ("resid", "resid"), ("nresid", "nresid")):
            paths.append(f"{prefix}_{suffix}.fits")
            fitsio.write(paths[-1], img[key])
        return paths
