"""The companion detection map and contrast curve of a fit, folded on the device
(include/olpe.h, olpe_detect_*).

Two questions a PSF fit of a binary leaves open: is there another source in this frame, and
how faint a one would have been seen, and where?  Both are one computation: at every
candidate position c of a lattice over the frame, the matched filter of a sample's residual
with that sample's own unit PSF (all sources share one shape, apf_step2.py:78-103),

    psi(u, v) = (1 - q) g1(u, v) + q g2(u - dx, v - dy)
    z_i = w_i (D_i - M_i),  w_i = 1 / err_i^2 (0 where masked),  K_i = psi(x_i - x_c, y_i - y_c)
    N = sum z_i K_i,  Q = sum w_i K_i^2,  A = N / Q,  sigma_A = 1 / sqrt(Q),  snr = N / sqrt(Q)

A is the maximum-likelihood amplitude of one more source of the shared shape, in the units
of A_k - b, so A / (A_0 - b) is its flux ratio to the primary.  ``Detect`` folds A, sigma_A
and snr over a whole ensemble, so that the PSF's posterior scatter enters the detection
sigma (``sigma_total``, the law of total variance).  The state is five planes of shifted
sums and a few numbers; it merges by addition (``add``) whenever the pivots are equal.

This is a score test: the fitted sources stay at each sample's values and nothing is
refitted.  Near a fitted source the extra amplitude is degenerate with that source's own,
which is why ``candidates`` flags (and keeps) what lies within ``exclude_px`` of one.

The NumPy functions below (``planes_from_state``, ``contrast_curve``, ``candidates``,
``merge_states``, ``table_lines``) need no GPU.  Not covered: refitting with the extra source,
a step-1 guess file for the 3-source scripts, sky-frame position angles, a collective over
the state, a factorised (FAST) fold, ``--detect`` in step 2.  (What the threshold means over
a map's correlated candidates: detect_null.)  Nothing here imports matplotlib or the oracle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, fitsio
from ._handle import Handle, _pd, load_npz  # noqa: F401  (load_npz: Detect.save's reader)
from ._lib import check

SUMS = ("d_amp", "d_amp2", "var_stat", "d_snr", "d_snr2")
PLANES = ("amp_mean", "amp_std", "sigma_stat", "sigma_total", "snr_mean", "snr_std",
          "snr_marg", "amp_best", "sigma_best", "snr_best")
SCALARS = ("samples", "n_bad", "pixels", "blind", "max_snr", "max_snr_at", "min_snr",
           "median_sigma")
POINT = ("amp", "sigma", "snr")
OVERSAMPLE = (1, 2, 4)


def lattice_side(n, oversample=1):
    """Candidates per axis: x_c, y_c = j / oversample, j = 0 .. oversample (n - 1)."""
    return int(oversample) * (int(n) - 1) + 1


def lattice(n, oversample=1):
    """The lattice's coordinates along one axis, in pixels."""
    return np.arange(lattice_side(n, oversample)) / float(oversample)


def flux0_of(theta, nsrc):
    """A_0 - b of a parameter vector: the primary's amplitude above the offset."""
    t = np.asarray(theta, dtype=np.float64)
    return float(t[6] - t[9]) if nsrc == 2 else float(t[8] - t[12])


def known_of(theta, nsrc):
    """The fitted sources' positions [(x, y)], the primary first."""
    t = np.asarray(theta, dtype=np.float64)
    return [(float(t[2 * s]), float(t[2 * s + 1])) for s in range(nsrc)]


def default_exclude_px(theta, nsrc):
    """2.355 x the larger narrow width of a parameter vector: the narrow core's FWHM."""
    t = np.asarray(theta, dtype=np.float64)
    k = 10 if nsrc == 2 else 13
    return 2.355 * float(max(t[k], t[k + 1]))


def planes_from_state(state, pivot_planes, best_planes=None):
    """olpe_detect_finalize's arithmetic on a ``state()`` and the pivot's ``point`` planes
    [3][g][g] (A_p, sigma_p, snr_p), so a merged state finishes anywhere.  Returns (planes by
    name, scalars); the ``*_best`` planes and ``pixels`` only with ``best_planes`` given
    (``point(best)``) -- the state does not hold the frame."""
    n = int(state["n"])
    if n <= 0:
        raise ValueError(f"no usable sample in the state ({int(state['n_bad'])} unusable)")
    s = np.asarray(state["sums"], dtype=np.float64)
    piv = np.asarray(pivot_planes, dtype=np.float64)
    nu = np.float64(n)
    with np.errstate(all="ignore"):
        m1 = s[0] / nu
        va = (s[1] - s[0] * m1) / nu
        vac = np.where(va < 0.0, 0.0, va)
        ms = s[2] / nu
        m4 = s[3] / nu
        vs = (s[4] - s[3] * m4) / nu
        out = {"amp_mean": piv[0] + m1, "amp_std": np.sqrt(vac), "sigma_stat": np.sqrt(ms),
               "sigma_total": np.sqrt(ms + vac), "snr_mean": piv[2] + m4,
               "snr_std": np.sqrt(np.where(vs < 0.0, 0.0, vs))}
        out["snr_marg"] = out["amp_mean"] / out["sigma_total"]
    if best_planes is not None:
        b = np.asarray(best_planes, dtype=np.float64)
        out.update(amp_best=b[0], sigma_best=b[1], snr_best=b[2])
    marg = out["snr_marg"].ravel()
    fin = ~np.isnan(marg)
    at = int(np.flatnonzero(fin)[np.argmax(marg[fin])]) if fin.any() else -1
    tot = out["sigma_total"]
    sc = {"samples": n, "n_bad": int(state["n_bad"]), "blind": int(np.isnan(ms).sum()),
          "max_snr": float(marg[at]) if at >= 0 else float("nan"), "max_snr_at": at,
          "min_snr": float(marg[fin].min()) if fin.any() else float("nan"),
          "median_sigma": float(np.median(tot[~np.isnan(tot)])) if (~np.isnan(tot)).any()
          else float("nan")}
    return out, sc


def merge_states(a, b):
    """The state of a's rows followed by b's (``Detect.add`` on dicts): the sums add when the
    pivots' parameters are equal in every bit; an empty ``a`` adopts b's pivot; b's best row
    wins only with a strictly smaller chi^2.  ValueError when the pivots differ."""
    na, nb = int(a["n"]), int(b["n"])
    out = {"n": na + nb, "n_bad": int(a["n_bad"]) + int(b["n_bad"])}
    pa, pb = (np.asarray(x["pivot"], dtype=np.float64) for x in (a, b))
    if nb == 0:
        out.update(pivot=pa.copy(), sums=np.array(a["sums"], dtype=np.float64),
                   best=np.array(a["best"], dtype=np.float64))
        return out
    if na == 0:
        out.update(pivot=pb.copy(), sums=np.array(b["sums"], dtype=np.float64),
                   best=np.array(b["best"], dtype=np.float64))
        return out
    if pa[:-1].tobytes() != pb[:-1].tobytes():
        raise ValueError("the pivots differ: sums about different planes do not add")
    ba, bb = (np.asarray(x["best"], dtype=np.float64) for x in (a, b))
    take_b = not np.isnan(bb[-1]) and (np.isnan(ba[-1]) or bb[-1] < ba[-1])
    out.update(pivot=pa.copy(),
               sums=np.asarray(a["sums"], dtype=np.float64) + np.asarray(b["sums"], dtype=np.float64),
               best=(bb if take_b else ba).copy())
    return out


def _dmag(ratio):
    with np.errstate(all="ignore"):
        r = np.asarray(ratio, dtype=np.float64)
        return -2.5 * np.log10(np.where(r > 0.0, r, np.nan))


def contrast_curve(sigma, centre, flux0, pixscale, k=5, bin_px=1.0, oversample=1):
    """The k-sigma contrast against separation from ``centre`` = (x, y), the primary's mean
    position: ring i holds the candidates with bin_px i <= r < bin_px (i + 1); NaN
    candidates are left out, rings without a candidate too.  ``flux0`` = A_0 - b at
    theta_hat: the amplitude ratio is the flux ratio, the shape being shared.  Returns
    arrays by name: ``count``, ``sep_px`` (the ring's middle), ``sep_mas``, ``contrast_median``,
    ``contrast_min`` (of k sigma / flux0) and ``dmag_median``, ``dmag_min`` = -2.5 log10."""
    sig = np.asarray(sigma, dtype=np.float64)
    g = sig.shape[0]
    ax = np.arange(g) / float(oversample)
    r = np.hypot(ax[None, :] - float(centre[0]), ax[:, None] - float(centre[1]))
    ok = ~np.isnan(sig)
    ring = np.floor(r / float(bin_px)).astype(np.int64)
    c = float(k) * sig / float(flux0)
    rows = []
    for i in np.unique(ring[ok]):
        v = c[ok & (ring == i)]
        rows.append((v.size, (i + 0.5) * bin_px, (i + 0.5) * bin_px * pixscale, np.median(v),
                     v.min()))
    a = np.array(rows, dtype=np.float64).reshape(-1, 5)
    return {"count": a[:, 0].astype(np.int64), "sep_px": a[:, 1], "sep_mas": a[:, 2],
            "contrast_median": a[:, 3], "contrast_min": a[:, 4],
            "dmag_median": _dmag(a[:, 3]), "dmag_min": _dmag(a[:, 4])}


def candidates(snr, amp, sigma, known, threshold=5.0, exclude_px=0.0, oversample=1,
               flux0=None, pixscale=None):
    """The strict local maxima of the ``snr`` map at or above ``threshold``: larger than each
    of the (up to 8) neighbours on the candidate lattice, a NaN neighbour counting as none;
    a plateau has no strict maximum.  ``known``: the fitted sources' (x, y), the primary
    first.  Each candidate is a dict: ``x``, ``y`` (pixels), ``index``, ``snr``, ``amp``, ``sigma``,
    ``contrast`` = amp / flux0 and ``dmag`` (with ``flux0``), ``sep_px`` (``sep_mas`` with
    ``pixscale``) and ``pa_deg`` from the primary in the detector frame (from +x towards +y),
    and ``flagged``: within ``exclude_px`` of a fitted source, where the test is degenerate
    with that source's amplitude -- flagged candidates are not dropped.  Sorted by snr,
    the largest first."""
    s = np.asarray(snr, dtype=np.float64)
    g = s.shape[0]
    pad = np.full((g + 2, g + 2), -np.inf)
    pad[1:-1, 1:-1] = np.where(np.isnan(s), -np.inf, s)
    c = pad[1:-1, 1:-1]
    peak = c >= threshold
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                peak &= c > pad[1 + dy:g + 1 + dy, 1 + dx:g + 1 + dx]
    out = []
    for jy, jx in zip(*np.nonzero(peak)):
        x, y = jx / float(oversample), jy / float(oversample)
        d = {"x": x, "y": y, "index": int(jy * g + jx), "snr": float(s[jy, jx]),
             "amp": float(amp[jy, jx]), "sigma": float(sigma[jy, jx]),
             "flagged": bool(any(np.hypot(x - kx, y - ky) <= exclude_px for kx, ky in known))}
        if flux0 is not None:
            d["contrast"] = d["amp"] / float(flux0)
            d["dmag"] = float(_dmag(d["contrast"]))
        if known:
            ddx, ddy = x - known[0][0], y - known[0][1]
            d["sep_px"] = float(np.hypot(ddx, ddy))
            if pixscale is not None:
                d["sep_mas"] = d["sep_px"] * float(pixscale)
            d["pa_deg"] = float(np.degrees(np.arctan2(ddy, ddx)) % 360.0)
        out.append(d)
    return sorted(out, key=lambda d: -d["snr"])


def table_lines(scalars, cands=None, curve=None, oversample=1):
    """The lines step 3 prints: the scalars, the candidate table and the contrast curve."""
    s = scalars
    lines = [f"{'samples':>16} {s['samples']}  (unusable rows {s['n_bad']})",
             f"{'pixels':>16} {s.get('pixels', 'n/a')}  (blind candidates {s['blind']})",
             f"{'median sigma':>16} {s['median_sigma']:.6g}",
             f"{'snr range':>16} {s['min_snr']:.4g} .. {s['max_snr']:.4g}  (max at candidate "
             f"{s['max_snr_at']})"]
    if cands is not None:
        lines.append(f"{'candidates':>16} {len(cands)}  "
                     f"({sum(not c['flagged'] for c in cands)} outside the fitted sources)")
        if cands:
            lines.append(f"{'':>4}{'x':>9}{'y':>9}{'snr':>9}{'amp':>12}{'sigma':>11}"
                         f"{'contrast':>11}{'dmag':>8}{'sep_px':>9}{'pa_deg':>9}  flag")
        for c in cands:
            lines.append(f"{'':>4}{c['x']:9.2f}{c['y']:9.2f}{c['snr']:9.2f}{c['amp']:12.5g}"
                         f"{c['sigma']:11.4g}{c.get('contrast', float('nan')):11.4g}"
                         f"{c.get('dmag', float('nan')):8.2f}{c.get('sep_px', float('nan')):9.2f}"
                         f"{c.get('pa_deg', float('nan')):9.2f}  "
                         f"{'near a fitted source' if c['flagged'] else '-'}")
    if curve is not None:
        lines.append(f"{'contrast curve':>16} {len(curve['count'])} rings")
        lines.append(f"{'':>4}{'sep_px':>9}{'sep_mas':>10}{'count':>7}{'median':>11}{'dmag':>8}"
                     f"{'best':>11}{'dmag':>8}")
        for i in range(len(curve["count"])):
            lines.append(f"{'':>4}{curve['sep_px'][i]:9.2f}{curve['sep_mas'][i]:10.2f}"
                         f"{int(curve['count'][i]):7d}{curve['contrast_median'][i]:11.4g}"
                         f"{curve['dmag_median'][i]:8.2f}{curve['contrast_min'][i]:11.4g}"
                         f"{curve['dmag_min'][i]:8.2f}")
    return lines


class Detect(Handle):
    """One ``olpe_detect`` on the sampler's GPU: a copy of its staged cutout, independent of
    the sampler afterwards.  ``pivot``: the parameter vector whose planes the sums are
    shifted by (the posterior mean, say); None takes the first usable row folded.
    ``oversample``: candidates per pixel and axis, 1, 2 or 4."""

    _destroy = "olpe_detect_destroy"

    def __init__(self, sampler, pivot=None, oversample=1):
        self.n, self.nsrc, self.np_, self.ps = sampler.n, sampler.nsrc, sampler.np_, sampler.ps
        self.oversample = int(oversample)
        self.g = lattice_side(self.n, self.oversample)
        self.data = np.array(sampler._img, dtype=np.float64)
        self.mask = np.array(sampler._mask, dtype=bool)
        self._lib = _lib.load()
        pv = None if pivot is None else self._vec(pivot, "pivot")
        h = C.c_void_p()
        check(self._lib.olpe_detect_create(sampler._ctx, None if pv is None else _pd(pv),
                                           self.oversample, C.byref(h)))
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
        copy).  A sample costs 2 G n^2 FP64 FMAs: thin."""
        check(self._lib.olpe_detect_fold_ctx(self._h, sampler._ctx, int(row_step),
                                             int(walker_step)))

    def fold_rows(self, rows):
        """Fold host rows [..., PS], in memory order."""
        r = np.ascontiguousarray(rows, dtype=np.float64)
        if r.ndim < 1 or r.shape[-1] != self.ps:
            raise ValueError(f"rows of shape {r.shape}, expected [..., {self.ps}]")
        check(self._lib.olpe_detect_fold_rows(self._h, _pd(r), r.size // self.ps))

    def point(self, vec):
        """(A, sigma_A, snr) [3][g][g] of one explicit vector; the state is left as it is."""
        v = self._vec(vec, "vector")
        out = np.empty((3, self.g, self.g))
        check(self._lib.olpe_detect_point(self._h, _pd(v), _pd(out)))
        return out

    # -- state --------------------------------------------------------------------
    def state(self):
        """``{"n", "n_bad", "pivot" [PS], "sums" [5][g][g], "best" [PS]}``; pivot / best are
        NaN while there is none."""
        n, bad = C.c_longlong(0), C.c_longlong(0)
        pivot, best = np.empty(self.ps), np.empty(self.ps)
        sums = np.empty((len(SUMS), self.g, self.g))
        check(self._lib.olpe_detect_get(self._h, C.byref(n), C.byref(bad), _pd(pivot),
                                        _pd(sums), _pd(best)))
        return {"n": int(n.value), "n_bad": int(bad.value), "pivot": pivot, "sums": sums,
                "best": best}

    def add(self, state):
        """Merge another object's, rank's or checkpoint's ``state()`` (equal pivots, unless
        this object is still empty: it then adopts the incoming one)."""
        arr = {k: np.ascontiguousarray(state[k], dtype=np.float64)
               for k in ("pivot", "sums", "best")}
        if (arr["pivot"].shape != (self.ps,) or arr["best"].shape != (self.ps,)
                or arr["sums"].shape != (len(SUMS), self.g, self.g)):
            raise ValueError("state of other shapes than this object's")
        check(self._lib.olpe_detect_add(self._h, int(state["n"]), int(state["n_bad"]),
                                        _pd(arr["pivot"]), _pd(arr["sums"]), _pd(arr["best"])))

    def reset(self):
        check(self._lib.olpe_detect_reset(self._h))

    def best(self):
        """The folded row with the smallest chi^2 column [PS] (NaN while there is none)."""
        best = np.empty(self.ps)
        check(self._lib.olpe_detect_get(self._h, None, None, None, None, _pd(best)))
        return best

    # -- results ------------------------------------------------------------------
    def finalize(self):
        """(planes [10][g][g], scalars [8]) as olpe_detect_finalize returns them."""
        planes = np.empty((len(PLANES), self.g, self.g))
        scal = np.empty(len(SCALARS))
        check(self._lib.olpe_detect_finalize(self._h, _pd(planes), _pd(scal)))
        return planes, scal

    @staticmethod
    def _scalars(scal):
        out = {k: float(v) for k, v in zip(SCALARS, scal)}
        for k in ("samples", "n_bad", "pixels", "blind", "max_snr_at"):
            out[k] = int(out[k])
        return out

    def maps(self):
        """The named planes [g][g]: amp_mean, amp_std (ddof 0), sigma_stat = sqrt(mean
        sigma_A^2), sigma_total = sqrt(mean sigma_A^2 + var A), snr_mean, snr_std, snr_marg =
        amp_mean / sigma_total, and the best row's amp_best, sigma_best, snr_best; NaN at
        candidates no unmasked pixel sees."""
        planes, _ = self.finalize()
        return dict(zip(PLANES, planes))

    def scalars(self):
        """samples, n_bad, (unmasked) pixels, blind candidates, max_snr (of snr_marg) and
        its candidate max_snr_at (row * g + column), min_snr, median_sigma (of
        sigma_total)."""
        return self._scalars(self.finalize()[1])

    def save(self, path, **extra):
        """One ``.npz``: the planes by name, ``scalar_<name>``, the lattice, the state with
        the pivot's planes (``planes_from_state`` finishes it), data and mask, and whatever
        arrays ``extra`` names.  Returns (maps, scalars)."""
        planes, scal = self.finalize()
        st = self.state()
        img, sc = dict(zip(PLANES, planes)), self._scalars(scal)
        with open(path, "wb") as f:
            np.savez(f, data=self.data, mask=self.mask, nsrc=np.int64(self.nsrc),
                     oversample=np.int64(self.oversample),
                     lattice=lattice(self.n, self.oversample), n=np.int64(st["n"]),
                     n_bad=np.int64(st["n_bad"]), pivot=st["pivot"], sums=st["sums"],
                     best=st["best"], pivot_planes=self.point(st["pivot"]), **img,
                     **{"scalar_" + k: np.float64(v) for k, v in sc.items()},
                     **{k: np.asarray(v) for k, v in extra.items()})
        return img, sc

    def write_fits(self, prefix, flux0=None, k=5.0):
        """``<prefix>_snr.fits`` (snr_marg), ``_sigma.fits`` (sigma_total) and
        ``_contrast.fits`` (k sigma_total / flux0; flux0 = A_0 - b of the best row unless
        given), float64.  Returns the paths."""
        img = self.maps()
        if flux0 is None:
            flux0 = flux0_of(self.best(), self.nsrc)
        paths = []
        for suffix, plane in (("snr", img["snr_marg"]), ("sigma", img["sigma_total"]),
                              ("contrast", float(k) * img["sigma_total"] / float(flux0))):
            paths.append(f"{prefix}_{suffix}.fits")
            fitsio.write(paths[-1], plane)
        return paths


def state_of(saved):
    """The ``state()`` dict inside a saved file (a path or its dict)."""
    z = load_npz(saved) if isinstance(saved, (str, bytes)) or hasattr(saved, "__fspath__") else saved
    return {"n": int(z["n"]), "n_bad": int(z["n_bad"]),
            **{k: np.array(z[k], dtype=np.float64) for k in ("pivot", "sums", "best")}}
