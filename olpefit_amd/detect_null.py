"""False-alarm calibration of the companion detection map (include/olpe.h,
olpe_detect_null_*): what a "5 sigma" candidate of ``detect.Detect``'s map means.

A candidate's snr is standard normal under the noise model, but a map is thousands of
strongly correlated candidates and what a user reports is the largest one.  ``DetectNull``
draws noise frames under the fit's own noise model on the device, passes each through the
same matched filter at one parameter vector theta and reduces each map to its maximum:

    eps_r = np.random.RandomState((seed + r) mod 2^32).standard_normal(n * n), raster order
    y_r,i = eps_r,i (1 / err_i), 0 at masked pixels
    snr_r(c) = scale(c) (sum_i K_i(c) y_r,i) / sqrt(Q(c)), NaN where Q(c) = 0

with K, Q of ``detect`` at theta.  Per realisation: the maximum over all candidates and over
those farther than ``exclude_px`` from every fitted source (``detect.candidates``' flag), the
number of strict local maxima at or above ``threshold`` (``detect.candidates``' rule) and the
maximum of every ring of ``detect.contrast_curve``.

The NumPy functions (``noise_frames``, ``map_stats``, ``merge_results``, ``tail_fit``, ``fap``,
``threshold_for``, ``ring_thresholds``, ``calibrated_curve``, ``table_lines``) need no GPU.  Beyond
the largest maxima drawn the false-alarm probability is extrapolated with the form of a 2-D
Gaussian random field's excursion probability, FAP(s) = 1 - exp(-a s exp(-s^2 / 2)), anchored
at an empirical quantile.

Not covered: the fit is not redone per realisation, so the noise the fitted parameters absorb
(the hat matrix of J^T J) is ignored; non-Gaussian or correlated detector noise; completeness
by injection; a collective (RCCL) split of the realisations -- ``merge_results`` joins what
ranks ran with disjoint index ranges.  Nothing here imports matplotlib or the oracle.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import math

import numpy as np

from . import _lib
from ._handle import Handle, _pd
from ._lib import check
from .detect import _dmag

FIELDS = ("max_all", "argmax_all", "max_out", "argmax_out", "peaks_all", "peaks_out", "ring_max")
SETTINGS = ("g", "oversample", "exclude_px", "bin_px", "threshold", "centre", "known", "vec",
            "scale_id")


# -- the definition, in NumPy ---------------------------------------------------------
def noise_frames(seed, r0, count, n):
    """eps [count][n][n] of realisations r0 .. r0 + count - 1: realisation r is
    ``RandomState((seed + r) mod 2^32).standard_normal(n * n)`` in raster order."""
    out = np.empty((int(count), int(n), int(n)))
    for k in range(int(count)):
        rs = np.random.RandomState((int(seed) + int(r0) + k) % 2 ** 32)
        out[k] = rs.standard_normal(int(n) * int(n)).reshape(int(n), int(n))
    return out


def rings(g, centre, bin_px=1.0, oversample=1):
    """The ring of every candidate [g][g]: floor(r / bin_px) of its distance from ``centre`` =
    (x, y), ``detect.contrast_curve``'s."""
    ax = np.arange(int(g)) / float(oversample)
    r = np.hypot(ax[None, :] - float(centre[0]), ax[:, None] - float(centre[1]))
    return np.floor(r / float(bin_px)).astype(np.int64)


def outside(g, known, exclude_px, oversample=1):
    """True [g][g] where a candidate lies farther than ``exclude_px`` from every (x, y) of
    ``known``: what ``detect.candidates`` does not flag."""
    ax = np.arange(int(g)) / float(oversample)
    out = np.ones((int(g), int(g)), dtype=bool)
    for kx, ky in known or ():
        out &= ~(np.hypot(ax[None, :] - float(kx), ax[:, None] - float(ky)) <= float(exclude_px))
    return out


def peaks(snr_map, threshold):
    """``detect.candidates``' rule as a mask: at or above ``threshold`` and larger than each of
    the (up to 8) lattice neighbours, a NaN neighbour counting as none."""
    s = np.asarray(snr_map, dtype=np.float64)
    g = s.shape[0]
    pad = np.full((g + 2, g + 2), -np.inf)
    pad[1:-1, 1:-1] = np.where(np.isnan(s), -np.inf, s)
    c = pad[1:-1, 1:-1]
    peak = (c >= threshold) & ~np.isnan(s)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                peak &= c > pad[1 + dy:g + 1 + dy, 1 + dx:g + 1 + dx]
    return peak


def _max_at(v, ok):
    """(max, flat index of its first occurrence) of v where ok; (NaN, -1) with none."""
    idx = np.flatnonzero(ok.ravel())
    if idx.size == 0:
        return float("nan"), -1
    at = int(idx[np.argmax(v.ravel()[idx])])
    return float(v.ravel()[at]), at


def map_stats(snr_map, known=None, exclude_px=0.0, centre=(0.0, 0.0), bin_px=1.0,
              threshold=5.0, oversample=1):
    """The stats kernel restated (comparisons only, so exact): the reductions of one snr map
    [g][g] as a dict of FIELDS; ``ring_max`` [largest ring + 1], NaN for a ring without a
    candidate that is a number."""
    s = np.asarray(snr_map, dtype=np.float64)
    g = s.shape[0]
    fin = ~np.isnan(s)
    out_ok = outside(g, known, exclude_px, oversample)
    ring = rings(g, centre, bin_px, oversample)
    pk = peaks(s, threshold)
    res = {}
    res["max_all"], res["argmax_all"] = _max_at(s, fin)
    res["max_out"], res["argmax_out"] = _max_at(s, fin & out_ok)
    res["peaks_all"], res["peaks_out"] = int(pk.sum()), int((pk & out_ok).sum())
    rm = np.full(int(ring.max()) + 1, np.nan)
    for k in np.unique(ring[fin]):
        rm[k] = s[fin & (ring == k)].max()
    res["ring_max"] = rm
    return res


# -- results: merging -----------------------------------------------------------------
def _stream_ids(ranges):
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([(int(s) + int(a) + np.arange(int(c), dtype=np.int64)) % 2 ** 32
                           for s, a, c in r] or [np.empty(0, np.int64)])


def merge_results(a, b):
    """a's realisations followed by b's (``DetectNull.results()`` dicts): concatenation.
    ValueError if the settings differ in any bit, if either holds explicit frames, or if a
    noise stream (seed + index mod 2^32) occurs in both."""
    for k in SETTINGS:
        if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes() \
                or np.asarray(a[k]).shape != np.asarray(b[k]).shape:
            raise ValueError(f"the results' settings differ: {k}")
    if a.get("frames") or b.get("frames"):
        raise ValueError("results of explicit frames carry no (seed, index) to tell them apart")
    ia, ib = _stream_ids(a["ranges"]), _stream_ids(b["ranges"])
    if np.intersect1d(ia, ib).size:
        raise ValueError("the (seed, index) ranges overlap: the same noise frames twice")
    out = {k: a[k] for k in SETTINGS}
    out["frames"] = False
    out["ranges"] = np.concatenate([np.asarray(x["ranges"], dtype=np.int64).reshape(-1, 3)
                                    for x in (a, b)])
    out["done"] = int(a["done"]) + int(b["done"])
    for k in FIELDS:
        out[k] = np.concatenate([np.asarray(a[k]), np.asarray(b[k])])
    return out


# -- the false-alarm probability ------------------------------------------------------
def _form(a, s):
    return -np.expm1(-a * s * np.exp(-0.5 * s * s))


def tail_fit(maxima, q=0.1):
    """Anchors FAP(s) = 1 - exp(-a s exp(-s^2 / 2)), the excursion probability of a 2-D
    Gaussian random field, at the empirical (1 - q) quantile s_q of the map maxima: a is chosen
    so that the form equals the empirical (1 + #{max >= s_q}) / (R + 1) there.  Returns
    ``{"a", "s_q", "p_q", "exceedances", "q", "R"}``; ValueError for fewer than 20 exceedances,
    a maximum that is NaN or an s_q <= 1 (the form decreases beyond 1 only)."""
    m = np.asarray(maxima, dtype=np.float64).ravel()
    if m.size == 0 or np.isnan(m).any():
        raise ValueError("the maxima must be numbers, at least one")
    if not 0.0 < q < 1.0:
        raise ValueError(f"q {q}: between 0 and 1")
    s_q = float(np.quantile(m, 1.0 - q))
    exc = int((m >= s_q).sum())
    if exc < 20:
        raise ValueError(f"{exc} maxima at or above the {1 - q:g} quantile: at least 20 are "
                         f"needed (run more realisations or raise q)")
    if s_q <= 1.0:
        raise ValueError(f"the {1 - q:g} quantile {s_q:g} is not beyond 1")
    p_q = (1.0 + exc) / (m.size + 1.0)
    a = -math.log1p(-p_q) / (s_q * math.exp(-0.5 * s_q * s_q))
    return {"a": a, "s_q": s_q, "p_q": p_q, "exceedances": exc, "q": float(q), "R": int(m.size)}


def fap(s, maxima, fit):
    """(the per-map false-alarm probability of a maximum >= s, "empirical" or
    "extrapolated"): up to s_q the empirical (1 + #{max >= s}) / (R + 1), beyond it the
    fitted form."""
    m = np.asarray(maxima, dtype=np.float64).ravel()
    s = float(s)
    if s <= fit["s_q"]:
        return (1.0 + float((m >= s).sum())) / (m.size + 1.0), "empirical"
    return float(_form(fit["a"], s)), "extrapolated"


def threshold_for(p, maxima, fit):
    """(the lowest s with fap(s) <= p, "empirical" or "extrapolated"): the inverse of
    ``fap``."""
    m = np.sort(np.asarray(maxima, dtype=np.float64).ravel())[::-1]
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError(f"p {p}: between 0 and 1")
    if p >= fit["p_q"]:
        # (1 + k) / (R + 1) <= p with k maxima at or above s: s just above the (k + 1)-th largest
        k = min(int(math.floor(p * (m.size + 1.0) - 1.0)), m.size - 1)
        return float(np.nextafter(m[k], np.inf)), "empirical"
    lo, hi = fit["s_q"], max(fit["s_q"], 1.0) + 1.0
    while _form(fit["a"], hi) > p:
        hi += 1.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if _form(fit["a"], mid) > p:
            lo = mid
        else:
            hi = mid
    return hi, "extrapolated"


def ring_thresholds(ring_max, p):
    """The empirical (1 - p) quantile of every ring's maximum over the realisations
    [R][nring] -> [nring]: the k with a per-ring false-alarm probability p.  NaN where
    R p < 10 (the quantile would rest on fewer than 10 maxima) and for a ring without
    candidates."""
    rm = np.asarray(ring_max, dtype=np.float64)
    out = np.full(rm.shape[1], np.nan)
    if rm.shape[0] * float(p) < 10.0:
        return out
    ok = ~np.isnan(rm).any(axis=0)
    if ok.any():
        out[ok] = np.quantile(rm[:, ok], 1.0 - float(p), axis=0)
    return out


def calibrated_curve(curve, sigma, ring_k, centre, flux0, bin_px=1.0, oversample=1):
    """``detect.contrast_curve`` with ring i's own k = ``ring_k[i]`` in place of a constant:
    ``curve`` (for its rings) plus ``k``, ``contrast_median_cal``, ``contrast_min_cal``,
    ``dmag_median_cal``, ``dmag_min_cal`` per ring of the curve; NaN where ring_k is."""
    sig = np.asarray(sigma, dtype=np.float64)
    ring = rings(sig.shape[0], centre, bin_px, oversample)
    ok = ~np.isnan(sig)
    ids = np.unique(ring[ok])
    if ids.size != len(curve["count"]):
        raise ValueError("the curve's rings are not this sigma map's")
    rk = np.asarray(ring_k, dtype=np.float64)
    k = np.array([rk[i] if i < rk.size else np.nan for i in ids])
    med = np.array([np.median(sig[ok & (ring == i)]) for i in ids]) * k / float(flux0)
    low = np.array([sig[ok & (ring == i)].min() for i in ids]) * k / float(flux0)
    return {**curve, "k": k, "contrast_median_cal": med, "contrast_min_cal": low,
            "dmag_median_cal": _dmag(med), "dmag_min_cal": _dmag(low)}


def summarise(res, threshold, p=0.01, q=0.1, cands=None):
    """The scalars step 3 prints and records, from a ``results()`` dict: quantiles of the map
    maximum (all candidates / outside the fitted sources), the mean number of false
    candidates per map, the per-map FAP at ``threshold`` and the threshold for FAP ``p`` (of
    the maxima outside the fitted sources, the ones a detection is claimed from), and one FAP
    per candidate of ``cands`` (flagged ones against the all-candidate maxima)."""
    out = {"realisations": int(res["done"]), "threshold": float(threshold), "p": float(p)}
    for key in ("all", "out"):
        m = np.asarray(res["max_" + key], dtype=np.float64)
        for name, qq in (("median", 0.5), ("q90", 0.9), ("q99", 0.99)):
            out[f"max_{key}_{name}"] = float(np.quantile(m, qq)) if m.size and not \
                np.isnan(m).any() else float("nan")
        out[f"false_per_map_{key}"] = float(np.mean(res["peaks_" + key])) if m.size else \
            float("nan")
    fits = {}
    for key in ("all", "out"):
        try:
            fits[key] = tail_fit(res["max_" + key], q)
        except ValueError:
            fits[key] = None
    f = fits["out"]
    if f is not None:
        out["fit_a"], out["fit_s_q"], out["fit_exceedances"] = f["a"], f["s_q"], f["exceedances"]
        out["fap_at_threshold"], out["fap_at_threshold_kind"] = fap(threshold, res["max_out"], f)
        out["threshold_for_p"], out["threshold_for_p_kind"] = threshold_for(p, res["max_out"], f)
    if cands is not None:
        out["candidate_fap"] = []
        for c in cands:
            key = "all" if c["flagged"] else "out"
            out["candidate_fap"].append(
                (None, "no fit") if fits[key] is None else fap(c["snr"], res["max_" + key],
                                                               fits[key]))
    return out


def table_lines(summ, cands=None, curve=None):
    """The lines step 3 prints after ``detect.table_lines``'."""
    s = summ
    lines = [f"{'null maps':>16} {s['realisations']} realisations"]
    for key, what in (("all", "all candidates"), ("out", "outside the fitted sources")):
        lines.append(f"{'map maximum':>16} median {s[f'max_{key}_median']:.3f}  90 % "
                     f"{s[f'max_{key}_q90']:.3f}  99 % {s[f'max_{key}_q99']:.3f}  ({what})")
    lines.append(f"{'false per map':>16} {s['false_per_map_all']:.4g} at or above "
                 f"{s['threshold']:g} ({s['false_per_map_out']:.4g} outside the fitted sources)")
    if "fap_at_threshold" in s:
        lines.append(f"{'per-map FAP':>16} {s['fap_at_threshold']:.3g} at {s['threshold']:g} "
                     f"({s['fap_at_threshold_kind']})")
        lines.append(f"{'threshold':>16} {s['threshold_for_p']:.3f} for a per-map FAP of "
                     f"{s['p']:g} ({s['threshold_for_p_kind']})")
    else:
        lines.append(f"{'per-map FAP':>16} n/a (too few realisations for the tail fit)")
    if cands:
        lines.append(f"{'candidate FAP':>16}")
        for c, (v, kind) in zip(cands, s.get("candidate_fap", [])):
            lines.append(f"{'':>4}{c['x']:9.2f}{c['y']:9.2f}{c['snr']:9.2f}  "
                         + (f"{v:.3g} ({kind})" if v is not None else "n/a"))
    if curve is not None and "k" in curve:
        lines.append(f"{'calibrated curve':>16} per-ring FAP {s['p']:g}")
        lines.append(f"{'':>4}{'sep_px':>9}{'sep_mas':>10}{'k':>8}{'median':>11}{'dmag':>8}")
        for i in range(len(curve["count"])):
            lines.append(f"{'':>4}{curve['sep_px'][i]:9.2f}{curve['sep_mas'][i]:10.2f}"
                         f"{curve['k'][i]:8.3f}{curve['contrast_median_cal'][i]:11.4g}"
                         f"{curve['dmag_median_cal'][i]:8.2f}")
    return lines


# -- the device object ----------------------------------------------------------------
class DetectNull(Handle):
    """One ``olpe_detect_null`` on ``detect``'s GPU: ``detect`` evaluated at ``vec``, its
    tables, Q plane and staged cutout copied; independent of ``detect`` afterwards.  ``scale``
    [g][g] multiplies the map (step 3 passes sigma_A(theta_hat) / sigma_total, the denominator
    of ``snr_marg``); ``known``: the fitted sources' (x, y) (default: those of ``vec``),
    ``exclude_px`` (default ``detect.default_exclude_px(vec)``), ``centre`` (default: the first
    known source), ``bin_px``: ``detect.candidates``' and ``detect.contrast_curve``'s.
    ``batch``: realisations per batch (default: from a byte budget); the results do not depend
    on it in any bit."""

    _destroy = "olpe_detect_null_destroy"

    def __init__(self, detect, vec, scale=None, known=None, exclude_px=None, centre=None,
                 bin_px=1.0, threshold=5.0, seed=0, batch=0):
        from . import detect as dt
        self.n, self.g, self.oversample = detect.n, detect.g, detect.oversample
        v = detect._vec(vec, "vector")
        if known is None:
            known = dt.known_of(v, detect.nsrc)
        if exclude_px is None:
            exclude_px = dt.default_exclude_px(v, detect.nsrc)
        if centre is None:
            centre = known[0] if len(known) else (0.0, 0.0)
        self.vec = v
        self.known = np.ascontiguousarray(known, dtype=np.float64).reshape(-1, 2)
        self.centre = np.ascontiguousarray(centre, dtype=np.float64).reshape(2)
        self.exclude_px, self.bin_px = float(exclude_px), float(bin_px)
        self.threshold, self.seed = float(threshold), int(seed)
        self.scale = None
        if scale is not None:
            self.scale = np.ascontiguousarray(scale, dtype=np.float64)
            if self.scale.shape != (self.g, self.g):
                raise ValueError(f"scale of shape {self.scale.shape}, expected {(self.g, self.g)}")
        if self.seed < 0:
            raise ValueError(f"seed {seed}: must be >= 0")
        self._ranges, self._frames = [], False
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.olpe_detect_null_create(
            detect._h, _pd(self.vec), None if self.scale is None else _pd(self.scale),
            _pd(self.known) if self.known.size else None, len(self.known), self.exclude_px,
            _pd(self.centre), self.bin_px, self.threshold, self.seed, int(batch), C.byref(h)))
        self._h = h

    def _done(self):
        done, nring = C.c_longlong(0), C.c_int(0)
        check(self._lib.olpe_detect_null_get(self._h, C.byref(done), C.byref(nring), None, None,
                                             None, None, None, None, None))
        return int(done.value), int(nring.value)

    def run(self, count):
        """``count`` more generated realisations, continuing at the index reached."""
        done, _ = self._done()
        check(self._lib.olpe_detect_null_run(self._h, int(count)))
        if count > 0:
            if self._ranges and self._ranges[-1][1] + self._ranges[-1][2] == done:
                self._ranges[-1][2] += int(count)
            else:
                self._ranges.append([self.seed, done, int(count)])

    def run_frames(self, eps):
        """Realisations of explicit noise frames eps [count][n][n] in place of the generator."""
        e = np.ascontiguousarray(eps, dtype=np.float64)
        if e.ndim != 3 or e.shape[1:] != (self.n, self.n):
            raise ValueError(f"frames of shape {e.shape}, expected [count][{self.n}][{self.n}]")
        check(self._lib.olpe_detect_null_run_frames(self._h, _pd(e), e.shape[0]))
        self._frames = self._frames or e.shape[0] > 0

    def results(self):
        """The per-realisation arrays by name (FIELDS; ``ring_max`` [done][nring]) with the
        settings, ``done`` and the (seed, first index, count) ``ranges`` ``merge_results``
        tells realisations apart by."""
        done, nring = self._done()
        d = {k: np.empty(done) for k in ("max_all", "max_out")}
        d.update({k: np.empty(done, dtype=np.int64)
                  for k in ("argmax_all", "argmax_out", "peaks_all", "peaks_out")})
        d["ring_max"] = np.empty((done, nring))
        pll = lambda a: a.ctypes.data_as(_lib._pll)   # noqa: E731
        check(self._lib.olpe_detect_null_get(
            self._h, None, None, _pd(d["max_all"]), pll(d["argmax_all"]), _pd(d["max_out"]),
            pll(d["argmax_out"]), pll(d["peaks_all"]), pll(d["peaks_out"]), _pd(d["ring_max"])))
        d.update(done=done, frames=self._frames,
                 ranges=np.array(self._ranges, dtype=np.int64).reshape(-1, 3),
                 g=np.int64(self.g), oversample=np.int64(self.oversample),
                 exclude_px=np.float64(self.exclude_px), bin_px=np.float64(self.bin_px),
                 threshold=np.float64(self.threshold), centre=self.centre.copy(),
                 known=self.known.copy(), vec=self.vec.copy(),
                 scale_id=np.int64(0 if self.scale is None else int.from_bytes(
                     hashlib.sha256(self.scale.tobytes()).digest()[:7], "little")))
        return d

    def maps(self, r0, count):
        """The snr maps [count][g][g] of generated realisations r0 .. r0 + count - 1,
        recomputed; the results so far are left as they are."""
        out = np.empty((int(count), self.g, self.g))
        check(self._lib.olpe_detect_null_maps(self._h, int(r0), int(count), _pd(out)))
        return out

    def noise(self, r0, count):
        """The noise frames eps [count][n][n] of generated realisations r0 .. r0 + count - 1."""
        out = np.empty((int(count), self.n, self.n))
        check(self._lib.olpe_detect_null_noise(self._h, int(r0), int(count), _pd(out)))
        return out

    def reset(self):
        check(self._lib.olpe_detect_null_reset(self._h))
        self._ranges, self._frames = [], False
