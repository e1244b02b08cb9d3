"""Photometry posteriors on the device (include/olpe.h, olpe_phot_*) and the reference's
aperture S/N and FWHM numbers on the host.

What step 3 is run for besides the position: how bright the companion is relative to the
star.  In ``build_analytical_model`` (apf_step2.py:78-124; 3-source: 3body/apf_step2_3body.py
:78-125) every source shares ``ampratio`` q, the four widths, both angles and the amplitude
offset b, so source k integrates to ``F_k = 2 pi (A_k - b) [(1 - q) sx sy + q sx2 sy2]`` and
the flux ratio of companion k to the primary is exactly ``(A_k - b) / (A_0 - b)``.
``Photometry`` turns every chain row into ``flux_ratio``, ``dmag``, ``flux_primary``,
``fwhm_major``, ``fwhm_minor``, ``fwhm_wide_major`` and ``core_fraction`` samples on the GPU
and reduces them there (count, mean, np.std, extremes, exact order statistics).

The reference's own photometry block (apf_step3.py:452-511; 3body :520-569) is per image,
not per sample, and stays on the host, NumPy only: ``reference_fwhm`` (what :454-470
compute, read literally), ``circle_overlap`` and ``aperture_snr`` (:476-511 without
photutils: the exact circle-pixel overlap is plain geometry).

Not covered: refraction, magnitudes on a photometric system, a checkpoint of the sample
store, ``--photometry`` in step 2, an RCCL merge, plots.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib
from ._handle import Handle, _pd
from ._lib import check

#: the planes, in the library's order
PLANES = {2: ["flux_ratio", "dmag", "flux_primary", "fwhm_major", "fwhm_minor",
              "fwhm_wide_major", "core_fraction"],
          3: ["flux_ratio_b", "dmag_b", "flux_ratio_c", "dmag_c", "flux_primary", "fwhm_major",
              "fwhm_minor", "fwhm_wide_major", "core_fraction"]}
#: the chain columns of the sources' x, y (apf_step3.py:174-186; 3body :196-217) and of sigmax
XY_COLS = {2: [(0, 1), (2, 3)], 3: [(0, 1), (2, 3), (4, 5)]}
SIGMAX_COL = {2: 10, 3: 13}
DEFAULT_PROBS = (0.16, 0.5, 0.84)


def out_len(nprobs: int) -> int:
    """OLPE_PHOT_LEN(nprobs)."""
    return 6 + 2 * int(nprobs)


def interpolate(lo, hi, n, p):
    """``np.percentile``'s linear rule between the order statistics ``floor((n - 1) p)`` and
    ``ceil((n - 1) p)`` of n samples: the virtual index ``(n - 1) p``, its fraction t, and
    ``lo + (hi - lo) t`` (``hi - (hi - lo) (1 - t)`` from t = 0.5 on), NumPy's ``_lerp``."""
    if n < 1:
        return float("nan")
    vi = np.float64(n - 1) * np.float64(p)
    t = vi - np.floor(vi)
    lo, hi = np.float64(lo), np.float64(hi)
    with np.errstate(invalid="ignore"):
        d = hi - lo
        return float(hi - d * (1 - t) if t >= 0.5 else lo + d * t)


class Photometry(Handle):
    """One ``olpe_phot``: the photometric samples of up to ``row_capacity`` rows of
    ``walkers`` walkers on one GPU (``PLANES[variant]``, each [rows, walkers])."""

    _destroy = "olpe_phot_destroy"

    def __init__(self, walkers: int, row_capacity: int, *, variant: int = 2, pixscale: float,
                 ps: int | None = None, device: int = 0):
        if variant not in (2, 3):
            raise ValueError("variant must be 2 or 3")
        lib = _lib.load()
        self.variant = variant
        self.ps = int(ps) if ps is not None else (17 if variant == 2 else 20)
        self.planes = list(PLANES[variant])
        self.W, self.capacity = int(walkers), int(row_capacity)
        self.pixscale = float(pixscale)
        self._lib = lib
        h = C.c_void_p()
        check(lib.olpe_phot_create(int(device), variant, self.ps, self.pixscale, self.W,
                                   self.capacity, C.byref(h)))
        self._h = h

    @property
    def rows(self) -> int:
        n = C.c_longlong(0)
        check(self._lib.olpe_phot_rows(self._h, C.byref(n)))
        return int(n.value)

    @property
    def unusable(self) -> int:
        """Rows that stored NaN in every plane (non-finite column, A_0 - b <= 0, width <= 0)."""
        n = C.c_longlong(0)
        check(self._lib.olpe_phot_unusable(self._h, C.byref(n)))
        return int(n.value)

    def fold(self, sampler, row_step: int = 1):
        """Fold every ``row_step``-th row of the sampler's last launch from its device chain
        (once per launch; no host copy)."""
        check(self._lib.olpe_phot_fold_ctx(self._h, sampler._ctx, int(row_step)))

    def fold_rows(self, chains):
        """Fold host rows [rows, walkers, PS] (``step3.load_chains``)."""
        c = np.ascontiguousarray(chains, dtype=np.float64)
        if c.ndim != 3 or c.shape[1] != self.W or c.shape[2] != self.ps:
            raise ValueError(f"rows of shape {c.shape}, expected (rows, {self.W}, {self.ps})")
        check(self._lib.olpe_phot_fold_rows(self._h, _pd(c), c.shape[0]))

    def reset(self):
        check(self._lib.olpe_phot_reset(self._h))

    def finalize(self, probs=DEFAULT_PROBS):
        """Per plane a dict: n (the samples that are not NaN), mean, std, min, max,
        ``percentiles`` (one per probability, interpolated as ``np.percentile`` does from the
        device's two order statistics, kept as ``brackets``) and the select's ``passes``."""
        p = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        out = np.zeros((len(self.planes), out_len(p.size)))
        check(self._lib.olpe_phot_finalize(self._h, _pd(p), int(p.size), _pd(out)))
        res = {}
        for name, o in zip(self.planes, out):
            n = int(o[0])
            br = [(float(o[6 + 2 * j]), float(o[7 + 2 * j])) for j in range(p.size)]
            res[name] = {"n": n, "mean": float(o[1]), "std": float(o[2]), "min": float(o[3]),
                         "max": float(o[4]), "passes": int(o[5]), "probs": [float(v) for v in p],
                         "brackets": br,
                         "percentiles": [interpolate(lo, hi, n, q) for (lo, hi), q in zip(br, p)]}
        return res

    def samples(self, plane):
        """One plane's samples [rows, walkers] (by name or index)."""
        k = self.planes.index(plane) if isinstance(plane, str) else int(plane)
        out = np.empty((self.rows, self.W))
        check(self._lib.olpe_phot_samples(self._h, k, _pd(out)))
        return out


def _quadrant(x, y, r):
    """The area of the disc of radius r about the origin inside [0, x] x [0, y], x, y >= 0."""
    x, y = np.minimum(x, r), np.minimum(y, r)
    inside = x * x + y * y <= r * r
    # the chord at height y ends at xa; left of it the column is full, right of it it
    # reaches the circle: G(t) = (t s + r^2 atan2(t, s)) / 2 with s = sqrt((r - t)(r + t))
    xa = np.sqrt((r - y) * (r + y))

    def G(t):
        s = np.sqrt((r - t) * (r + t))
        return 0.5 * (t * s + r * r * np.arctan2(t, s))
    return np.where(inside, x * y, xa * y + (G(x) - G(np.minimum(xa, x))))


def _anchored(x, y, r):
    """The signed area of the disc inside the rectangle spanned by the origin and (x, y)."""
    return np.sign(x) * np.sign(y) * _quadrant(np.abs(x), np.abs(y), r)


def circle_overlap(ny: int, nx: int, x0: float, y0: float, r: float):
    """The exact area of each pixel of an [ny, nx] grid inside the circle of radius r about
    (x0, y0) (x along the second axis).  Pixel (j, i) covers [i - 1/2, i + 1/2] x [j - 1/2,
    j + 1/2]: photutils' convention and its ``method='exact'``, the default the reference's
    ``do_photometry`` calls use (apf_step3.py:483-488).  A pixel wholly inside the circle is
    exactly 1, one wholly outside exactly 0."""
    r = float(r)
    xl = np.arange(nx, dtype=np.float64)[None, :] - 0.5 - float(x0)
    yl = np.arange(ny, dtype=np.float64)[:, None] - 0.5 - float(y0)
    xh, yh = xl + 1.0, yl + 1.0

    def box(xl, xh, yl, yh):      # (A - B) - (C - D): the same bits for a mirrored pixel
        return ((_anchored(xh, yh, r) - _anchored(xl, yh, r))
                - (_anchored(xh, yl, r) - _anchored(xl, yl, r)))
    # the mean of the form and its transpose, so that a transposed pixel has the same bits
    a = 0.5 * (box(xl, xh, yl, yh) + box(yl, yh, xl, xh))
    far2 = np.maximum(np.abs(xl), np.abs(xh)) ** 2 + np.maximum(np.abs(yl), np.abs(yh)) ** 2
    nearx = np.where((xl <= 0) & (xh >= 0), 0.0, np.minimum(np.abs(xl), np.abs(xh)))
    neary = np.where((yl <= 0) & (yh >= 0), 0.0, np.minimum(np.abs(yl), np.abs(yh)))
    a = np.clip(a, 0.0, 1.0)
    a = np.where(far2 <= r * r, 1.0, a)
    return np.where(nearx ** 2 + neary ** 2 >= r * r, 0.0, a)


def aperture_snr(image, x, y, radius=5, r_in=11, r_out=14, parts: bool = False):
    """apf_step3.py:482-495 (:498-511; 3body :550-565) for one source at the integer
    position (x, y) of :476-477: a circular aperture and a sky annulus at (x - 1, y - 1),
    summed with the exact overlap and clipped to the image, ``signal = apsum - ap.area *
    skysum / annulus.area`` with the analytic areas, and the noise ``np.std`` of the box
    ``image[y+12:y+27, x+12:x+27]`` times ``sqrt(ap.area)``.  NumPy slicing applies to the
    box: a truncated one is used as it is, an empty one gives ``nan``.  ``parts=True``
    returns (snr, signal, noise)."""
    image = np.asarray(image, dtype=np.float64)
    x, y = int(x), int(y)
    ny, nx = image.shape
    ap_area = np.pi * radius ** 2
    an_area = np.pi * (r_out ** 2 - r_in ** 2)
    apsum = np.sum(image * circle_overlap(ny, nx, x - 1, y - 1, radius))
    skysum = np.sum(image * (circle_overlap(ny, nx, x - 1, y - 1, r_out)
                             - circle_overlap(ny, nx, x - 1, y - 1, r_in)))
    signal = apsum - ap_area * (skysum / an_area)
    box = image[y + 12:y + 12 + 15, x + 12:x + 12 + 15]
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        noise = np.std(box) * np.sqrt(ap_area)
        snr = signal / noise
    return (float(snr), float(signal), float(noise)) if parts else float(snr)


def reference_fwhm(sigmax, pixscale):
    """apf_step3.py:454-470 (3body :522-538) read literally, for ``sigmax`` [rows, walkers]
    after the additional burn-in: ``sigy`` is overwritten on every iteration of :460-461 and
    ends as ``sigx`` plus one row, so :464 pairs ``sigx`` with itself and ``sigmay`` never
    enters.  (FWHMmean, FWHMstd) of ``2.355 * sigmax[i] * pixscale`` over i in
    ``arange(len - 100, len)``, all walkers: negative indices wrap as NumPy indexing does,
    and below 50 rows the reference's ``sigmax[i]`` raises ``IndexError``, as this does."""
    sigmax = np.asarray(sigmax, dtype=np.float64)
    n = len(sigmax)
    sigx = sigmax[np.arange(n - 100, n)].ravel()           # :458-459
    fwhm = 2.355 * sigx * pixscale                          # :469
    return float(np.mean(fwhm)), float(np.std(fwhm))


def source_positions(chains, variant: int = 2):
    """apf_step3.py:476-477 (3body :543-545) after the + 1 of :211-214: the integer means
    ``np.int_(np.mean(x + 1))`` of every source's x and y columns of [rows, walkers, PS]
    chains, primary first."""
    with np.errstate(invalid="ignore"):
        return [(int(np.int_(np.mean(chains[:, :, cx] + 1))),
                 int(np.int_(np.mean(chains[:, :, cy] + 1)))) for cx, cy in XY_COLS[variant]]


def reference_numbers(image, chains, pixscale, variant: int = 2) -> dict:
    """The pasep line's photometry fields (apf_step3.py:522-525; 3body :584-588) from the
    image and [rows, walkers, PS] chains after the burn-in: the sources' S/N, primary first
    (``starsnr``, ``compsnr``; 3body ``snra``, ``snrb``, ``snrc``), FWHMmean and FWHMstd."""
    pos = source_positions(chains, variant)
    mean, std = reference_fwhm(chains[:, :, SIGMAX_COL[variant]], pixscale)
    return {"positions": [list(p) for p in pos],
            "snr": [aperture_snr(image, x, y) for x, y in pos],
            "fwhm_mean": mean, "fwhm_std": std}
