"""Separation / position-angle posteriors on the device (include/olpe.h, olpe_astrom_*).

What step 3 is run for (apf_step3.py:211-256, :283-343, :401-450; 3-source:
3body/apf_step3_3body.py:247-288, :315-390, :450-518): every chain row becomes a
(separation, position angle) sample, corrected for distortion, detector rotation and
differential refraction, and the run is summarised by the samples' medians and scatter and
by delta RA / Dec.  ``Astrometry`` keeps the samples on the GPU and reduces them there;
the host does the reference's scalar work only (``from_header``).

Not covered: computing ``deltaR`` itself (the name resolver, the AltAz transform and
``atm_corr``, apf_step3.py:348-391: pass it as ``delta_r``), medians over several objects
and the plots.  The photometry fields of the output lines are ``photometry.py``'s
(``pasep_line(photometry=...)``; ``nan`` without).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._handle import Handle, _pd
from ._lib import check

OUT_LEN = 16
BRANCHES = {0: "below+180", 1: "below", 2: "above+360", 3: "above+180", 4: "above",
            5: "below, +180 per negative sample"}
#: the pairs' columns {x, y of the primary, x, y of the companion} in the chain rows
PAIR_COLS = {2: [[0, 1, 2, 3]], 3: [[0, 1, 2, 3], [0, 1, 4, 5]]}
PAIR_NAMES = {2: [""], 3: ["b", "c"]}


def prepost_of(epoch: int) -> str:
    """apf_step3.py:149-153: the distortion solution by the epoch (the year the image's
    directory name starts with)."""
    return "post" if int(epoch) >= 2015 else "pre"


def epoch_of(image_path: str) -> int:
    """apf_step3.py:149: ``int(d[-2].split('_')[0])`` of the image path."""
    return int(image_path.split('/')[-2].split('_')[0])


def _get_sec(time_str):                     # apf_step3.py:318-320
    h, m, s = time_str.split(':')
    return float(h) * 3600 + float(m) * 60 + float(s)


PIXSCALE = {"pre": 9.952, "post": 9.971}    # mas / px, apf_step3.py:224, :231


def header_scalars(hdr, prepost: str) -> dict:
    """The host-side scalar work of apf_step3.py:218-231 and :294-337 (3body :336-380) and
    PARANTEL (:393): pixscale, rotation_angle, the vertical-angle-mode correction."""
    if prepost not in ("pre", "post"):
        raise ValueError("prepost must be 'pre' or 'post'")
    p, r, i, e = hdr['PARANG'], hdr['ROTPPOSN'], hdr['INSTANGL'], hdr['EL']
    if prepost == "pre":
        pixscale = PIXSCALE["pre"]                    # :224
        rotation_angle = p + r - e - i - 0.252        # :300, Yelda 2010
    else:
        pixscale = PIXSCALE["post"]                   # :231
        rotation_angle = p + r - e - i - 0.262        # :302, Service 2016
    out = {"prepost": prepost, "pixscale": pixscale, "rotation_angle": float(rotation_angle),
           "vertical_angle_mode": "no", "rotcorr": 0.0, "use_rotcorr": False,
           "parantel": float(hdr['PARANTEL'])}
    if hdr['ROTMODE'] == 'vertical angle':            # :309
        dt = _get_sec(hdr['EXPSTOP']) - _get_sec(hdr['EXPSTART'])
        az = hdr['AZ'] * (np.pi / 180)
        el = hdr['EL'] * (np.pi / 180)
        L = 0.346036
        etadot = (-0.262) * np.cos(L) * np.cos(az) / np.cos(el)
        etadot = etadot * (180 / np.pi) / 3600
        out.update(vertical_angle_mode="yes", rotcorr=float(etadot * (dt / 2)),
                   use_rotcorr=True)
    return out


def table_offsets(image_shape) -> tuple[int, int]:
    """apf_step3.py:241-242: (xdiff, ydiff)."""
    return (int(np.ceil(0.5 * (1024 - image_shape[1]))),
            int(np.ceil(0.5 * (1024 - image_shape[0]))))


def py2_str(x) -> str:
    """Python 2's ``str(float)``, which the reference's output lines use: 12 significant
    digits (``%.12g``), and ``.0`` after a value that would read as an integer."""
    x = float(x)
    s = "%.12g" % x
    if math.isfinite(x) and "." not in s and "e" not in s:
        s += ".0"
    return s


def pasep_line(koaid, results, rc_mean, rc_std, variant: int = 2, photometry=None) -> str:
    """The ``epoch_grand_pasep`` line (apf_step3.py:517-527; 3body :575-590) without its
    newline.  ``photometry`` carries the S/N and FWHM fields (:522-525; 3body :584-588) as
    ``photometry.reference_numbers`` returns them: ``snr`` (the primary's first, one per
    source), ``fwhm_mean``, ``fwhm_std``; without it they are ``nan``."""
    nan = float("nan")
    nsnr = 2 if variant == 2 else 3
    f = [str(koaid)]
    for r in results:
        f += [py2_str(r["sep_median"]), py2_str(r["sep_std"]), py2_str(r["pa_median"]),
              py2_str(r["pa_std"])]
    if photometry is None:
        snr, fwhm = [nan] * nsnr, [nan, nan]
    else:
        snr = list(photometry["snr"])
        fwhm = [photometry["fwhm_mean"], photometry["fwhm_std"]]
        if len(snr) != nsnr:
            raise ValueError(f"{len(snr)} S/N values for {nsnr} sources")
    f += [py2_str(v) for v in snr]                          # star / companion S/N
    f += [py2_str(v) for v in fwhm]                         # FWHM mean, std
    f += [py2_str(rc_mean), py2_str(rc_std)]
    return " , ".join(f)


def radec_line(koaid, results) -> str:
    """The ``epoch_grand_radec`` line (apf_step3.py:538-542; 3body :601-609)."""
    f = [str(koaid)]
    for r in results:
        f += [py2_str(r["ra"]), py2_str(r["ra_std"]), py2_str(r["dec"]), py2_str(r["dec_std"])]
    return " , ".join(f)


class Astrometry(Handle):
    """One ``olpe_astrom``: the (sep, pa) samples of up to ``row_capacity`` rows of
    ``walkers`` walkers on one GPU."""

    _destroy = "olpe_astrom_destroy"

    def __init__(self, walkers: int, row_capacity: int, *, variant: int = 2, ps: int | None = None,
                 pixscale: float, rotation_angle: float, rotcorr: float = 0.0,
                 use_rotcorr: bool = False, parantel: float = 0.0, x_dist=None, y_dist=None,
                 xdiff: int = 0, ydiff: int = 0, pair_cols=None, device: int = 0):
        if variant not in (2, 3):
            raise ValueError("variant must be 2 or 3")
        lib = _lib.load()
        self.variant = variant
        self.ps = int(ps) if ps is not None else (17 if variant == 2 else 20)
        cols = np.ascontiguousarray(PAIR_COLS[variant] if pair_cols is None else pair_cols,
                                    dtype=np.int32).reshape(-1, 4)
        self.npairs = int(cols.shape[0])
        if (x_dist is None) != (y_dist is None):
            raise ValueError("give both distortion tables or neither")
        self.distortion = x_dist is not None
        xd = yd = None
        ny = nx = 0
        if self.distortion:
            xd = np.ascontiguousarray(x_dist, dtype=np.float64)
            yd = np.ascontiguousarray(y_dist, dtype=np.float64)
            if xd.ndim != 2 or xd.shape != yd.shape:
                raise ValueError("distortion tables must be 2-D and of one shape")
            ny, nx = xd.shape
        self.W, self.capacity = int(walkers), int(row_capacity)
        self.parantel = float(parantel)
        self._lib = lib
        h = C.c_void_p()
        check(lib.olpe_astrom_create(
            int(device), variant, self.ps, cols.ctypes.data_as(C.POINTER(C.c_int)), self.npairs,
            None if xd is None else _pd(xd), None if yd is None else _pd(yd), ny, nx,
            int(xdiff), int(ydiff),
            float(pixscale), float(rotation_angle), float(rotcorr), int(bool(use_rotcorr)),
            self.W, self.capacity, C.byref(h)))
        self._h = h

    @classmethod
    def from_header(cls, hdr, walkers: int, row_capacity: int, *, prepost: str | None = None,
                    epoch: int | None = None, variant: int = 2, image_shape=None, x_dist=None,
                    y_dist=None, device: int = 0):
        """From a NIRC2 header (apf_step3.py:144-153, :294-337, :393).  ``epoch`` (the
        year) or ``prepost`` selects the solution; ``image_shape`` gives the table offsets
        of :241-242 (needed with tables)."""
        if prepost is None:
            if epoch is None:
                raise ValueError("give epoch or prepost")
            prepost = prepost_of(epoch)
        s = header_scalars(hdr, prepost)
        xdiff = ydiff = 0
        if x_dist is not None:
            if image_shape is None:
                raise ValueError("image_shape is needed with distortion tables")
            xdiff, ydiff = table_offsets(image_shape)
        a = cls(walkers, row_capacity, variant=variant, pixscale=s["pixscale"],
                rotation_angle=s["rotation_angle"], rotcorr=s["rotcorr"],
                use_rotcorr=s["use_rotcorr"], parantel=s["parantel"], x_dist=x_dist,
                y_dist=y_dist, xdiff=xdiff, ydiff=ydiff, device=device)
        a.scalars = s
        return a

    @property
    def rows(self) -> int:
        n = C.c_longlong(0)
        check(self._lib.olpe_astrom_rows(self._h, C.byref(n)))
        return int(n.value)

    def fold(self, sampler):
        """Fold the rows of the sampler's last launch from its device chain (once per
        launch; no host copy)."""
        check(self._lib.olpe_astrom_fold_ctx(self._h, sampler._ctx))

    def fold_rows(self, chains):
        """Fold host rows [rows, walkers, PS] (``step3.load_chains``)."""
        c = np.ascontiguousarray(chains, dtype=np.float64)
        if c.ndim != 3 or c.shape[1] != self.W or c.shape[2] != self.ps:
            raise ValueError(f"rows of shape {c.shape}, expected (rows, {self.W}, {self.ps})")
        check(self._lib.olpe_astrom_fold_rows(self._h, _pd(c), c.shape[0]))

    def finalize(self, delta_r: float = 0.0, parantel: float | None = None):
        """The reference's summary per pair (a list of dicts, one per pair)."""
        out = np.zeros((self.npairs, OUT_LEN))
        par = self.parantel if parantel is None else float(parantel)
        check(self._lib.olpe_astrom_finalize(self._h, float(delta_r), par, _pd(out)))
        res = []
        for p in range(self.npairs):
            o = out[p]
            res.append({"pair": PAIR_NAMES.get(self.variant, [""] * self.npairs)[p],
                        "sep_median": float(o[0]), "sep_std": float(o[1]),
                        "pa_median": float(o[2]), "pa_std": float(o[3]),
                        "ra": float(o[4]), "ra_std": float(o[5]),
                        "dec": float(o[6]), "dec_std": float(o[7]),
                        "pa_mean_uncorrected": float(o[8]), "branch": BRANCHES[int(o[9])],
                        "branch_code": int(o[9]), "samples": int(o[10]),
                        "added_360": bool(o[11]),
                        "position_means": [float(v) for v in o[12:16]]})
        self._n = int(out[0, 10])
        return res

    def samples(self, pair: int = 0):
        """After finalize: the device's (sep_corrected, pa_angle), each [rows, walkers]."""
        rows = self.rows
        out = np.empty((2, rows, self.W))
        check(self._lib.olpe_astrom_samples(self._h, int(pair), _pd(out)))
        return out[0], out[1]
