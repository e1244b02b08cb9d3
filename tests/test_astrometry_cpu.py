"""CPU checks of the astrometry feature: the header scalars (apf_step3.py:144-153,
:294-337), the output-line formatter (:517-546), the new entry points' argument
validation, their place in the header / library / ctypes table, and the NumPy restatement
(tests/astrom_restatement.py) against hand-computed cases for every branch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from astrom_restatement import restate2, restate3
from olpefit_amd import _lib
from olpefit_amd import astrometry as am

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["olpe_astrom_create", "olpe_astrom_destroy", "olpe_astrom_fold_ctx",
       "olpe_astrom_fold_rows", "olpe_astrom_rows", "olpe_astrom_finalize",
       "olpe_astrom_samples"]

HDR = {"PARANG": 12.5, "ROTPPOSN": 100.25, "INSTANGL": 0.7, "EL": 55.0, "AZ": 200.0,
       "ROTMODE": "position angle", "PARANTEL": -20.0, "EXPSTART": "10:00:01.5",
       "EXPSTOP": "10:01:31.5", "KOAID": "N2.20140101.00001.fits"}


@pytest.fixture(scope="module")
def lib():
    from olpefit_amd import build
    build.build(verbose=False)
    return _lib.load()


# --- from_header's scalar work --------------------------------------------------------
def test_header_scalars_pre_and_post():
    pre = am.header_scalars(HDR, "pre")
    post = am.header_scalars(HDR, "post")
    assert pre["pixscale"] == 9.952 and post["pixscale"] == 9.971          # :224, :231
    assert pre["rotation_angle"] == 12.5 + 100.25 - 55.0 - 0.7 - 0.252      # :300
    assert post["rotation_angle"] == 12.5 + 100.25 - 55.0 - 0.7 - 0.262     # :302
    for s in (pre, post):
        assert s["parantel"] == -20.0 and s["vertical_angle_mode"] == "no"
        assert s["use_rotcorr"] is False and s["rotcorr"] == 0.0
    assert am.prepost_of(2014) == "pre" and am.prepost_of(2015) == "post"   # :150
    assert am.epoch_of("/data/2016_05_12/N2.20160512.00001.LDIF.fits") == 2016
    with pytest.raises(ValueError):
        am.header_scalars(HDR, "Post")


def test_header_scalars_vertical_angle_mode():
    s = am.header_scalars({**HDR, "ROTMODE": "vertical angle"}, "post")
    # :314-334 by hand: 90 s exposure; d(eta)/dt = 0.262 * 0.941 * 0.940 / 0.574 = 0.403 rad/hr
    # = 0.00642 deg/s, times dt / 2 = 45 s: 0.289 deg
    etadot = -0.262 * np.cos(0.346036) * np.cos(np.radians(200.0)) / np.cos(np.radians(55.0))
    want = etadot * (180 / np.pi) / 3600 * 45.0
    assert s["use_rotcorr"] is True and s["vertical_angle_mode"] == "yes"
    assert s["rotcorr"] == pytest.approx(want, rel=1e-14) and 0.28 < s["rotcorr"] < 0.30
    assert s["rotation_angle"] == 12.5 + 100.25 - 55.0 - 0.7 - 0.262
    assert am.table_offsets((64, 64)) == (480, 480)                         # :241-242
    assert am.table_offsets((1024, 1023)) == (1, 0)


# --- the line formatter ---------------------------------------------------------------
def test_py2_str_is_python_2_str_of_a_float():
    assert am.py2_str(1732.123456789012345) == "1732.12345679"
    assert am.py2_str(5.0) == "5.0" and am.py2_str(-0.0) == "-0.0"
    assert am.py2_str(1e22) == "1e+22" and am.py2_str(1.5e-7) == "1.5e-07"
    assert am.py2_str(float("nan")) == "nan" and am.py2_str(float("inf")) == "inf"
    assert am.py2_str(np.float64(0.1) + 0.2) == "0.3"


def test_output_lines_have_the_reference_fields():
    r = {"sep_median": 1234.56789012345, "sep_std": 1.25, "pa_median": 287.123456789012,
         "pa_std": 0.5, "ra": -100.0, "ra_std": 2.0, "dec": 50.125, "dec_std": 3.0}
    line = am.pasep_line("N2.x.fits", [r], 1.0123456789012, 0.01)
    assert line == ("N2.x.fits , 1234.56789012 , 1.25 , 287.123456789 , 0.5 , nan , nan , nan , "
                    "nan , 1.0123456789 , 0.01")                             # :517-527
    assert am.radec_line("N2.x.fits", [r]) == "N2.x.fits , -100.0 , 2.0 , 50.125 , 3.0"
    three = am.pasep_line("K", [r, r], 1.0, 0.0, variant=3).split(" , ")     # 3body :575-590
    assert len(three) == 1 + 8 + 3 + 2 + 2 and three[9:14] == ["nan"] * 5
    assert len(am.radec_line("K", [r, r]).split(" , ")) == 9                 # 3body :601-609


# --- the C-ABI --------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "olpe.h")).read(),
                  flags=re.S)
    declared = set(re.findall(r"\b(olpe_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(olpe_\w+)", out))
    for name in NEW:
        assert name in declared and name in exported and name in _lib.SIGNATURES, name
    from olpefit_amd import build
    assert any(s.endswith("olpe_astrom.hip") for s in build.SOURCES)


def _create(lib, device=0, variant=2, ps=17, cols=(0, 1, 2, 3), npairs=1, xd=None, yd=None,
            ny=0, nx=0, pixscale=9.952, rot=0.0, rotcorr=0.0, use=0, walkers=4, cap=4, out=True):
    h = C.c_void_p()
    arr = (C.c_int * len(cols))(*cols) if cols is not None else None
    rc = lib.olpe_astrom_create(device, variant, ps, arr, npairs,
                                None if xd is None else xd.ctypes.data_as(_lib._pd),
                                None if yd is None else yd.ctypes.data_as(_lib._pd), ny, nx, 0, 0,
                                pixscale, rot, rotcorr, use, walkers, cap,
                                C.byref(h) if out else None)
    return rc, h


def test_create_validates_arguments_before_touching_a_gpu(lib):
    t = np.zeros((4, 4))
    bad = [dict(out=False), dict(device=-1), dict(variant=4), dict(npairs=2),
           dict(variant=3, npairs=1), dict(cols=None), dict(cols=(0, 1, 2, 17)),
           dict(cols=(0, 1, -1, 3)), dict(ps=3), dict(xd=t), dict(yd=t),
           dict(xd=t, yd=t, ny=0, nx=4), dict(pixscale=float("nan")),
           dict(rot=float("inf")), dict(rotcorr=float("nan"), use=1), dict(walkers=0),
           dict(cap=0), dict(walkers=1 << 30, cap=1 << 30)]
    for kw in bad:
        rc, h = _create(lib, **kw)
        assert rc == _lib.EINVAL and not h.value, kw
    assert b"walkers" in lib.olpe_last_error()
    n = C.c_int(0)
    lib.olpe_device_count(C.byref(n))
    if not n.value:                     # valid arguments fail only for lack of a GPU
        rc, h = _create(lib)
        assert rc == _lib.EHIP and not h.value


def test_null_arguments_are_errors(lib):
    out = np.zeros(16)
    pd = out.ctypes.data_as(_lib._pd)
    assert lib.olpe_astrom_fold_ctx(None, None) == _lib.EINVAL
    assert lib.olpe_astrom_fold_rows(None, pd, 1) == _lib.EINVAL
    assert lib.olpe_astrom_rows(None, None) == _lib.EINVAL
    assert lib.olpe_astrom_finalize(None, 0.0, 0.0, pd) == _lib.EINVAL
    assert lib.olpe_astrom_samples(None, 0, pd) == _lib.EINVAL
    lib.olpe_astrom_destroy(None)
    with pytest.raises(ValueError):
        am.Astrometry(4, 4, variant=4, pixscale=9.952, rotation_angle=0.0)
    with pytest.raises(ValueError):
        am.Astrometry(4, 4, pixscale=9.952, rotation_angle=0.0, x_dist=np.zeros((4, 4)))


# --- the restatement, by hand -------------------------------------------------------------
PIX = 9.952
R2 = np.sqrt(2.0)


def one(dx, dy, variant=2):
    """One sample: the primary at (9, 9), the companion dx, dy away (pair c: the same)."""
    c = np.zeros((1, 1, 17 if variant == 2 else 20))
    c[0, 0, :2] = 9.0
    c[0, 0, 2:4] = 9.0 + dx, 9.0 + dy
    if variant == 3:
        c[0, 0, 4:6] = 9.0 + dx, 9.0 + dy
    return c


def sc(rot=0.0, parantel=0.0, rotcorr=0.0, use=False):
    return {"pixscale": PIX, "rotation_angle": rot, "rotcorr": rotcorr, "use_rotcorr": use,
            "parantel": parantel}


def near(a, b):
    return abs(float(a) - b) <= 1e-12 * max(1.0, abs(b))


# geometric PA = atan2(-dx, dy): (-10, 10) -> 45, (-10, -10) -> 135, (10, -10) -> -135
@pytest.mark.parametrize("variant,dx,dy,rot,par,branch,added,pa_out", [
    (2, 10, 10, 0.0, 0.0, 2, True, 315.0),      # mean -45 < 0: + 360 (:340); pop 315: + 360
    (2, -10, -10, 0.0, 0.0, 0, False, 135.0),   # below, mean >= 90: atan(tan 135) = -45, + 180
    (2, -10, 10, 0.0, -60.0, 1, False, 45.0),   # below (pop 105), mean < 90: + 0
    (2, -10, 10, 0.0, 0.0, 4, False, 45.0),     # plain above
    (2, 10, -10, 360.0, -60.0, 2, False, 405.0),  # pa 225, pop 285: :425 tests pop twice
    (2, -10, 10, 240.0, 0.0, 2, False, 285.0),  # pa 285, pop 285: atan(tan 285) = -75, + 360
    (3, 10, 10, 0.0, 0.0, 2, False, 315.0),     # % 360 (3body :334): 315, never negative
    (3, 10, -10, 0.0, -60.0, 3, False, 225.0),  # pop 285, mean 225 < 270: + 180 (3body :483)
    (3, -10, -10, 0.0, 0.0, 5, False, 135.0),   # below: -45 < 0 -> + 180 per sample
    (3, -10, 10, 0.0, -60.0, 5, False, 45.0),   # below, 45 >= 0: nothing added
    (3, -10, 10, 0.0, 0.0, 4, False, 45.0),
])
def test_restatement_branches_by_hand(variant, dx, dy, rot, par, branch, added, pa_out):
    f = restate2 if variant == 2 else restate3
    for r in f(one(dx, dy, variant), sc(rot, par)):
        assert r["branch_code"] == branch and r["added_360"] == added
        sep = 10 * R2 * PIX
        assert near(r["sep_median"], sep) and near(r["pa_median"], pa_out)
        assert r["sep_std"] == 0 and r["pa_std"] == 0
        a = np.radians(pa_out)
        if variant == 2:                                    # :446-450
            assert near(r["ra"], -sep * np.cos(a)) and near(r["dec"], sep * np.sin(a))
        else:                                               # 3body :508-512
            assert near(r["ra"], sep * np.sin(a)) and near(r["dec"], sep * np.cos(a))


def test_restatement_refraction_and_rotcorr_by_hand():
    # pa 45, parantel 0, above: deltasep = dR cos 45, deltapa = dR sin 45, pa_mas = sep tan 45
    # = sep: both legs grow by dR / sqrt 2, the angle stays 45 and sep grows by dR / sqrt 2
    r, = restate2(one(-10, 10), sc(), deltaR=7.0)
    assert near(r["sep_median"], 10 * R2 * PIX + 7.0 / R2) and near(r["pa_median"], 45.0)
    # variant 3 multiplies tan by sep_corrected (3body :477): the angle moves
    r3 = restate3(one(-10, 10, 3), sc(), deltaR=7.0)[1]
    s, sc3 = 10 * R2 * PIX, 10 * R2 * PIX + 7.0 / R2
    assert near(r3["sep_median"], sc3)
    assert near(r3["pa_median"], np.degrees(np.arctan((sc3 + 7.0 / R2) / sc3)))
    # below (pa 135, parantel 0): the angle of the correction is 180 - 135 = 45
    r, = restate2(one(-10, -10), sc(), deltaR=7.0)
    assert near(r["sep_median"], s + 7.0 / R2)
    assert near(r["pa_median"], np.degrees(np.arctan((-s + 7.0 / R2) / (s + 7.0 / R2))) + 180.)
    # rotcorr is added only in vertical-angle mode (:309, :337)
    assert near(restate2(one(-10, 10), sc(1.0, rotcorr=0.5, use=True))[0]["pa_median"], 46.5)
    assert near(restate2(one(-10, 10), sc(1.0, rotcorr=0.5, use=False))[0]["pa_median"], 46.0)


def test_restatement_distortion_lookup_by_hand():
    # x_dist[y, x] = 0.001 x, y_dist = 0.01 y, offsets 100: star (9, 9) + 1 -> index 110,
    # companion (3.2, 15.7) + 1 -> int 4, 16 -> index 104, 116 (:234-253)
    y, x = np.mgrid[:256, :256].astype(float)
    r, = restate2(one(-5.8, 6.7), sc(), 0.001 * x, 0.01 * y, 100, 100)
    xs, ys = 10 + 0.110, 10 + 1.10
    xc, yc = 4.2 + 0.104, 16.7 + 1.16
    assert np.allclose(r["position_means"], [xs, ys, xc, yc], rtol=1e-14)
    assert near(r["sep_median"], np.hypot(xc - xs, yc - ys) * PIX)
    assert near(r["pa_median"], np.degrees(np.arctan2(-(xc - xs), yc - ys)))
    # the median of an even count is the mean of the middle pair (np.median)
    c = np.concatenate([one(-10, 10), one(-10, 10.5)], axis=0)
    r, = restate2(c, sc())
    seps = [10 * R2 * PIX, np.hypot(10, 10.5) * PIX]
    assert near(r["sep_median"], np.mean(seps)) and near(r["sep_std"], np.std(seps))
