"""Separation / position-angle posteriors on the GPU (olpe_astrom_*, olpefit_amd/astrometry.py)
against the NumPy restatement of the reference's lines (tests/astrom_restatement.py).

* Medians: the device's medians equal ``np.median`` of the device's own samples bit for
  bit (the radix select is exact, whatever libm does).
* Per-sample parity: the largest deviations measured on this file's inputs were
  6.78e-16 relative for ``sep_corrected`` and 1.71e-13 deg for ``pa_angle`` (device libm's
  atan2 / tan / atan / sin / cos against the host's); the bounds are 8x
  those.  Both are far inside the 1e-11 at which the operation order would be in doubt.
* Summary numbers: a median moves by no more than its samples do; np.std and np.mean are
  1-Lipschitz in the largest per-sample deviation, and the two summation orders (NumPy's
  pairwise sum, the device's fixed tree) differ by at most n * 2^-53 relative to the
  largest term -- so the bound is the per-sample one plus that.
* Fold splitting, device fold against host fold: bit-identical.
"""
import json
import os

import numpy as np
import pytest

import fold_scale_cases as fc
from astrom_restatement import RESTATE
from olpefit_amd import _lib, fitsio, step2, step3, synth
from olpefit_amd.astrometry import Astrometry, header_scalars, py2_str

pytestmark = pytest.mark.gpu

SEP_RTOL = 8 * 6.78e-16       # 8 x the measured largest deviation (see the docstring)
PA_ATOL = 8 * 1.71e-13        # deg
PIXSCALE = 9.952
N_IMG = 64                   # cutout side: table offsets 480


def tables():
    """A smooth synthetic 1024 x 1024 distortion pair (a few tenths of a pixel)."""
    y, x = np.mgrid[:1024, :1024].astype(np.float64)
    xd = 0.3 * np.sin(2 * np.pi * y / 1024.) * np.cos(2 * np.pi * x / 700.) + 1e-4 * x
    yd = 0.25 * np.cos(2 * np.pi * y / 900.) * np.sin(2 * np.pi * x / 1024.) - 2e-4 * y
    return xd, yd


XD, YD = tables()
XDIFF = YDIFF = int(np.ceil(0.5 * (1024 - N_IMG)))


def make_chain(walkers, rows, variant, seed=0, repeat=1, pa0=30.0, scatter=0.05):
    """[rows * repeat, walkers, PS]: the primary near (30, 32), the companion(s) 10 px
    away at geometric position angle pa0 (and pa0 + 25 for variant 3's second pair), each
    row repeated ``repeat`` times (a rejected proposal repeats the row)."""
    ps = 17 if variant == 2 else 20
    rng = np.random.RandomState(seed)
    c = rng.normal(0.0, 1.0, size=(rows, walkers, ps)) * 3.0 + 50.0
    c[:, :, 0] = 30.0 + scatter * rng.normal(size=(rows, walkers))
    c[:, :, 1] = 32.0 + scatter * rng.normal(size=(rows, walkers))
    for k, ang in ((2, pa0), (4, pa0 + 25.0))[:variant - 1]:
        a = np.radians(ang)
        c[:, :, k] = 30.0 - 10.0 * np.sin(a) + scatter * rng.normal(size=(rows, walkers))
        c[:, :, k + 1] = 32.0 + 10.0 * np.cos(a) + scatter * rng.normal(size=(rows, walkers))
    return np.repeat(c, repeat, axis=0)


def straddle_chain(variant):
    """PA samples on both sides of 0, and exactly 0: the companion straight above the
    primary, x offsets of both signs and exact zeros (deltax = +0.0, so -deltax = -0.0)."""
    c = make_chain(6, 7, variant, seed=5, pa0=0.0, scatter=0.0)
    off = np.array([-0.4, -0.25, -0.1, 0.0, 0.0, 0.05, 0.2])[:, None] * np.ones((1, 6))
    off[:, 1::2] *= 1.5
    for k in (2, 4)[:variant - 1]:
        c[:, :, k] = c[:, :, 0] + off
    return c


def scalars(rotation_angle=0.0, parantel=0.0, rotcorr=0.0, use_rotcorr=False):
    return {"pixscale": PIXSCALE, "rotation_angle": rotation_angle, "rotcorr": rotcorr,
            "use_rotcorr": use_rotcorr, "parantel": parantel}


def device(chain, s, variant, delta_r=0.0, with_tables=True, splits=None, capacity=None):
    rows, W = chain.shape[:2]
    kw = dict(x_dist=XD, y_dist=YD, xdiff=XDIFF, ydiff=YDIFF) if with_tables else {}
    with Astrometry(W, capacity or rows, variant=variant, pixscale=s["pixscale"],
                    rotation_angle=s["rotation_angle"], rotcorr=s["rotcorr"],
                    use_rotcorr=s["use_rotcorr"], parantel=s["parantel"], **kw) as a:
        edges = [0] + list(splits or []) + [rows]
        for lo, hi in zip(edges, edges[1:]):
            a.fold_rows(chain[lo:hi])
        res = a.finalize(delta_r=delta_r)
        return res, [a.samples(p) for p in range(a.npairs)]


def restated(chain, s, variant, delta_r=0.0, with_tables=True):
    if with_tables:
        return RESTATE[variant](chain, s, XD, YD, XDIFF, YDIFF, delta_r)
    return RESTATE[variant](chain, s, deltaR=delta_r)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


SHAPES = {"1x1": lambda v: make_chain(1, 1, v, 1),
          "3x5": lambda v: make_chain(3, 5, v, 2),
          "4x5": lambda v: make_chain(4, 5, v, 3),
          "130x67": lambda v: make_chain(130, 67, v, 4),
          "ties": lambda v: make_chain(10, 6, v, 6, repeat=8),
          "straddle": straddle_chain}


def check_parity(res, samp, ref, n):
    for p, (r, (sep, pa), q) in enumerate(zip(res, samp, ref)):
        dsep = np.max(np.abs(sep - q["sep_corrected"]) / np.abs(q["sep_corrected"]))
        dpa = np.max(np.abs(pa - q["pa_angle"]))
        print(f"pair {p}: max rel dev sep {dsep:.3e}, max dev pa {dpa:.3e} deg")
        assert dsep <= SEP_RTOL and dpa <= PA_ATOL, (p, dsep, dpa)
        assert r["branch_code"] == q["branch_code"] and r["added_360"] == q["added_360"]
        assert r["samples"] == n
        smax = np.max(np.abs(q["sep_corrected"]))
        pmax = np.max(np.abs(q["pa_angle"]))
        sum_eps = n * 2.0 ** -53
        tol_sep = (SEP_RTOL + sum_eps) * smax
        tol_pa = PA_ATOL + sum_eps * pmax
        tol_rd = tol_sep + smax * np.radians(tol_pa) + 8 * 2.0 ** -53 * smax
        for key, tol in (("sep_median", tol_sep), ("sep_std", tol_sep), ("pa_median", tol_pa),
                         ("pa_std", tol_pa), ("ra", tol_rd), ("ra_std", tol_rd),
                         ("dec", tol_rd), ("dec_std", tol_rd)):
            d = abs(r[key] - float(q[key]))
            print(f"  {key}: device {r[key]!r} restatement {float(q[key])!r} dev {d:.3e}")
            assert d <= tol, (p, key, r[key], float(q[key]), tol)
        np.testing.assert_allclose(r["position_means"], q["position_means"],
                                   rtol=sum_eps + 4 * 2.0 ** -53)
        assert abs(r["pa_mean_uncorrected"] - q["pa_mean_uncorrected"]) <= \
            (sum_eps + 4 * 2.0 ** -53) * 400 + PA_ATOL


@pytest.mark.parametrize("variant", [2, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_medians_are_exact_and_samples_match(lib_loaded, shape, variant):
    chain = SHAPES[shape](variant)
    s = scalars(rotation_angle=0.0 if shape == "straddle" else 10.0)
    # (the straddling case without tables: with them deltax is never exactly zero)
    tab = shape != "straddle"
    delta_r = 20.0 if tab else 0.0
    res, samp = device(chain, s, variant, delta_r, with_tables=tab)
    n = chain.shape[0] * chain.shape[1]
    for r, (sep, pa) in zip(res, samp):
        assert sep.shape == chain.shape[:2]
        assert bits(r["sep_median"]) == bits(np.median(sep))
        assert bits(r["pa_median"]) == bits(np.median(pa))
    if shape == "straddle" and variant == 2:
        pa = samp[0][1]
        assert (pa < 0).any() and (pa > 0).any() and (pa == 0).any()
    check_parity(res, samp, restated(chain, s, variant, delta_r, with_tables=tab), n)


@pytest.mark.parametrize("shape", list(fc.ASTROM))
def test_medians_and_parity_past_the_grid_caps(lib_loaded, shape):
    """Variant 2 with the tables at sample counts past the caps (tests/fold_scale_cases.py):
    700 x 400 = 280,000 samples give the select's 1024 x 256 threads a second trip of their
    grid-stride loops; 1025 x 1024 = 1,049,600 are past astrom_correct_kernel's 4096 x 256
    threads and make 257 stage-1 partials for the 256 threads of reduce_stage2_kernel
    (olpe_reduce.h).  (The
    NumPy restatement of the larger case takes 0.3 s with the tables, so they stay.)"""
    W, rows, tab = fc.ASTROM[shape]
    chain = make_chain(W, rows, 2, seed=31)
    s = scalars(rotation_angle=10.0)
    res, samp = device(chain, s, 2, 20.0, with_tables=tab)
    for r, (sep, pa) in zip(res, samp):
        assert sep.shape == (rows, W)
        assert bits(r["sep_median"]) == bits(np.median(sep))
        assert bits(r["pa_median"]) == bits(np.median(pa))
    check_parity(res, samp, restated(chain, s, 2, 20.0, with_tables=tab), W * rows)


# (rotation_angle, parantel) for a geometric PA of about 30 deg -> the branch it lands in
BRANCH_CASES = {
    "mean_negative": (-60.0, 0.0),        # mean(pa) ~ -30 -> + 360 (:340), then pop ~ 330
    "below_ge90": (90.0, 0.0),            # mean ~ 120, pop ~ 120
    "below_lt90": (20.0, -60.0),          # mean ~ 50, pop ~ 110
    "above_gt270_mean_gt270": (270.0, 0.0),   # mean ~ 300, pop ~ 300
    "above_gt270_mean_lt270": (170.0, -80.0),  # mean ~ 200, pop ~ 280
    "above_plain": (10.0, 0.0),           # mean ~ 40, pop ~ 40
}
EXPECT_BRANCH = {2: {"mean_negative": 2, "below_ge90": 0, "below_lt90": 1,
                     "above_gt270_mean_gt270": 2, "above_gt270_mean_lt270": 2, "above_plain": 4},
                 3: {"mean_negative": 2, "below_ge90": 5, "below_lt90": 5,
                     "above_gt270_mean_gt270": 2, "above_gt270_mean_lt270": 3, "above_plain": 4}}


@pytest.fixture(scope="module")
def branch_chains():
    # variant 3's second pair sits 25 deg further round: 20 + 10 and 45 + 10 deg keep both
    # pairs in the branch (and a degree away from 90 / 270) in every case below
    return {2: make_chain(130, 67, 2, 11), 3: make_chain(130, 67, 3, 12, pa0=20.0)}


@pytest.mark.parametrize("delta_r", [0.0, 35.0])
@pytest.mark.parametrize("variant", [2, 3])
@pytest.mark.parametrize("case", list(BRANCH_CASES))
def test_parity_with_restatement_in_every_branch(lib_loaded, branch_chains, case, variant,
                                                 delta_r):
    chain = branch_chains[variant]
    rot, par = BRANCH_CASES[case]
    rot += 10.0 * (variant - 2)          # variant 3's first pair sits at 20 deg, not 30
    s = scalars(rot, par, rotcorr=0.0123, use_rotcorr=(case == "below_ge90"))
    ref = restated(chain, s, variant, delta_r)
    assert ref[0]["branch_code"] == EXPECT_BRANCH[variant][case]
    assert ref[0]["added_360"] == (case == "mean_negative")
    if variant == 3 and case in ("below_ge90", "below_lt90"):
        # variant 3's + 180 applies per sample, where degrees(arctan) came out negative
        assert (ref[0]["pa_angle"] >= 0).all()
    res, samp = device(chain, s, variant, delta_r)
    check_parity(res, samp, ref, chain.shape[0] * chain.shape[1])


def test_parity_without_tables(lib_loaded):
    chain = make_chain(130, 67, 2, 13)
    s = scalars(10.0, 0.0)
    res, samp = device(chain, s, 2, 12.5, with_tables=False)
    check_parity(res, samp, restated(chain, s, 2, 12.5, with_tables=False), 130 * 67)


@pytest.mark.parametrize("variant", [2, 3])
def test_fold_splitting_is_bit_identical(lib_loaded, variant):
    chain = make_chain(130, 67, variant, 21)
    s = scalars(90.0, 0.0)
    one, s_one = device(chain, s, variant, 17.0)
    three, s_three = device(chain, s, variant, 17.0, splits=[1, 30])
    assert json.dumps(one) == json.dumps(three)
    for a, b in zip(s_one, s_three):
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


def test_device_fold_equals_host_fold(golden, lib_loaded):
    """fold(sampler) reads the launch's device chain [W][nrec][PS]; fold_rows the same
    rows from the host, collated [rows][W][PS]: bit-identical samples and summary."""
    from olpefit_amd.core import Sampler
    g = golden("c32")
    smp = Sampler(g["image"], 1.0, 1, 1, 2, nsrc=2)
    smp.seed([1, 2, 3, 4])
    smp.set_state(g["p_init"])
    chain = smp.run(50, burn_in=0, record_stride=1)
    assert chain.shape == (4, 50, 17)
    kw = dict(pixscale=PIXSCALE, rotation_angle=15.0, x_dist=XD, y_dist=YD,
              xdiff=int(np.ceil(0.5 * (1024 - 32))), ydiff=int(np.ceil(0.5 * (1024 - 32))))
    with Astrometry(4, 50, **kw) as a, Astrometry(4, 50, **kw) as b:
        a.fold(smp)
        with pytest.raises(_lib.OlpeError) as e:     # the same launch twice
            a.fold(smp)
        assert e.value.code == _lib.ESTATE and "already folded" in str(e.value)
        b.fold_rows(np.ascontiguousarray(np.transpose(chain, (1, 0, 2))))
        ra, rb = a.finalize(3.0), b.finalize(3.0)
        assert json.dumps(ra) == json.dumps(rb)
        for x, y in zip(a.samples(0), b.samples(0)):
            assert np.array_equal(bits(x), bits(y))
        assert a.rows == 50
    smp.close()


def test_bad_rows_are_errors_not_faults(lib_loaded):
    s = scalars(10.0, 0.0)
    chain = make_chain(5, 9, 2, 31)
    chain[3, 2, 2] = np.nan
    chain[4, 1, 0] = np.inf
    with pytest.raises(_lib.OlpeError) as e:
        device(chain, s, 2)
    assert e.value.code == _lib.EINVAL and "2 sample(s)" in str(e.value)
    # table indices outside the table: beyond it, and negative (NumPy would wrap)
    chain = make_chain(5, 9, 2, 32)
    chain[0, 0, 3] = 1024.0 - YDIFF          # + 1 -> index 1025 - ... beyond the last row
    chain[1, 1, 2] = -XDIFF - 5.0            # negative index
    chain[2, 2, 1] = 1e300
    with pytest.raises(_lib.OlpeError) as e:
        device(chain, s, 2)
    assert e.value.code == _lib.EINVAL and "3 sample(s)" in str(e.value)
    # without tables only the non-finite position is unusable
    chain[2, 2, 1] = 32.0
    res, _ = device(chain, s, 2, with_tables=False)
    assert res[0]["samples"] == 45


def test_refused_calls(lib_loaded):
    chain = make_chain(3, 5, 2, 41)
    with Astrometry(3, 4, pixscale=PIXSCALE, rotation_angle=0.0) as a:
        a.fold_rows(chain[:3])
        with pytest.raises(_lib.OlpeError) as e:
            a.fold_rows(chain[3:])                 # 3 + 2 rows into a capacity of 4
        assert e.value.code == _lib.ESTATE and "store full" in str(e.value)
        assert a.rows == 3
        with pytest.raises(_lib.OlpeError) as e:
            a.samples(0)                           # before finalize
        assert e.value.code == _lib.ESTATE
        a.finalize()
        with pytest.raises(_lib.OlpeError) as e:
            a.finalize()
        assert e.value.code == _lib.ESTATE
    with Astrometry(3, 4, pixscale=PIXSCALE, rotation_angle=0.0) as a:
        with pytest.raises(_lib.OlpeError) as e:
            a.finalize()                           # nothing folded
        assert e.value.code == _lib.ESTATE


HEADER = {"KOAID": "N2.20250127.00001.fits", "PARANG": 12.5, "ROTPPOSN": 100.25,
          "INSTANGL": 0.7, "EL": 55.0, "AZ": 200.0, "ROTMODE": "position angle",
          "PARANTEL": -20.0, "ITIME": 1.0, "COADDS": 1, "MULTISAM": 1, "SAMPMODE": 2}


def test_cli_astrometry_lines_and_unchanged_default(tmp_path, lib_loaded):
    """apf_step3 --astrometry on a small step-2 output: the appended lines' fields equal
    the restatement's (within the parity bounds), formatted as Python 2's str(float);
    without --astrometry the summary file is what it was before the option existed."""
    d = tmp_path / "2014_test"
    path = synth.write_case(str(d), 32, 2)
    img, _ = synth.make_image(32, 2, 0)
    fitsio.write(path, img, {**synth.HEADER, **HEADER})
    out = step2.main([path, "--walkers", "4", "--seed", "3", "--iters", "120", "--burn-in", "20",
                      "-q"])
    plain = step3.main([path, "sys", "-s", "4", "-q"])
    with open(out + "step3_summary.json", "rb") as f:
        before = f.read()
    assert "astrometry" not in plain and b"astrometry" not in before
    assert before == json.dumps(plain, indent=1).encode()
    assert not os.path.exists(str(d) + "/epoch_grand_pasep")
    got = step3.main([path, "sys", "-s", "4", "-q", "--astrometry", "--delta-r", "4.5"])
    chains = step3.load_chains(out, 4, 1)
    hdr = fitsio.getdata_header(path)[1]
    sc = header_scalars(hdr, "pre")                    # directory 2014_*: pre-2015
    assert got["astrometry"]["prepost"] == "pre" and got["astrometry"]["distortion"] is None
    ref = RESTATE[2](chains, sc, deltaR=4.5)[0]
    with open(str(d) + "/epoch_grand_pasep") as f:
        pasep = f.read().splitlines()
    with open(str(d) + "/epoch_grand_radec") as f:
        radec = f.read().splitlines()
    assert len(pasep) == 1 and len(radec) == 1
    pf, rf = pasep[0].split(" , "), radec[0].split(" , ")
    assert pf[0] == rf[0] == HEADER["KOAID"] and len(pf) == 11 and len(rf) == 5
    assert pf[5:9] == ["nan"] * 4
    assert pf[9:] == [py2_str(plain["gr_rc_mean"]), py2_str(plain["gr_rc_std"])]
    res = got["astrometry"]["pairs"][0]
    for field, key in zip(pf[1:5] + rf[1:], ("sep_median", "sep_std", "pa_median", "pa_std",
                                             "ra", "ra_std", "dec", "dec_std")):
        assert field == py2_str(res[key])
        assert field == py2_str(ref[key]), (key, res[key], float(ref[key]))
    with open(out + "step3_summary.json") as f:
        saved = json.load(f)
    assert saved["astrometry"]["pasep_line"] == pasep[0]
    assert {k: v for k, v in saved.items() if k != "astrometry"} == json.loads(before)
    # with the tables (written as FITS, big-endian f64): a second line, the tables' values in it
    fitsio.write(str(tmp_path / "xd.fits"), XD)
    fitsio.write(str(tmp_path / "yd.fits"), YD)
    got = step3.main([path, "sys", "-s", "4", "-q", "--astrometry", "--prepost", "post",
                      "--distortion", str(tmp_path / "xd.fits"), str(tmp_path / "yd.fits")])
    ref = RESTATE[2](chains, header_scalars(hdr, "post"), XD, YD, 496, 496, 0.0)[0]
    with open(str(d) + "/epoch_grand_pasep") as f:
        pasep = f.read().splitlines()
    assert len(pasep) == 2 and got["astrometry"]["pixscale"] == 9.971
    assert pasep[1].split(" , ")[1:5] == [py2_str(ref[k]) for k in
                                          ("sep_median", "sep_std", "pa_median", "pa_std")]
    assert pasep[1] != pasep[0]


def test_cli_astrometry_three_sources(tmp_path, lib_loaded):
    """3body/apf_step3_3body.py --astrometry: b and c about a, in the 3-source script's
    field order (3body :575-613), each pair in its own branch."""
    d = tmp_path / "2016_test"
    path = synth.write_case(str(d), 64, 3)
    img, _ = synth.make_image(64, 3, 0)
    fitsio.write(path, img, {**synth.HEADER, **HEADER})
    out = step2.main([path, "--walkers", "3", "--seed", "5", "--iters", "100", "--burn-in", "20",
                      "-q"], nsrc=3)
    got = step3.main([path, "sys", "-s", "3", "-q", "--astrometry", "--delta-r", "-6.25"], nsrc=3)
    chains = step3.load_chains(out, 3, 1)
    assert chains.shape[2] == 20
    sc = header_scalars(fitsio.getdata_header(path)[1], "post")      # directory 2016_*
    ref = RESTATE[3](chains, sc, deltaR=-6.25)
    pairs = got["astrometry"]["pairs"]
    assert [p["pair"] for p in pairs] == ["b", "c"]
    assert [p["branch_code"] for p in pairs] == [r["branch_code"] for r in ref]
    with open(str(d) + "/epoch_grand_pasep") as f:
        pf = f.read().splitlines()[0].split(" , ")
    with open(str(d) + "/epoch_grand_radec") as f:
        rf = f.read().splitlines()[0].split(" , ")
    assert len(pf) == 16 and len(rf) == 9 and pf[9:14] == ["nan"] * 5
    want_p = [py2_str(r[k]) for r in ref for k in ("sep_median", "sep_std", "pa_median", "pa_std")]
    want_r = [py2_str(r[k]) for r in ref for k in ("ra", "ra_std", "dec", "dec_std")]
    assert pf[1:9] == want_p and rf[1:] == want_r
