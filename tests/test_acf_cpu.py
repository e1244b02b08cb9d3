"""Autocorrelation times without a GPU: the windowing and flags of
autocorr.integrated_time on hand-made lag sums, the NumPy restatement (acf_restatement.py)
against the analytic AR(1) value, and the argument checks of olpe_acf_create and the CLI,
which come before any GPU call."""
import ctypes as C

import numpy as np
import pytest

import acf_restatement as ar
from olpefit_amd import _lib, autocorr, step3


@pytest.fixture(scope="module")
def lib():
    from olpefit_amd import build
    build.build(verbose=False)
    return _lib.load()


def geometric(phi, L, c0=3.5):
    return c0 * phi ** np.arange(L + 1)


def test_delta_gives_tau_one():
    """f = delta: tau(M) = 1 for every M, so the window is the smallest M >= c: 1 for c = 1,
    5 for emcee's c = 5."""
    Cm = np.zeros((2, 65))
    Cm[:, 0] = [2.0, 7.0]
    r = autocorr.integrated_time(Cm, 4000, 2, c=1.0)
    assert r["tau"].tolist() == [1.0, 1.0] and r["window"].tolist() == [1, 1]
    assert r["windowed"].all() and r["reliable"].all() and r["notes"] == ["", ""]
    assert r["ess"].tolist() == [4000.0, 4000.0] and r["min_ess"] == 4000.0
    assert r["suggested_stride"].tolist() == [1, 1]
    r = autocorr.integrated_time(Cm[0], 4000, 2)          # one column, c = 5
    assert r["tau"].tolist() == [1.0] and r["window"].tolist() == [5]


def test_geometric_gives_three_and_window_fifteen():
    """f = 0.5^k: tau(M) = 3 - 4 x 0.5^(M+1) -> 3, and M* = 15 is the first M >= 5 tau(M)."""
    r = autocorr.integrated_time(geometric(0.5, 64), 64 * 2000, 64)
    want = 3.0 - 4.0 * 0.5 ** 16
    assert r["window"].tolist() == [15] and abs(r["tau"][0] - want) < 1e-14
    assert abs(r["tau"][0] - 3.0) < 1e-4
    assert r["windowed"][0] and r["reliable"][0]
    assert r["suggested_stride"].tolist() == [3]
    assert abs(r["ess"][0] - 64 * 2000 / want) < 1e-6
    assert np.allclose(r["f"][0], 0.5 ** np.arange(65), rtol=1e-15)
    # the restatement's windowing is the same rule
    tau, m, windowed, reliable, _ = ar.integrated_time(geometric(0.5, 64), 64 * 2000, 64)
    assert (m, windowed, reliable) == (15, True, True) and abs(tau - want) < 1e-14


def test_no_window_is_a_lower_bound_with_a_note():
    """phi = 0.97: tau = 65.7, 5 tau > 64, so no M <= L = 64 qualifies: tau(L) is reported,
    windowed and reliable are False."""
    r = autocorr.integrated_time(geometric(0.97, 64), 10 ** 9, 10)
    assert not r["windowed"][0] and not r["reliable"][0]
    assert r["window"].tolist() == [64] and r["notes"] == ["max_lag too small"]
    want = 2.0 * (1 - 0.97 ** 65) / 0.03 - 1.0
    assert abs(r["tau"][0] - want) < 1e-10 and r["tau"][0] < 1.97 / 0.03
    assert autocorr.integrated_time(geometric(0.97, 1024), 10 ** 9, 10)["windowed"][0]


def test_constant_column_and_no_samples():
    Cm = np.stack([np.zeros(65), geometric(0.5, 64)])
    r = autocorr.integrated_time(Cm, 640, 10)
    assert np.isnan(r["tau"][0]) and np.isnan(r["ess"][0]) and r["notes"][0] == "constant column"
    assert not r["windowed"][0] and not r["reliable"][0] and r["suggested_stride"][0] == 0
    assert r["notes"][1] == "" and r["min_ess"] == r["ess"][1]
    r = autocorr.integrated_time(np.zeros((2, 65)), 0, 0)
    assert r["notes"] == ["no samples"] * 2 and np.isnan(r["tau"]).all()
    assert np.isnan(r["min_ess"])


def test_reliable_flips_at_fifty_tau():
    """reliable iff the mean series length n / series >= tol tau; f = delta has tau = 1
    exactly, so the flip is at n / series = 50 (and at 20 for tol = 20)."""
    Cm = np.zeros(65)
    Cm[0] = 1.0
    assert autocorr.integrated_time(Cm, 50 * 8, 8)["reliable"][0]
    assert not autocorr.integrated_time(Cm, 50 * 8 - 1, 8)["reliable"][0]
    assert autocorr.integrated_time(Cm, 20 * 8, 8, tol=20.0)["reliable"][0]
    assert not autocorr.integrated_time(Cm, 20 * 8 - 1, 8, tol=20.0)["reliable"][0]


@pytest.fixture(scope="module")
def ar1_case():
    """64 series x 2,000 rows, columns phi = 0.5 and white noise, seed 4 (tau 2.966 and
    0.9986; seeds 0 .. 4 give 2.92 .. 3.07 and 0.966 .. 1.011)."""
    rows = ar.ar1([0.5, 0.0], 64, 2000, 4)
    rows.setflags(write=False)
    return rows, ar.lag_sums(rows, 512)


def test_restatement_against_the_analytic_ar1_value(ar1_case):
    """AR(1) with phi = 0.5 has tau = (1 + phi) / (1 - phi) = 3; white noise has tau = 1.
    This bounds the reference alone (the device is compared with the restatement)."""
    _, ref = ar1_case
    assert ref["n"] == 64 * 2000 and ref["series"] == 64 and ref["skipped"] == 0
    tau, m, windowed, reliable, ess = ar.integrated_time(ref["C"][0], ref["n"], ref["series"])
    print("AR(1) phi 0.5: tau", tau, "window", m)
    assert abs(tau - 3.0) <= 0.3 and windowed and reliable
    tau0, m0, *_ = ar.integrated_time(ref["C"][1], ref["n"], ref["series"])
    print("white noise: tau", tau0, "window", m0)
    assert abs(tau0 - 1.0) <= 0.05
    # the package's host arithmetic on the same sums
    r = autocorr.integrated_time(ref["C"].astype(np.float64), ref["n"], ref["series"])
    assert r["window"].tolist() == [m, m0]
    assert abs(r["tau"][0] - tau) <= 1e-12 * tau and abs(r["tau"][1] - tau0) <= 1e-12


def test_restatement_shapes_and_skips():
    """Time-major rows give the same sums; a lag >= N is exactly 0; a series with a NaN or
    an inf is left out whole."""
    rows = ar.chain_like(5, 40, 3, 1)
    a = ar.lag_sums(rows, 64)
    b = ar.lag_sums(np.swapaxes(rows, 0, 1), 64, time_major=True)
    assert np.array_equal(a["C"], b["C"]) and a["n"] == 200
    assert np.all(a["C"][:, 40:] == 0.0) and np.all(a["C"][:, 0] > 0)
    bad = rows.copy()
    bad[1, 7, 2] = np.nan
    bad[3, 0, 0] = np.inf
    c = ar.lag_sums(bad, 64)
    assert (c["series"], c["skipped"], c["n"]) == (3, 2, 120)
    assert np.array_equal(c["C"], ar.lag_sums(rows[[0, 2, 4]], 64)["C"])


@pytest.mark.parametrize("max_lag", [0, 63, 96, 1088])
def test_create_refuses_a_bad_max_lag_before_any_gpu_call(lib, max_lag):
    h = C.c_void_p()
    assert lib.olpe_acf_create(0, 17, max_lag, C.byref(h)) == _lib.EINVAL
    msg = lib.olpe_last_error().decode()
    assert f"max_lag {max_lag}" in msg and not h.value


@pytest.mark.parametrize("ncols", [0, 25])
def test_create_refuses_bad_ncols_before_any_gpu_call(lib, ncols):
    h = C.c_void_p()
    assert lib.olpe_acf_create(0, ncols, 512, C.byref(h)) == _lib.EINVAL
    assert f"ncols {ncols}" in lib.olpe_last_error().decode() and not h.value
    assert lib.olpe_acf_create(-1, 17, 512, C.byref(h)) == _lib.EINVAL      # no CPU path
    assert lib.olpe_acf_create(0, 17, 512, None) == _lib.EINVAL


def test_tile_knob_is_validated(lib, monkeypatch):
    h = C.c_void_p()
    for bad in ("0", "96", "576", "x"):
        monkeypatch.setenv("OLPE_ACF_TILE", bad)
        assert lib.olpe_acf_create(0, 17, 512, C.byref(h)) == _lib.EINVAL
        assert "OLPE_ACF_TILE=" + bad in lib.olpe_last_error().decode()


def test_null_handles_are_errors(lib):
    assert lib.olpe_acf_fold_ctx(None, None) == _lib.EINVAL
    assert lib.olpe_acf_fold_rows(None, None, 1, 1, 0) == _lib.EINVAL
    assert lib.olpe_acf_get(None, None, None, None, None) == _lib.EINVAL
    assert lib.olpe_acf_add(None, 17, 512, 0, 0, 0, None) == _lib.EINVAL
    assert lib.olpe_acf_reset(None) == _lib.EINVAL
    lib.olpe_acf_destroy(None)


def test_no_gpu_fails_cleanly(lib):
    """Without a GPU a valid create is OLPE_EHIP with a message and no object (no abort,
    no CPU path); with one it succeeds."""
    n = C.c_int(0)
    lib.olpe_device_count(C.byref(n))
    if n.value == 0:
        with pytest.raises(_lib.OlpeError) as e:
            autocorr.Autocorr(17)
        assert e.value.code == _lib.EHIP and "no HIP device" in str(e.value)
    else:
        with autocorr.Autocorr(17) as a:
            assert a.state()["n"] == 0


def test_autocorr_with_from_moments_is_an_argument_error(tmp_path):
    image = str(tmp_path / "N2.20250127.00042.LDIF.fits")
    with pytest.raises(SystemExit) as e:
        step3.main([image, "x", "-s", "4", "-q", "--autocorr", "--from-moments"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        step3.main([image, "x", "-s", "4", "-q", "--autocorr", "--autocorr-max-lag", "96"])
    assert e.value.code == 2
