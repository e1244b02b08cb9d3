"""The host arithmetic of olpefit_amd/covariance.py on hand-made states and matrices with
known answers, to 1e-12 relative (the matrices have condition <= 100, so an eigen-solve is
good to about 1e-14: two orders of margin), and the argument checks of olpe_cov_* that come
before any GPU call.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import cov_restatement as cr
from olpefit_amd import _lib, covariance as cv, step3

RTOL = 1e-12


def close(a, b):
    return np.allclose(a, b, rtol=RTOL, atol=0.0)


def state_of(rows, pivot=None):
    """A state dict as Covariance.state() gives it, from the restatement's sums rounded to
    double; rows [W][N][C]."""
    r = cr.sums(rows, pivot)
    W, _, ncols = np.shape(rows)
    return {"ncols": ncols, "walkers": W, "n": r["n"], "skipped": r["skipped"],
            "has_pivot": True, "pivot": r["pivot"].copy(), "S1": r["S1"].astype(np.float64),
            "S2": r["S2"].astype(np.float64), "nw": r["nw"].copy(),
            "S1w": r["S1w"].astype(np.float64)}


@pytest.fixture(scope="module")
def lib():
    from olpefit_amd import build
    build.build(verbose=False)
    return _lib.load()


def test_diagonal_matrix_gives_axis_aligned_ellipses():
    """cov = diag(sigma^2) over (xa, ya, xb, yb): the offset's covariance is the sum of the
    two sources', its axes the square roots, the angle 0 (x the wider) or 90, rho 0."""
    e = cv.error_ellipse(np.diag([4.0, 1.0, 5.0, 3.0]), (0, 1), (2, 3), pixscale=9.952)
    assert close(e["cov2"], np.diag([9.0, 4.0]))
    assert close([e["semi_major"], e["semi_minor"]], [3.0, 2.0])
    assert e["angle"] == 0.0 and e["rho"] == 0.0
    assert close([e["semi_major_mas"], e["semi_minor_mas"]], [3.0 * 9.952, 2.0 * 9.952])
    e = cv.error_ellipse(np.diag([1.0, 4.0, 3.0, 5.0]), (0, 1), (2, 3))
    assert close([e["semi_major"], e["semi_minor"]], [3.0, 2.0])
    assert e["angle"] == 90.0 and e["rho"] == 0.0 and "semi_major_mas" not in e


@pytest.mark.parametrize("rho", [0.6, -0.6, 0.98])
def test_correlated_pair(rho):
    """A 2 x 2 matrix with correlation rho and equal variances: the conditional width is
    sigma sqrt(1 - rho^2), the major axis lies at 45 (rho > 0) or 135 degrees, the
    eigenvalues are sigma^2 (1 +- |rho|).  Condition (1 + |rho|) / (1 - |rho|) <= 99."""
    s = 0.37
    c2 = s * s * np.array([[1.0, rho], [rho, 1.0]])
    cs = cv.conditional_sigma(c2)
    assert close(cs["sigma_cond"], [s * np.sqrt(1 - rho * rho)] * 2)
    assert close(cs["efficiency"], [np.sqrt(1 - rho * rho)] * 2)
    assert close(cs["sigma_marginal"], [s, s])
    assert close(cs["condition"], (1 + abs(rho)) / (1 - abs(rho)))
    # the star fixed (zero variance, columns 0, 1): the offset's covariance is the companion's
    c4 = np.zeros((4, 4))
    c4[2:, 2:] = c2
    e = cv.error_ellipse(c4, (0, 1), (2, 3))
    assert close(e["angle"], 45.0 if rho > 0 else 135.0)
    assert close(e["rho"], rho)
    assert close([e["semi_major"], e["semi_minor"]],
                 [s * np.sqrt(1 + abs(rho)), s * np.sqrt(1 - abs(rho))])
    # unequal variances: sigma_cond = sigma_j sqrt(1 - rho^2) still
    c2 = np.array([[4.0, rho * 2 * 0.5], [rho * 2 * 0.5, 0.25]])
    assert close(cv.conditional_sigma(c2)["sigma_cond"],
                 [2 * np.sqrt(1 - rho * rho), 0.5 * np.sqrt(1 - rho * rho)])


def test_identical_walkers_give_the_floor_of_rhat():
    """m walkers with the same n rows: the walker means coincide, B = 0 and
    Rp = (n - 1) / n, as every univariate value."""
    rng = np.random.RandomState(5)
    one = rng.normal(size=(40, 3)) @ np.array([[1.0, 0.2, 0.0], [0.0, 1.0, 0.3], [0.0, 0.0, 1.0]])
    st = state_of(np.tile(one, (6, 1, 1)), pivot=one.mean(axis=0))
    mp = cv.mpsrf(st)
    assert (mp["m"], mp["n"], mp["note"]) == (6, 40, "")
    assert abs(mp["mpsrf"] - 39.0 / 40.0) <= 1e-12
    assert np.allclose(mp["rhat"], 39.0 / 40.0, rtol=0, atol=1e-12)
    # the device's between term and the host's are the same function of the state
    bt = cv.between_of(st)
    assert bt["m"] == 6 and bt["nw_min"] == bt["nw_max"] == 40
    assert cv.mpsrf(st, bt)["mpsrf"] == mp["mpsrf"]


def test_mpsrf_equals_the_definition_and_needs_equal_counts():
    rng = np.random.RandomState(6)
    Lm = np.array([[1.0, 0, 0], [0.5, 1.0, 0], [0.2, -0.4, 0.7]])
    rows = rng.normal(size=(5, 60, 3)) @ Lm.T
    rows[3, :, 1] += 2.0
    st = state_of(rows, pivot=rows.mean(axis=(0, 1)))
    mp = cv.mpsrf(st)
    want, rhat = cr.mpsrf(rows)
    assert abs(mp["mpsrf"] - want) <= 1e-9 * want and mp["mpsrf"] > 1.05
    assert np.allclose(mp["rhat"], rhat, rtol=1e-9, atol=0)
    sub = cv.mpsrf(st, cols=[0, 2])
    want2, rhat2 = cr.mpsrf(rows, [0, 2])
    assert abs(sub["mpsrf"] - want2) <= 1e-9 * want2 and np.allclose(sub["rhat"], rhat2, rtol=1e-9)
    # one walker a row short: not defined, and the note gives the counts
    bad = rows.copy()
    bad[2, 7, 0] = np.nan
    mp = cv.mpsrf(state_of(bad, pivot=rows.mean(axis=(0, 1))))
    assert mp["mpsrf"] is None and "59" in mp["note"] and "60" in mp["note"]
    assert cv.mpsrf({**st, "walkers": 0})["mpsrf"] is None


def test_constant_column_is_noted_and_left_out():
    rng = np.random.RandomState(7)
    rows = rng.normal(size=(2, 50, 3))
    rows[:, :, 1] = 512.3
    st = state_of(rows)
    corr, notes = cv.correlation(st)
    assert notes == ["", "constant column", ""]
    assert np.isnan(corr[1]).all() and np.isnan(corr[:, 1]).all()
    assert corr[0, 0] == corr[2, 2] == 1.0 and np.isfinite(corr[0, 2])
    cs = cv.conditional_sigma(cv.covariance(st))
    assert np.isnan(cs["sigma_cond"][1]) and np.isnan(cs["efficiency"][1])
    r = corr[0, 2]
    sd = np.sqrt(np.diag(cv.covariance(st)))
    assert close(cs["sigma_cond"][[0, 2]], sd[[0, 2]] * np.sqrt(1 - r * r))
    mp = cv.mpsrf(st)
    assert np.isnan(mp["rhat"][1]) and np.isfinite(mp["mpsrf"])
    lines = cv.table_lines(cv.summarize(st, ["a", "b", "c"]))
    assert any("(constant column)" in l and l.lstrip().startswith("b ") for l in lines)


def test_covariance_and_mean_equal_numpy():
    rng = np.random.RandomState(8)
    rows = 512.3 + 1e-2 * rng.normal(size=(3, 70, 4))
    st = state_of(rows, pivot=rows[0, 0])
    flat = rows.reshape(-1, 4)
    assert np.allclose(cv.mean(st), flat.mean(axis=0), rtol=1e-14)
    assert np.allclose(cv.covariance(st), np.cov(flat.T), rtol=1e-9)
    assert np.allclose(cv.covariance(st, ddof=0), np.cov(flat.T, ddof=0), rtol=1e-9)
    assert np.allclose(cv.correlation(st)[0], np.corrcoef(flat.T), rtol=1e-9)


def test_rebase():
    """To the same pivot it is the identity; a round trip returns within rounding; a rebased
    state equals the sums taken about the new pivot."""
    rng = np.random.RandomState(9)
    rows = 100.0 + rng.normal(size=(4, 30, 3))
    st = state_of(rows, pivot=rows[0, 0])
    same = cv.rebase(st, st["pivot"])
    for k in ("S1", "S2", "S1w", "pivot"):
        assert np.array_equal(same[k], st[k]), k
    q = rows.mean(axis=(0, 1)) + 0.5
    moved = cv.rebase(st, q)
    want = state_of(rows, pivot=q)
    assert np.array_equal(moved["pivot"], q) and moved["n"] == st["n"]
    assert np.array_equal(moved["S2"], moved["S2"].T)
    for k in ("S1", "S2", "S1w"):
        scale = np.abs(want[k]).max()
        assert np.abs(moved[k] - want[k]).max() <= 1e-12 * scale, k
    back = cv.rebase(moved, st["pivot"])
    for k in ("S1", "S2", "S1w"):
        assert np.abs(back[k] - st[k]).max() <= 1e-12 * np.abs(st[k]).max(), k
    with pytest.raises(ValueError):
        cv.rebase(st, [0.0, np.nan, 0.0])


def test_table_lines_name_the_pairs_and_the_ellipses():
    rng = np.random.RandomState(10)
    z = rng.normal(size=(4, 80, 17))
    z[:, :, 3] += 0.9 * z[:, :, 2]                     # ycc follows xcc
    st = state_of(z, pivot=np.zeros(17))
    res = cv.summarize(st, step3.NAMES_2, k=3, nsrc=2, pixscale=9.952, param_cols=range(16))
    assert res["pairs"][0][:2] == ("xcc", "ycc") and len(res["pairs"]) == 3
    assert [e["name"] for e in res["ellipses"]] == ["companion - star"]
    assert res["conditional"]["cols"] == list(range(16))
    lines = cv.table_lines(res)
    assert lines[0].split()[:2] == ["xcc", "ycc"]
    assert sum(l.startswith("ellipse ") for l in lines) == 1 and "mas" in lines[3]
    assert sum(" efficiency " in l for l in lines) == 16
    assert lines[-1].startswith("Multivariate R-hat (4 walkers x 80 rows): ")
    res3 = cv.summarize(state_of(rng.normal(size=(2, 30, 20))), step3.NAMES_3, nsrc=3)
    assert [e["name"] for e in res3["ellipses"]] == ["b - a", "c - a"]


def test_argument_errors_come_before_any_gpu_call(lib):
    """ncols outside 1 .. 24, negative walkers, a non-finite pivot, row_step < 1, a bad
    OLPE_COV_TILE and NULL handles are EINVAL whether or not there is a GPU."""
    h = C.c_void_p()
    for ncols, walkers in ((0, 0), (25, 0), (-3, 4), (17, -1)):
        assert lib.olpe_cov_create(0, ncols, walkers, None, C.byref(h)) == _lib.EINVAL
        msg = lib.olpe_last_error().decode()
        assert ("ncols" in msg) if walkers >= 0 else ("walkers" in msg)
        assert not h.value
    p = np.zeros(17)
    p[5] = np.inf
    assert lib.olpe_cov_create(0, 17, 0, p.ctypes.data_as(_lib._pd), C.byref(h)) == _lib.EINVAL
    assert b"pivot" in lib.olpe_last_error() and b"5" in lib.olpe_last_error()
    assert lib.olpe_cov_create(-1, 17, 0, None, C.byref(h)) == _lib.EINVAL   # no CPU path
    rows = np.zeros((2, 3, 17))
    assert lib.olpe_cov_fold_rows(None, rows.ctypes.data_as(_lib._pd), 2, 3, 0) == _lib.EINVAL
    assert lib.olpe_cov_fold_ctx(None, None, 1) == _lib.EINVAL
    assert lib.olpe_cov_get(None, None, None, None, None, None, None) == _lib.EINVAL
    assert lib.olpe_cov_walkers_get(None, None, None) == _lib.EINVAL
    assert lib.olpe_cov_between(None, None, None, None, None) == _lib.EINVAL
    assert lib.olpe_cov_add(None, 17, 0, 0, 0, None, None, None, None, None) == _lib.EINVAL
    assert lib.olpe_cov_reset(None) == _lib.EINVAL
    lib.olpe_cov_destroy(None)
    with pytest.raises(ValueError):
        cv.Covariance(17, labels=["a"])
    with pytest.raises(ValueError):
        cv.Covariance(17, pivot=np.zeros(3))


def test_tile_knob_is_validated(lib, monkeypatch):
    h = C.c_void_p()
    monkeypatch.setenv("OLPE_COV_TILE", "100")
    assert lib.olpe_cov_create(0, 17, 0, None, C.byref(h)) == _lib.EINVAL
    assert b"OLPE_COV_TILE" in lib.olpe_last_error()


def test_valid_arguments_fail_only_for_lack_of_a_gpu(lib):
    """Where there is no GPU a create with valid arguments is EHIP, not EINVAL: the argument
    checks above came first and passed.  Negative counts of olpe_cov_fold_rows are EINVAL."""
    n = C.c_int(0)
    lib.olpe_device_count(C.byref(n))
    if not n.value:
        h = C.c_void_p()
        for walkers in (0, 48):
            assert lib.olpe_cov_create(0, 17, walkers, None, C.byref(h)) == _lib.EHIP
            assert not h.value
    rows = np.zeros((2, 3, 17))
    assert lib.olpe_cov_fold_rows(None, rows.ctypes.data_as(_lib._pd), -1, 3, 0) == _lib.EINVAL


def test_covariance_from_moments_is_an_argument_error(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        step3.main([str(tmp_path / "N2.20250127.00001.LDIF.fits"), "sys", "-s", "4",
                    "--covariance", "--from-moments"])
    assert e.value.code == 2
    assert "per-column moments hold no cross terms" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        step3.main([str(tmp_path / "N2.20250127.00001.LDIF.fits"), "sys", "-s", "4",
                    "--covariance", "--covariance-thin", "0"])
