"""Settable proposal widths and their tuner, the parts that need no GPU: the C-ABI's
declarations and bindings, the update rule's NumPy restatement against exact rationals, the
host arithmetic from a covariance state to widths, the widths file, and the step-2 CLI's
argument checks (before any GPU call).
"""
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import tune_restatement as tr
from olpefit_amd import _lib, covariance as cv, step2, tune

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("olpe_widths_set", "olpe_widths_get", "olpe_tune_begin", "olpe_tune_step",
         "olpe_tune_get", "olpe_tune_end")


def _source(*parts):
    with open(os.path.join(REPO, *parts)) as f:
        return f.read()


# -- C-ABI ------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", _source("include", "olpe.h"), flags=re.S)
    for name in ENTRY:
        assert re.search(r"\bint\s+%s\s*\(\s*olpe_ctx\s*\*" % name, text), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is _lib._i
    head = _source("include", "olpe.h")
    assert float(re.search(r"#define OLPE_LOG_WIDTH_MAX\s+([\d.]+)", head).group(1)) == \
        _lib.LOG_WIDTH_MAX
    assert int(re.search(r"#define OLPE_TUNE_LOG\s+(\d+)", head).group(1)) == _lib.TUNE_LOG >= 256
    # each names the reference's line
    assert "apf_step2.py:234" in head and "220-238" in head


def test_log_width_bound_follows_from_the_exp_table_and_the_polar_method():
    """|g| <= sqrt(-2 ln r2) with r2 >= 2^-104 (x1, x2 multiples of 2^-52), and the table
    exp is tested up to 710: the stated bound keeps |w g ln 10| inside it, and is not
    needlessly small (within 5 % of the largest such width)."""
    gmax = np.sqrt(208.0 * np.log(2.0))
    wmax = 710.0 / (gmax * np.log(10.0))
    assert 0.95 * wmax < _lib.LOG_WIDTH_MAX < wmax
    # the tuner's upper clamp (default x 64) stays under it for every log-proposed parameter
    for nsrc in (2, 3):
        d = tune.default_widths(nsrc)
        assert np.all(d[list(tune.log_params(nsrc))] * tune.CLAMP_HI < _lib.LOG_WIDTH_MAX)


def test_python_defaults_equal_the_device_tables_and_the_oracle():
    src = _source("olpefit_amd", "csrc", "olpe.hip")
    for nsrc, n in ((2, 16), (3, 19)):
        m = re.search(r"__constant__ double c_widths%d\[%d\] = \{([^}]*)\}" % (nsrc, n), src)
        table = np.array([float(v) for v in m.group(1).split(",")])
        np.testing.assert_array_equal(table, tune.default_widths(nsrc))
        np.testing.assert_array_equal(table, tr.defaults(nsrc))
        from oracle import olpe_oracle as ora
        assert tuple(ora.layout(nsrc)[3]) == tune.log_params(nsrc)
        assert len(tune.param_names(nsrc)) == n and "chisquare" not in tune.param_names(nsrc)


# -- the rule ---------------------------------------------------------------------------
def test_rule_keeps_the_bits_of_an_untried_parameter():
    d = tr.defaults(2)
    w = d * np.float64(1.2345678901234567)
    dT = np.zeros(16, dtype=np.int64)
    dA = np.zeros(16, dtype=np.int64)
    dT[3], dA[3] = 10, 9
    dT[5], dA[5] = -4, 2                          # counters set back: dT <= 0 keeps too
    out = tr.step(w, dT, dA, 1, 0.44, 2.0, d)
    keep = np.arange(16) != 3
    assert np.array_equal(out[keep].view(np.uint64), w[keep].view(np.uint64))
    assert out[3] != w[3]
    np.testing.assert_array_equal(out, tune.update(w, dT, dA, 1, 0.44, 2.0, d))


def test_rule_hits_both_clamps_exactly():
    d = tr.defaults(3)
    dT = np.full(19, 100, dtype=np.int64)
    # from default x 48, every proposal accepted, target 0.25, gain 2: f = 2.5 -> x 120 > x 64
    up = tr.step(d * 48.0, dT, dT, 1, 0.25, 2.0, d)
    np.testing.assert_array_equal(up, d * 64.0)
    # from default / 1000, nothing accepted, target 0.5, gain 1: f = 0.5 -> / 2000 < / 1024
    dn = tr.step(d / 1000.0, dT, np.zeros(19, dtype=np.int64), 1, 0.5, 1.0, d)
    np.testing.assert_array_equal(dn, d / 1024.0)
    for k in (up, dn):
        np.testing.assert_array_equal(k, tune.update(
            d * 48.0 if k is up else d / 1000.0, dT, dT if k is up else 0 * dT, 1,
            0.25 if k is up else 0.5, 2.0 if k is up else 1.0, d))
    assert tune.CLAMP_LO == 1.0 / tr.CLAMP_LO_DIV and tune.CLAMP_HI == tr.CLAMP_HI_MUL


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_factor_against_exact_rationals(k):
    """dA / dT = 1/4 and target 1/2 are exact and their difference, -1/4, is too; g_k times it
    is a power-of-two scaling of the double g_k, exact; so f is the one rounding of
    1 - g_k / 4, which Fraction -> float performs correctly rounded.  g_k itself: 3 / sqrt(k)
    in double, 3, 3 / sqrt(2), 3 / sqrt(3), 3/2."""
    gk = tr.gain_at(1.5 * 2.0, k)
    if k in (1, 4):
        assert Fraction(float(gk)) == Fraction(3, 1 if k == 1 else 2)
    want = float(Fraction(1) - Fraction(float(gk)) / 4)
    got = tr.factor(8, 2, k, 0.5, 3.0)
    assert got == want and isinstance(got, np.float64)
    if k == 1:
        assert got == 0.25
    if k == 4:
        assert got == 0.625
    # an inexact quotient: a = fl(1/3), d = fl(a - 0.44), p = fl(g d), f = fl(1 + p)
    a = float(Fraction(1, 3))
    d = float(Fraction(a) - Fraction(0.44))
    g2 = tr.gain_at(2.0, k)
    p = float(Fraction(float(g2)) * Fraction(d))
    assert tr.factor(3, 1, k, 0.44, 2.0) == float(Fraction(1) + Fraction(p))
    w = tr.defaults(2)
    dT, dA = np.full(16, 3), np.full(16, 1)
    np.testing.assert_array_equal(tr.step(w, dT, dA, k, 0.44, 2.0, w),
                                  tune.update(w, dT, dA, k, 0.44, 2.0, w))


# -- covariance -> widths ------------------------------------------------------------------
def _state_from_cov(C3, mean3, nsrc, n=4000):
    """A state over PS columns whose columns (0, 6, chi^2) have exactly the covariance of
    rows built from C3's Cholesky factor (n rows, sample covariance matched exactly by
    construction of the sums), every other column constant."""
    P = 16 if nsrc == 2 else 19
    PS = P + 1
    rs = np.random.RandomState(5)
    z = rs.standard_normal((n, 3))
    z -= z.mean(0)
    L = np.linalg.cholesky(np.cov(z.T))
    z = z @ np.linalg.inv(L).T                    # sample covariance = identity
    x3 = z @ np.linalg.cholesky(C3).T + mean3
    rows = np.tile(np.arange(1.0, PS + 1.0), (n, 1))      # constant columns 1, 2, ...
    cols = (0, 6 if nsrc == 2 else 8, PS - 1)
    rows[:, cols] = x3
    pivot = rows[0].copy()
    dd = rows - pivot
    return {"ncols": PS, "walkers": 0, "n": n, "skipped": 0, "has_pivot": True, "pivot": pivot,
            "S1": dd.sum(0), "S2": dd.T @ dd}, cols


@pytest.mark.parametrize("nsrc", [2, 3])
def test_proposal_widths_closed_form(nsrc):
    C3 = np.array([[0.04, 0.9 * 0.2 * 30.0, 0.1], [0.9 * 0.2 * 30.0, 900.0, 5.0],
                   [0.1, 5.0, 7.0]])
    mean3 = np.array([30.5, 5000.0, 4096.0])
    st, cols = _state_from_cov(C3, mean3, nsrc)
    w = cv.proposal_widths(st, nsrc)
    d = tune.default_widths(nsrc)
    P = d.size
    assert w.shape == (P,)
    # chi^2 is absent: the conditional widths are those of the 2 x 2 block alone
    rho = 0.9
    sc0 = 0.2 * np.sqrt(1.0 - rho * rho)
    sc1 = 30.0 * np.sqrt(1.0 - rho * rho)
    amp = cols[1]
    assert amp in tune.log_params(nsrc) and 0 not in tune.log_params(nsrc)
    np.testing.assert_allclose(w[0], 2.38 * sc0, rtol=1e-9)
    np.testing.assert_allclose(w[amp], 2.38 * sc1 / (5000.0 * np.log(10.0)), rtol=1e-9)
    # the constant columns keep the default, bit for bit
    const = [j for j in range(P) if j not in (0, amp)]
    np.testing.assert_array_equal(w[const], d[const])
    # the scale is a plain factor
    np.testing.assert_allclose(cv.proposal_widths(st, nsrc, scale=1.0)[[0, amp]] * 2.38,
                               w[[0, amp]], rtol=1e-15)
    # with chi^2 in the inverse the answer would differ: it is not
    full = cv.conditional_sigma(cv.covariance(st), [0, amp, P])["sigma_cond"]
    assert abs(full[0] - sc0) > 1e-6 * sc0
    # no rows: every default
    empty = dict(st, n=0, S1=np.zeros(P + 1), S2=np.zeros((P + 1, P + 1)))
    np.testing.assert_array_equal(cv.proposal_widths(empty, nsrc), d)


# -- widths file ----------------------------------------------------------------------------
def test_widths_file_round_trip(tmp_path):
    w = tune.default_widths(2) * np.linspace(0.3, 3.1, 16)
    p = str(tmp_path / "w.json")
    tune.save_widths(p, 2, w, "given")
    np.testing.assert_array_equal(tune.load_widths(p, 2), w)
    doc = json.load(open(p))
    assert doc["nsrc"] == 2 and doc["source"] == "given" and doc["names"] == tune.param_names(2)
    assert "history" not in doc
    dT = np.arange(32).reshape(2, 16)
    hist = (0.44, 2.0, dT, dT // 2, np.vstack([w, w * 2]))
    tune.save_widths(p, 2, w * 2, "tuned", hist)
    doc = tune.load_doc(p, 2)
    assert doc["source"] == "tuned" and doc["history"]["dT"] == dT.tolist()
    np.testing.assert_array_equal(np.array(doc["history"]["widths"]), np.vstack([w, w * 2]))
    with pytest.raises(ValueError):
        tune.save_widths(p, 2, w, "tuned")                 # a tuned file carries its history
    tune.save_widths(p, 3, tune.default_widths(3), "covariance")
    np.testing.assert_array_equal(tune.load_widths(p, 3), tune.default_widths(3))


def test_widths_file_wrong_length_and_wrong_nsrc(tmp_path):
    p = str(tmp_path / "w.json")
    tune.save_widths(p, 2, tune.default_widths(2))
    with pytest.raises(ValueError, match="nsrc"):
        tune.load_widths(p, 3)
    doc = json.load(open(p))
    doc["widths"] = doc["widths"][:-1]
    json.dump(doc, open(p, "w"))
    with pytest.raises(ValueError, match="15 widths"):
        tune.load_widths(p, 2)
    with pytest.raises(ValueError):
        tune.save_widths(p, 2, tune.default_widths(3))
    doc["widths"] = list(tune.default_widths(2))
    doc["widths"][4] = -1.0
    json.dump(doc, open(p, "w"))
    with pytest.raises(ValueError, match="finite"):
        tune.load_widths(p, 2)
    json.dump({"widths": [1.0] * 16, "nsrc": 2}, open(p, "w"))
    with pytest.raises(ValueError, match="not a widths file"):
        tune.load_widths(p, 2)


# -- step-2 CLI ---------------------------------------------------------------------------
BASE = ["frame.fits", "--walkers", "8", "--seed", "1"]
OK = ["--tune-widths", "480", "--tune-every", "240", "--burn-in", "480", "--iters", "600"]


def _err(argv, nsrc=2, capsys=None):
    with pytest.raises(SystemExit) as e:
        step2.parse(BASE + argv, nsrc)
    assert e.value.code == 2
    return capsys.readouterr().err if capsys else ""


def test_tuning_flags_parse(capsys):
    a = step2.parse(BASE + OK, 2)
    assert (a.tune_widths, a.tune_every, a.tune_target, a.tune_gain) == (480, 240, 0.44, 2.0)
    a = step2.parse(BASE, 2)
    assert a.tune_widths == 0 and a.widths is None
    # --widths is valid at any --gpus
    assert step2.parse(BASE + ["--widths", "w.json", "--gpus", "4"], 2).widths == "w.json"


def test_tuning_argument_errors(capsys):
    assert "burn-in" in _err(["--tune-widths", "480", "--burn-in", "470", "--iters", "600"],
                             capsys=capsys)
    # N divides T, N a multiple of 10
    assert "tune-every" in _err(["--tune-widths", "480", "--tune-every", "200", "--burn-in", "480",
                                 "--iters", "600"], capsys=capsys)
    assert "tune-every" in _err(["--tune-widths", "96", "--tune-every", "48", "--burn-in", "480",
                                 "--iters", "600"], capsys=capsys)
    # accept_min mode: T <= P x accept_min (16 x 10 = 160 < 240; 19 x 10 = 190 < 240)
    for nsrc in (2, 3):
        assert "accept-min" in _err(["--tune-widths", "240", "--burn-in", "480", "--accept-min",
                                     "10"], nsrc, capsys)
    step2.parse(BASE + ["--tune-widths", "240", "--burn-in", "480", "--accept-min", "15"], 2)
    assert "accept-min" in _err(["--tune-widths", "240", "--burn-in", "480", "--accept-min", "14"],
                                capsys=capsys)
    # more than one context per rank
    assert "--gpus 1" in _err(OK + ["--gpus", "2"], capsys=capsys)
    # the tuner's own domain
    assert "tune-target" in _err(OK + ["--tune-target", "0.6", "--tune-gain", "2"], capsys=capsys)
    assert "tune-target" in _err(OK + ["--tune-target", "1.0"], capsys=capsys)


def test_tuning_refuses_more_than_one_rank():
    a = step2.parse(BASE + OK, 2)
    assert step2.tuning_needs_one_context(a, 1) is None
    assert "--widths" in step2.tuning_needs_one_context(a, 2)
    assert step2.tuning_needs_one_context(step2.parse(BASE, 2), 8) is None


def test_config_gains_keys_only_with_the_flags(tmp_path):
    plain = step2.parse(BASE + ["--burn-in", "480", "--iters", "600"], 2)
    cfg0, w0 = step2.run_config(plain, 2, "2", 1)
    assert w0 is None
    assert set(cfg0) == {"image", "nsrc", "variant", "walkers", "accept_min", "burn_in", "iters",
                         "stride", "exact", "fixed_bkgd", "csv", "npy", "ranks"}
    tuned = step2.parse(BASE + OK, 2)
    cfg1, _ = step2.run_config(tuned, 2, "2", 1)
    assert cfg1.pop("tune") == [480, 240, 0.44, 2.0] and cfg1 == cfg0
    p = str(tmp_path / "w.json")
    w = tune.default_widths(2) * 2.0
    tune.save_widths(p, 2, w)
    given = step2.parse(BASE + ["--burn-in", "480", "--iters", "600", "--widths", p], 2)
    cfg2, w2 = step2.run_config(given, 2, "2", 1)
    np.testing.assert_array_equal(w2, w)
    assert cfg2.pop("widths") == list(w) and cfg2 == cfg0
    # a widths file for the other layout is refused before anything runs
    with pytest.raises(ValueError, match="nsrc"):
        step2.run_config(given, 3, "2", 1)
