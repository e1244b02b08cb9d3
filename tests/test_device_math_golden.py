"""Self-check of tests/golden/device_math.npz (no GPU): a broken fixture must not pass
silently.  NumPy's own exp / sin / cos / log lie within 1 ulp of the stored exact values,
the inputs are the generator's, and -- where mpmath is importable -- a thin slice
regenerated now equals the file."""
import importlib.util
import os

import numpy as np
import pytest

from probe_lib import ulp_err

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PI4 = 0.78539816339744830962


def _gen():
    spec = importlib.util.spec_from_file_location(
        "make_device_math_golden", os.path.join(GOLDEN, "make_device_math_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_is_small_and_complete(golden):
    g = golden("device_math")
    size = os.path.getsize(os.path.join(GOLDEN, "device_math.npz"))
    assert size < os.path.getsize(os.path.join(GOLDEN, "c128_3.npz"))
    for grp, n_min in (("exp", 3000), ("expneg", 3000), ("trig", 1000), ("log", 1000)):
        assert g[grp + "_x"].size >= n_min
    x = g["exp_x"]
    for v in (-1000.0, 710.0, 0.0, -np.inf, np.inf, 1e300, -1e300):
        assert v in x
    assert np.sum(np.abs(x - -708.3964185322641) < 1e-9) > 200
    assert np.sum(np.abs(x - -745.1332191019411) < 1e-9) > 200
    assert np.sum(np.abs(x - 709.782712893384) < 1e-9) > 200
    th = g["trig_x"]
    assert PI4 in th and -PI4 in th and np.nextafter(PI4, 1) in th and np.nextafter(PI4, 0) in th
    assert np.abs(th).max() == 50.0 and 0.0 in th
    u = g["log_x"]
    assert 0.0 in u and 2.0 ** -53 in u and 1.0 - 2.0 ** -53 in u and u.max() < 1.0


def test_inputs_are_the_generators():
    """The inputs are deterministic: the generator's input functions (NumPy only) give
    the arrays of the file."""
    gen = _gen()
    with np.load(os.path.join(GOLDEN, "device_math.npz")) as g:
        np.testing.assert_array_equal(g["exp_x"], gen.exp_inputs())
        q, far = gen.expneg_inputs()
        np.testing.assert_array_equal(g["expneg_x"], q)
        np.testing.assert_array_equal(g["expneg_far_x"], far)
        np.testing.assert_array_equal(g["trig_x"], gen.trig_inputs())
        np.testing.assert_array_equal(g["log_x"], gen.log_inputs())
        assert g["thr0"][0] == gen.THR0 == 1490.2664382038824


def test_numpy_within_one_ulp_of_fixture(golden):
    g = golden("device_math")
    with np.errstate(all="ignore"):
        cases = [("exp", np.exp(g["exp_x"]), g["exp_hi"], g["exp_lo"], g["exp_lo_ulp"]),
                 ("expneg", np.exp(-g["expneg_x"]), g["expneg_hi"], g["expneg_lo"],
                  g["expneg_lo_ulp"]),
                 ("sin", np.sin(g["trig_x"]), g["trig_sin_hi"], g["trig_sin_lo"], None),
                 ("cos", np.cos(g["trig_x"]), g["trig_cos_hi"], g["trig_cos_lo"], None),
                 ("log", -2.0 * np.log(g["log_x"]), g["log_hi"], g["log_lo"], None)]
    for name, got, hi, lo, lo_ulp in cases:
        fin = np.isfinite(hi)
        # overflow, exact zero beyond the range, NaN: the same special value
        np.testing.assert_array_equal(got[~fin], hi[~fin], err_msg=name)
        e = np.abs(ulp_err(got, hi, lo, lo_ulp)[fin])
        print(f"numpy {name}: max {e.max():.3f} ulp over {fin.sum()} finite values")
        assert e.max() <= 1.0, (name, e.max())
        # hi is the nearest double: the residual is at most half an ulp
        r = np.abs(ulp_err(hi, hi, lo, lo_ulp)[fin])
        assert r.max() <= 0.5, (name, r.max())
    # the squared terms and sin(2 th) against their definition from sin and cos
    s, c = g["trig_sin_hi"], g["trig_cos_hi"]
    for k, v in (("c2", c * c), ("s2", s * s), ("s2t", 2.0 * s * c)):
        e = np.abs(ulp_err(v, g[f"trig_{k}_hi"], g[f"trig_{k}_lo"]))
        # two factors of <= 0.5 ulp each and the roundings of the products
        assert np.nanmax(e) <= 2.5, (k, np.nanmax(e))


def test_thin_slice_regenerates(golden):
    """With mpmath: every 41st entry recomputed now equals the file, and the accept
    threshold of dice = 0 is the smallest d whose exp(-d/2) rounds to 0."""
    pytest.importorskip("mpmath")        # the report shows when it did not run
    gen = _gen()
    g = golden("device_math")
    gen.check_threshold_constant()
    sl = slice(None, None, 41)
    for grp, f in (("exp", gen.exact_exp), ("expneg", gen.exact_expneg),
                   ("log", gen.exact_m2log)):
        hi, lo, lo_ulp = f(g[grp + "_x"][sl])
        np.testing.assert_array_equal(hi, g[grp + "_hi"][sl], err_msg=grp)
        np.testing.assert_array_equal(lo, g[grp + "_lo"][sl], err_msg=grp)
        if grp != "log":
            np.testing.assert_array_equal(lo_ulp, g[grp + "_lo_ulp"][sl], err_msg=grp)
    for k, (hi, lo) in gen.exact_trig(g["trig_x"][sl]).items():
        np.testing.assert_array_equal(hi, g[f"trig_{k}_hi"][sl], err_msg=k)
        np.testing.assert_array_equal(lo, g[f"trig_{k}_lo"][sl], err_msg=k)
