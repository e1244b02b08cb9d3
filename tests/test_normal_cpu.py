"""The restatement of the Gauss-Newton sums (tests/normal_restatement.py) against the oracle:
its analytic J equals central differences of oracle.build_analytical_model, and it has the
two properties of the model the fit is designed around.  No GPU."""
import os

import numpy as np
import pytest

import normal_restatement as nr
from olpefit_amd import synth
from olpefit_amd.pipeline import initial_parameters
from oracle import olpe_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LD = np.longdouble


def fixture(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return z["image"], int(z["nsrc"]), z["params"].copy()


@pytest.mark.parametrize("name", ["c32", "c64", "c64_3"])
@pytest.mark.parametrize("bkgd_mode", [0, 1])
def test_jacobian_equals_central_differences_of_the_oracle(name, bkgd_mode):
    """Per column: |J - (M(p + h e_k) - M(p - h e_k)) / 2h| <= 1e-6 max|column|, with
    h = 1e-5 max(1, |p_k|) rounded so that p +- h are exact: the truncation error h^2 M''' / 6
    and the oracle's rounding 1e-13 max|M| / h = 1e-8 max|M| / max(1, |p_k|) both lie well
    inside it for these vectors (vector 1 of each fixture: every parameter off its special
    value, theta != 0, sigma_x != sigma_y)."""
    img, nsrc, params = fixture(name)
    n, p = img.shape[0], params[1]
    P = nr.columns(nsrc)["P"]
    M, J = nr.jacobian(p, n, nsrc, bkgd_mode)
    M0 = olpe_oracle.build_analytical_model(p, n, nsrc, bkgd_mode)
    assert np.abs(M.astype(np.float64) - M0).max() <= 1e-13 * np.abs(M0).max()
    for k in range(P):
        h = 1e-5 * max(1.0, abs(p[k]))
        hi, lo = p.copy(), p.copy()
        hi[k], lo[k] = p[k] + h, p[k] - h
        num = (olpe_oracle.build_analytical_model(hi, n, nsrc, bkgd_mode).astype(LD)
               - olpe_oracle.build_analytical_model(lo, n, nsrc, bkgd_mode)) / LD(hi[k] - lo[k])
        scale = float(np.abs(J[k]).max())
        assert scale > 0, k
        err = float(np.abs(J[k] - num).max())
        assert err <= 1e-6 * scale, (name, bkgd_mode, k, err / scale)


def _flat(nsrc):
    c = nr.columns(nsrc)
    v = np.zeros(c["P"], LD)
    v[c["amp"][0]] = v[c["amp"][1]] = v[c["off"]] = 1
    return v


def test_off_is_exactly_flat_in_two_source_mode_0_only():
    """J (e_amps + e_ampc + e_off) = 0 to rounding in the 2-source layout with bkgd_mode 0:
    `off` enters only as A_k - off.  Not in bkgd_mode 1 (off is the background too), not with
    three sources (p[12] is off and background; and the third amplitude moves alone)."""
    img, nsrc, params = fixture("c64")
    _, J = nr.jacobian(params[1], 64, 2, 0)
    d = np.tensordot(_flat(2), J, 1)
    assert float(np.abs(d).max()) <= 8 * 2.0 ** -64 * float(np.abs(J[[6, 7, 9]]).max())
    _, J1 = nr.jacobian(params[1], 64, 2, 1)
    assert float(np.abs(np.tensordot(_flat(2), J1, 1)).max()) > 0.5
    img3, _, params3 = fixture("c64_3")
    _, J3 = nr.jacobian(params3[1], 64, 3, 0)
    assert float(np.abs(np.tensordot(_flat(3), J3, 1)).max()) > 0.5


@pytest.mark.parametrize("n, nsrc", [(64, 2), (33, 2), (64, 3)])
def test_theta_column_is_exactly_zero_at_equal_sigmas(n, nsrc):
    """At the step-1 guess sigma_x = sigma_y in both sets: both theta columns of J are
    exactly 0 (Marquardt's diagonal damping is singular there), whatever theta is."""
    img, _ = synth.make_image(n, nsrc, 0)
    p = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
    c = nr.columns(nsrc)
    for th in (0.0, 0.3):
        p[c["narrow"][2]] = p[c["wide"][2]] = th
        _, J = nr.jacobian(p, n, nsrc, 0)
        assert not J[c["narrow"][2]].any() and not J[c["wide"][2]].any()
        assert np.abs(J[c["narrow"][0]]).max() > 0
    chi2, grad, jtj = nr.sums(p, *nr.frame(img), nsrc, 0)
    assert jtj[c["narrow"][2], c["narrow"][2]] == 0 and grad[c["wide"][2]] == 0
