"""olpefit_amd.mapfit on the CPU, with the long-double restatement of the Gauss-Newton sums
(tests/normal_restatement.py) in place of the device.  No GPU."""
import functools
import json

import numpy as np
import pytest

import normal_restatement as nr
from olpefit_amd import _lib, covariance, mapfit, synth, tune
from olpefit_amd.pipeline import initial_parameters

FRAMES = [(64, 2), (64, 3), (33, 2), (128, 3)]


@functools.lru_cache(maxsize=None)
def frame(n, nsrc):
    img, truth = synth.make_image(n, nsrc, 0)
    p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)[:-1]
    normal = nr.normal(nr.frame(img), nsrc, 0)
    return normal, p0, truth


@functools.lru_cache(maxsize=None)
def fitted(n, nsrc):
    normal, p0, _ = frame(n, nsrc)
    return mapfit.fit(normal, p0, nsrc)


@pytest.mark.parametrize("n, nsrc", FRAMES)
def test_fit_reaches_the_truths_chi2_within_20_steps(n, nsrc):
    """From the step-1 guess, chi^2 at the minimum <= chi^2(truth) within 20 accepted steps (a
    cap: the NumPy experiment over central differences took 5 on each of these frames)."""
    normal, p0, truth = frame(n, nsrc)
    res = fitted(n, nsrc)
    chi_truth = normal(truth[None])[0][0]
    print(n, nsrc, res.history[0], "truth", chi_truth, res.status, res.steps, res.evals)
    assert res.status == ["converged"]
    assert res.steps[0] <= 20
    assert res.chi2[0] <= chi_truth
    assert res.history[0][0] > 4 * chi_truth         # the guess is far from the mode
    assert np.all(np.diff(res.history[0]) < 0) and len(res.history[0]) == res.steps[0] + 1


def test_singular_start_does_not_raise():
    """At the guess sigma_x = sigma_y and theta = 0: the theta columns of J are exactly zero
    and, with `off` free, (amps, ampc, off) is flat; lambda diag(J^T J) would be singular."""
    normal, p0, _ = frame(33, 2)
    _, _, F = normal(p0[None])
    assert F[0][14, 14] == 0 and F[0][15, 15] == 0
    res = mapfit.fit(normal, p0, 2, free=np.ones(16, bool), max_steps=3)
    assert res.steps[0] == 3 and res.chi2[0] < res.history[0][0]


def test_fixed_parameters_are_bit_unchanged():
    normal, p0, _ = frame(33, 2)
    free = mapfit.free_mask(2, 0, fix=("bkgd", "theta", "theta2"))
    names = tune.param_names(2)
    fixed = [names.index(k) for k in ("bkgd", "theta", "theta2")]
    assert not free[fixed].any() and free.sum() == 13
    res = mapfit.fit(normal, p0, 2, free=free)
    assert np.array_equal(res.theta[0, fixed], p0[fixed]) and res.steps[0] > 0
    assert fitted(33, 2).theta[0, 9] == p0[9]            # `off`, fixed by default
    assert not np.array_equal(res.theta[0, free], p0[free])


def test_nan_chi2_is_a_rejected_step():
    """A trial whose chi^2 is NaN multiplies lambda by 10 like any rejected step: the fit goes
    on from the same point and ends at the same minimum."""
    normal, p0, _ = frame(33, 2)
    calls = []

    def poisoned(v):
        c, g, F = normal(v)
        calls.append(len(calls))
        if len(calls) in (2, 4):
            c, g, F = c * np.nan, g * np.nan, F * np.nan
        return c, g, F

    res, clean = mapfit.fit(poisoned, p0, 2), fitted(33, 2)
    assert res.status == ["converged"] and res.evals[0] >= clean.evals[0] + 2
    assert np.all(np.isfinite(res.history[0])) and np.all(np.diff(res.history[0]) < 0)
    assert abs(res.chi2[0] - clean.chi2[0]) <= 1e-6 * clean.chi2[0]
    allnan = mapfit.fit(lambda v: tuple(a * np.nan for a in normal(v)), p0, 2)
    assert allnan.status == ["stalled"] and allnan.steps[0] == 0
    assert np.array_equal(allnan.theta[0], p0)


def test_laplace_and_proposal_widths():
    """proposal_widths = 2.38 conditional_sigma of F^-1 where F is regular (in dex for the
    log-proposed ones); fixed parameters keep the default; with `off` free the flat direction
    (amps, ampc, off) is found and left out of the covariance."""
    normal, p0, _ = frame(33, 2)
    res = fitted(33, 2)
    lap = mapfit.laplace(normal, res.theta[0], 2, pixscale=9.95)
    free, th = lap.free, lap.theta_hat
    assert not lap.flat.any() and lap.eigenvalues.min() > 1e-3
    w = mapfit.proposal_widths(lap.F, th, 2, free)
    cs = covariance.conditional_sigma(lap.cov_u)["sigma_cond"]
    want = 2.38 * cs / np.where(mapfit._logmask(2)[free], np.log(10.0), 1.0)
    assert np.allclose(w[free], np.minimum(want, 1e300), rtol=1e-8)
    assert w[9] == tune.default_widths(2)[9]
    Fz = lap.F.copy()
    Fz[3, 3] = 0.0
    Fz[4, 4] = np.nan
    wz = mapfit.proposal_widths(Fz, th, 2, free)
    assert wz[3] == tune.default_widths(2)[3] and wz[4] == tune.default_widths(2)[4]
    tiny = mapfit.proposal_widths(lap.F * 1e-120, th, 2, free)
    assert tiny[6] == _lib.LOG_WIDTH_MAX
    # sigma of the offsets: the ellipse and the separation agree with the covariance
    e = lap.ellipses[0]
    assert e["semi_major"] >= e["semi_minor"] > 0 and e["semi_major_mas"] == e["semi_major"] * 9.95
    assert e["semi_minor"] <= lap.separation[0]["sigma_px"] <= e["semi_major"]
    full = mapfit.laplace(normal, res.theta[0], 2, free=np.ones(16, bool))
    assert full.flat.sum() == 1
    v = np.abs(full.flat_directions[0])
    u = np.zeros(16)
    u[[6, 7, 9]] = th[[6, 7, 9]] ** -1.0           # d theta = (1, 1, 1) in ln coordinates
    assert np.allclose(v, u / np.linalg.norm(u), atol=1e-6)


def test_laplace_draws_of_a_shard_equal_the_whole():
    normal, p0, _ = frame(33, 2)
    lap = mapfit.laplace(normal, fitted(33, 2).theta[0], 2)
    seeds = np.arange(100, 108)
    whole = mapfit.laplace_draws(lap, seeds, 1.0)
    assert np.array_equal(mapfit.laplace_draws(lap, seeds[2:5], 1.0), whole[2:5])
    assert np.array_equal(mapfit.laplace_draws(lap, seeds[5], 1.0)[0], whole[5])
    assert np.all(whole[:, 9] == lap.theta_hat[9])
    assert len({tuple(r) for r in whole}) == 8 and np.all(whole[:, [6, 7, 10, 11, 12, 13]] > 0)
    z = (mapfit.to_u(whole, 2)[:, lap.free] - mapfit.to_u(lap.theta_hat, 2)[lap.free]) / lap.sigma_u
    assert np.abs(z).max() < 6 and np.abs(z).max() > 0.5
    two = mapfit.laplace_draws(lap, seeds, 2.0)
    assert np.allclose(mapfit.to_u(two, 2) - mapfit.to_u(lap.theta_hat, 2),
                       2 * (mapfit.to_u(whole, 2) - mapfit.to_u(lap.theta_hat, 2)), atol=1e-12)
    # with a flat direction the factor leaves it out: in the scaled coordinates, where the
    # eigenvectors are orthogonal, the draws have no component along it
    full = mapfit.laplace(normal, lap.theta_hat, 2, free=np.ones(16, bool))
    d = mapfit.laplace_draws(full, seeds, 1.0)
    ds = (mapfit.to_u(d, 2) - mapfit.to_u(full.theta_hat, 2)) * full.scale
    along = ds @ full.eigenvectors[:, full.flat]
    assert np.abs(along).max() < 1e-9 * np.abs(ds).max()


def test_multi_start_finds_one_minimum():
    normal, p0, _ = frame(33, 2)
    ms = mapfit.multi_start(normal, p0, 2, starts=4, scatter=1.0, seed=3)
    assert ms.minima == 1 and ms.status == ["converged"] * 4
    assert np.all(np.diff(ms.chi2) >= 0)
    assert abs(ms.chi2[0] - fitted(33, 2).chi2[0]) <= 1e-9 * ms.chi2[0]
    a = mapfit.scattered_starts(p0, 2, 4, 1.0, 3)
    assert np.array_equal(a[0], p0) and not np.array_equal(a[1], p0)
    assert np.array_equal(a, mapfit.scattered_starts(p0, 2, 4, 1.0, 3))


def test_canonical_angles_leave_the_model_unchanged():
    """theta + pi / 2 with the sigmas exchanged (narrow set) and theta + pi (wide set, whose
    sigma_x is the background in bkgd_mode 0) are copies of the same model: chi^2 agrees to
    rounding and `canonical` maps the copy back."""
    normal, p0, truth = frame(33, 2)
    copy = truth.copy()
    copy[[10, 11]] = truth[[11, 10]]
    copy[14] = truth[14] + 5 * np.pi / 2
    copy[15] = truth[15] - 46 * np.pi
    c = normal(np.stack([truth, copy]))[0]
    assert abs(c[1] - c[0]) <= 1e-9 * c[0]
    back = mapfit.canonical(copy, 2, 0)
    assert np.array_equal(back[[10, 11]], truth[[10, 11]])
    assert np.allclose(back[[14, 15]], truth[[14, 15]], atol=1e-12)
    assert mapfit.same_minimum(copy, truth, 2, mapfit.default_free(2), 0)
    fixed = mapfit.free_mask(2, 0, fix=("theta",))
    assert mapfit.canonical(copy, 2, 0, fixed)[14] == copy[14]


def test_widths_file_round_trips_with_source_laplace(tmp_path):
    normal, p0, _ = frame(33, 2)
    res = fitted(33, 2)
    lap = mapfit.laplace(normal, res.theta[0], 2)
    w = mapfit.proposal_widths(lap.F, lap.theta_hat, 2, lap.free)
    path = tmp_path / "map_widths.json"
    doc = tune.save_widths(path, 2, w, "laplace")
    assert doc["source"] == "laplace" and "laplace" in tune.SOURCES
    assert np.array_equal(tune.load_widths(path, 2), w)
    assert tune.load_doc(path, 2)["source"] == "laplace"
    # map_fit.json: laplace_draws from the file equals laplace_draws from the result
    mp = tmp_path / "map_fit.json"
    mp.write_text(json.dumps(mapfit.map_doc(lap, res, 33, {"starts": 1})))
    back = mapfit.load_map(mp, 2, 0, 33)
    assert np.array_equal(back["theta_hat"], lap.theta_hat)
    assert np.array_equal(mapfit.laplace_draws(back, [1, 2]), mapfit.laplace_draws(lap, [1, 2]))
    for bad in ((3, 0, 33), (2, 1, 33), (2, 0, 64)):
        with pytest.raises(ValueError):
            mapfit.load_map(mp, *bad)
