"""Best fit and Laplace approximation from the Gauss-Newton normal equations.

The sampler has no way to find the posterior mode: every walker starts at the step-1 guess
and walks there by single-parameter Metropolis steps.  With the sums  chi^2 = sum r^2,
g = J^T r  and  J^T J  of the model at a parameter vector (r = (D - M) / err, J = (dM /
dtheta) / err; ``Sampler.normal_equations`` on the device) the mode is a Levenberg-Marquardt
fit of a few steps, and around it the Fisher matrix F = J^T J gives the Laplace
approximation: a covariance, the proposal widths 2.38 / sqrt(F_jj) (``covariance``'s
conditional width is exactly 1 / sqrt(F_jj)) and an equilibrium start for the ensemble.

Everything here is NumPy on 16 x 16 or 19 x 19 matrices.  Every function takes a callable
``normal(vecs [W, P]) -> (chi2 [W], grad [W, P], jtj [W, P, P])``, so the module runs
without a GPU on any restatement of the sums (tests/normal_restatement.py).

Coordinates.  The fit works in u: u_k = ln theta_k for the log-proposed parameters
(``tune.log_params``), theta_k otherwise; g and J^T J are scaled by theta_k on those rows
and columns.  Two properties of the model shape the algebra:

* in the 2-source layout with bkgd_mode 0, ``off`` (p[9]) enters only as A_k - off, so
  (amps, ampc, off) ~ (1, 1, 1) is exactly flat: ``off`` is fixed by default;
* at sigma_x = sigma_y (the step-1 guess) the theta column of J is exactly zero, so
  Marquardt's lambda diag(J^T J) damping is singular there: the matrix is scaled to a unit
  diagonal with a zero diagonal replaced by 1, and lambda I is added in the scaled space.
"""
from __future__ import annotations

import numpy as np

from . import _lib, covariance, tune

FLAT_RTOL = 1e-10          # eigenvalues of the scaled F below this x the largest are flat
LAMBDA_MAX = 1e12
SAME_MINIMUM = 1e-6


def _p(nsrc: int) -> int:
    return tune.default_widths(nsrc).size


def default_free(nsrc: int, bkgd_mode: int = 0) -> np.ndarray:
    """Every parameter but ``off`` (p[9]) of the 2-source layout in bkgd_mode 0."""
    free = np.ones(_p(nsrc), dtype=bool)
    if nsrc == 2 and bkgd_mode == 0:
        free[9] = False
    return free


def free_mask(nsrc: int, bkgd_mode: int = 0, free=None, fix=()) -> np.ndarray:
    """``free`` (default ``default_free``) with the parameters named in ``fix`` taken out."""
    m = default_free(nsrc, bkgd_mode) if free is None else np.array(free, dtype=bool)
    if m.shape != (_p(nsrc),):
        raise ValueError(f"the free mask must have {_p(nsrc)} entries")
    names = tune.param_names(nsrc)
    for name in fix:
        if name not in names:
            raise ValueError(f"no parameter {name!r}; the names are {names}")
        m[names.index(name)] = False
    return m


def _logmask(nsrc: int) -> np.ndarray:
    m = np.zeros(_p(nsrc), dtype=bool)
    m[list(tune.log_params(nsrc))] = True
    return m


def _vecs(p, nsrc: int) -> np.ndarray:
    P = _p(nsrc)
    v = np.atleast_2d(np.asarray(p, dtype=np.float64))
    if v.ndim != 2 or v.shape[1] not in (P, P + 1):
        raise ValueError(f"parameter vectors must have {P} or {P + 1} entries")
    return np.array(v[:, :P])


def to_u(theta, nsrc: int) -> np.ndarray:
    theta = np.asarray(theta, dtype=np.float64)
    lg = _logmask(nsrc)
    if np.any(theta[..., lg] <= 0.0):
        raise ValueError("a log-proposed parameter is not > 0")
    u = np.array(theta)
    u[..., lg] = np.log(theta[..., lg])
    return u


def from_u(u, nsrc: int) -> np.ndarray:
    lg = _logmask(nsrc)
    theta = np.array(u, dtype=np.float64)
    with np.errstate(over="ignore"):
        theta[..., lg] = np.exp(theta[..., lg])
    return theta


def _scaled(F, theta, nsrc: int, free):
    """(Fs, d, Fu): J^T J in u over the free parameters, its unit-diagonal scaling
    Fs = Fu / (d d^T) with d = sqrt(diag Fu), a zero or non-finite diagonal replaced by 1."""
    sc = np.where(_logmask(nsrc), theta, 1.0)[free]
    Fu = np.asarray(F, dtype=np.float64)[np.ix_(free, free)] * np.outer(sc, sc)
    dg = np.diag(Fu)
    ok = np.isfinite(dg) & (dg > 0.0)
    d = np.sqrt(np.where(ok, dg, 1.0))
    return Fu / np.outer(d, d), d, Fu


def _step(g, F, theta, lam: float, nsrc: int, free) -> np.ndarray:
    """The damped Gauss-Newton step du over the free parameters."""
    sc = np.where(_logmask(nsrc), theta, 1.0)[free]
    Fs, d, _ = _scaled(F, theta, nsrc, free)
    b = (np.asarray(g, dtype=np.float64)[free] * sc) / d
    A = Fs + lam * np.eye(len(d))
    try:
        x = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        x = np.linalg.lstsq(A, b, rcond=None)[0]
    return x / d


class Fit(dict):
    """The result of ``fit``: a dict whose keys read as attributes."""
    __getattr__ = dict.__getitem__


def fit(normal, p0, nsrc: int, bkgd_mode: int = 0, free=None, max_steps: int = 50,
        ftol: float = 1e-9, lam0: float = 1e-3) -> Fit:
    """Levenberg-Marquardt from the starts ``p0`` [S, P] (or one [P]), all still-active starts
    in one ``normal`` call per iteration.  lambda starts at ``lam0``; a step that does not
    lower chi^2, or whose chi^2 is not finite, is rejected and multiplies lambda by 10, an
    accepted one divides it by 10.  A start stops ``converged`` when an accepted step lowers
    chi^2 by less than ``ftol`` chi^2, ``stalled`` when lambda passes 1e12 (or its first
    chi^2 is not finite), ``max_steps`` after that many accepted steps.  A parameter outside
    ``free`` keeps its p0 value bit for bit; amplitude-like partners of a fixed ``off`` are
    relative to it (``amp_minus_off``).

    Returns theta [S, P], chi2 [S], steps (accepted) [S], evals [S], status [S], history
    (chi^2 at the start and after each accepted step) per start, free, nsrc, bkgd_mode."""
    theta = _vecs(p0, nsrc)
    S = theta.shape[0]
    free = free_mask(nsrc, bkgd_mode, free)
    lg = _logmask(nsrc)
    if np.any(theta[:, lg & free] <= 0.0):
        raise ValueError("a free log-proposed parameter is not > 0")
    chi2, g, F = (np.array(a, dtype=np.float64) for a in normal(theta))
    lam = np.full(S, float(lam0))
    steps = np.zeros(S, dtype=np.int64)
    evals = np.ones(S, dtype=np.int64)
    status = np.array(["max_steps"] * S, dtype=object)
    history = [[float(c)] for c in chi2]
    active = np.isfinite(chi2) & (max_steps > 0)
    status[~np.isfinite(chi2)] = "stalled"
    while active.any():
        idx = np.flatnonzero(active)
        trial = theta[idx].copy()
        for q, s in enumerate(idx):
            du = _step(g[s], F[s], theta[s], lam[s], nsrc, free)
            with np.errstate(over="ignore", invalid="ignore"):
                new = np.where(lg[free], theta[s, free] * np.exp(du), theta[s, free] + du)
            trial[q, free] = new
        c2, g2, F2 = (np.asarray(a, dtype=np.float64) for a in normal(trial))
        evals[idx] += 1
        for q, s in enumerate(idx):
            if np.isfinite(c2[q]) and np.isfinite(trial[q]).all() and c2[q] < chi2[s]:
                drop, before = chi2[s] - c2[q], chi2[s]
                theta[s], chi2[s], g[s], F[s] = trial[q], c2[q], g2[q], F2[q]
                lam[s] /= 10.0
                steps[s] += 1
                history[s].append(float(c2[q]))
                if drop < ftol * before:
                    status[s], active[s] = "converged", False
                elif steps[s] >= max_steps:
                    active[s] = False
            else:
                lam[s] *= 10.0
                if lam[s] > LAMBDA_MAX:
                    status[s], active[s] = "stalled", False
    return Fit(theta=theta, chi2=chi2, steps=steps, evals=evals, status=list(status),
               history=history, free=free, nsrc=int(nsrc), bkgd_mode=int(bkgd_mode))


def amp_minus_off(theta, nsrc: int) -> np.ndarray:
    """A_k - off per source: what the model sees of the amplitudes."""
    theta = np.asarray(theta, dtype=np.float64)
    amp, off = ((6, 7), 9) if nsrc == 2 else ((8, 9, 10), 12)
    return theta[..., list(amp)] - theta[..., [off]]


def _source_columns(nsrc: int):
    return [(2 * s, 2 * s + 1) for s in range(nsrc)]


def laplace(normal, theta_hat, nsrc: int, bkgd_mode: int = 0, free=None, pixscale=None) -> Fit:
    """The Laplace approximation at ``theta_hat`` [P]: F = J^T J over the free parameters in
    u-coordinates.  ``eigenvalues`` are those of the unit-diagonal-scaled F (ascending, with
    ``eigenvectors`` in its columns); the ones below 1e-10 of the largest are ``flat`` and
    the covariance is the pseudo-inverse off them.  Returns theta_hat, chi2, free, F (raw
    parameters, [P, P] as the device gives it), F_u / cov_u / sigma_u [nfree...] in u,
    cov / sigma / corr [P...] in the raw parameters (linearised: sigma_theta = theta sigma_u
    for a log-proposed one; zero rows for fixed parameters), ``flat_directions`` (unit
    vectors over the free parameters in u), ``ellipses``: per companion
    ``covariance.error_ellipse`` of its offset from source 0 in the detector frame, and
    ``separation`` / ``position_angle`` with their sigma (px, mas with ``pixscale``; degrees
    from +x towards +y)."""
    th = _vecs(theta_hat, nsrc)[0]
    free = free_mask(nsrc, bkgd_mode, free)
    P = th.size
    chi2, _, F = normal(th[None])
    F = np.array(F[0], dtype=np.float64)
    Fs, d, Fu = _scaled(F, th, nsrc, free)
    w, V = np.linalg.eigh(0.5 * (Fs + Fs.T))
    flat = ~(w > FLAT_RTOL * w.max()) if np.isfinite(w).all() and w.max() > 0 else np.ones(len(w), bool)
    keep = ~flat
    cov_s = (V[:, keep] / w[keep]) @ V[:, keep].T
    cov_u = cov_s / np.outer(d, d)
    sigma_u = np.sqrt(np.clip(np.diag(cov_u), 0.0, None))
    sc = np.where(_logmask(nsrc), th, 1.0)
    cov = np.zeros((P, P))
    cov[np.ix_(free, free)] = cov_u * np.outer(sc[free], sc[free])
    sigma = np.sqrt(np.clip(np.diag(cov), 0.0, None))
    with np.errstate(invalid="ignore", divide="ignore"):
        corr = cov / np.outer(sigma, sigma)
    flat_dirs = []
    for k in np.flatnonzero(flat):
        v = V[:, k] / d
        flat_dirs.append(v / np.linalg.norm(v))
    cols = _source_columns(nsrc)
    ellipses, sep, pa = [], [], []
    for b in cols[1:]:
        ellipses.append(covariance.error_ellipse(cov, cols[0], b, pixscale))
        ox, oy = th[b[0]] - th[cols[0][0]], th[b[1]] - th[cols[0][1]]
        rho = float(np.hypot(ox, oy))
        c2 = ellipses[-1]["cov2"]
        jr = np.array([ox, oy]) / rho
        ja = np.array([-oy, ox]) / (rho * rho)
        item = {"px": rho, "sigma_px": float(np.sqrt(jr @ c2 @ jr))}
        if pixscale is not None:
            item["mas"], item["sigma_mas"] = rho * pixscale, item["sigma_px"] * pixscale
        sep.append(item)
        pa.append({"deg": float(np.degrees(np.arctan2(oy, ox)) % 360.0),
                   "sigma_deg": float(np.degrees(np.sqrt(ja @ c2 @ ja)))})
    return Fit(theta_hat=th, chi2=float(chi2[0]), free=free, nsrc=int(nsrc),
               bkgd_mode=int(bkgd_mode), F=F, F_u=Fu, scale=d, eigenvalues=w, eigenvectors=V,
               flat=flat, flat_directions=flat_dirs, cov_u=cov_u, sigma_u=sigma_u, cov=cov,
               sigma=sigma, corr=corr, ellipses=ellipses, separation=sep, position_angle=pa,
               amp_minus_off=amp_minus_off(th, nsrc))


def proposal_widths(F, theta_hat, nsrc: int, free=None, scale: float = 2.38) -> np.ndarray:
    """Proposal widths [P] from the Fisher matrix F [P, P] of the raw parameters at
    ``theta_hat``: a proposed parameter gets ``scale`` / sqrt(F_jj), a log-proposed one the
    same in u-coordinates (F_jj theta_j^2) divided by ln 10: dex.  Where F_jj is zero or not
    finite, or the parameter is fixed, the default stays.  Clipped to what ``set_widths``
    accepts (log-proposed: ``_lib.LOG_WIDTH_MAX`` dex)."""
    w = tune.default_widths(nsrc)
    th = _vecs(theta_hat, nsrc)[0]
    dg = np.diag(np.asarray(F, dtype=np.float64))
    free = np.ones(w.size, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    lg = _logmask(nsrc)
    for j in range(w.size):
        if not (free[j] and np.isfinite(dg[j]) and dg[j] > 0.0):
            continue
        fu = dg[j] * th[j] * th[j] if lg[j] else dg[j]
        if not (np.isfinite(fu) and fu > 0.0):
            continue
        v = scale / np.sqrt(fu)
        if lg[j]:
            v = min(v / np.log(10.0), _lib.LOG_WIDTH_MAX)
        if np.isfinite(v) and v > 0.0:
            w[j] = v
    return w


def scattered_starts(p0, nsrc: int, starts: int, scatter: float, seed: int, free=None):
    """[starts, P]: p0 itself, then p0 + ``scatter`` x the default widths x standard normals
    (in ln-space, the width in dex x ln 10, for log-proposed parameters), RandomState(seed);
    fixed parameters stay."""
    p0 = _vecs(p0, nsrc)[0]
    free = np.ones(p0.size, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    lg = _logmask(nsrc)
    wd = tune.default_widths(nsrc) * np.where(lg, np.log(10.0), 1.0)
    z = np.random.RandomState(seed).standard_normal((max(int(starts), 1), p0.size))
    z[0] = 0.0
    z[:, ~free] = 0.0
    step = scatter * wd * z
    return np.where(lg, p0 * np.exp(step), p0 + step)


def canonical(theta, nsrc: int, bkgd_mode: int = 0, free=None) -> np.ndarray:
    """``theta`` with each shape set's angle brought back to its principal value.  A Gaussian
    is unchanged by theta -> theta + pi, and by theta -> theta + pi / 2 with sigma_x and
    sigma_y exchanged, and a fit that starts where sigma_x = sigma_y (no gradient in theta)
    may land on any of these copies: theta goes to [-pi / 4, pi / 4] with the sigmas swapped
    for an odd number of quarter turns.  The wide set of the 2-source layout in bkgd_mode 0
    only takes whole half turns: its sigma_x is the background too.  A set with a fixed
    member is left as it is."""
    th = np.array(theta, dtype=np.float64)
    sets = ((10, 11, 14), (12, 13, 15)) if nsrc == 2 else ((13, 14, 17), (15, 16, 18))
    for sx, sy, t in sets:
        if free is not None and not np.asarray(free, dtype=bool)[[sx, sy, t]].all():
            continue
        if nsrc == 2 and bkgd_mode == 0 and sx == 12:
            th[..., t] -= np.pi * np.round(th[..., t] / np.pi)
            continue
        k = np.round(th[..., t] / (np.pi / 2))
        th[..., t] -= (np.pi / 2) * k
        odd = (k % 2) != 0
        a, b = th[..., sx].copy(), th[..., sy].copy()
        th[..., sx], th[..., sy] = np.where(odd, b, a), np.where(odd, a, b)
    return th


def same_minimum(a, b, nsrc: int, free, bkgd_mode: int = 0) -> bool:
    """Every free u of the two (``canonical``) vectors within 1e-6 max(1, |u|)."""
    a, b = canonical(a, nsrc, bkgd_mode, free), canonical(b, nsrc, bkgd_mode, free)
    ua, ub = to_u(a, nsrc)[free], to_u(b, nsrc)[free]
    return bool(np.all(np.abs(ua - ub) < SAME_MINIMUM * np.maximum(1.0, np.abs(ua))))


def multi_start(normal, p0, nsrc: int, starts: int = 8, scatter: float = 1.0, seed: int = 0,
                bkgd_mode: int = 0, free=None, **kw) -> Fit:
    """``fit`` from ``scattered_starts``; the fits sorted by chi^2 (not finite last) and
    ``minima``: the number of distinct minima among the converged ones, two fits being the
    same minimum when every free u differs by less than 1e-6 max(1, |u|), the angles
    compared at their principal values (``canonical``)."""
    free = free_mask(nsrc, bkgd_mode, free)
    res = fit(normal, scattered_starts(p0, nsrc, starts, scatter, seed, free), nsrc, bkgd_mode,
              free, **kw)
    order = np.argsort(np.where(np.isfinite(res.chi2), res.chi2, np.inf), kind="stable")
    out = Fit(res)
    for k in ("theta", "chi2", "steps", "evals"):
        out[k] = res[k][order]
    out["status"] = [res.status[i] for i in order]
    out["history"] = [res.history[i] for i in order]
    out["order"] = order
    distinct = []
    for i in range(len(order)):
        if out.status[i] != "converged":
            continue
        if not any(same_minimum(out.theta[i], out.theta[j], nsrc, free, bkgd_mode)
                   for j in distinct):
            distinct.append(i)
    out["distinct"] = distinct
    out["minima"] = len(distinct)
    return out


def laplace_draws(lap, seeds, inflate: float = 1.0) -> np.ndarray:
    """Equilibrium starts [W, P] from a ``laplace`` result: walker w starts at theta_hat +
    inflate L z_w in u-coordinates, L the Cholesky factor of the covariance (with flat
    directions: V diag(1 / sqrt(lambda)) over the others, which has the same L L^T), z_w
    standard normals from RandomState((seed_w + 0x9E3779B9) & 0xFFFFFFFF): a stream per
    walker, so a shard's walkers start where the whole ensemble's do."""
    th, free, nsrc = lap["theta_hat"], np.asarray(lap["free"], dtype=bool), lap["nsrc"]
    cov_u = np.asarray(lap["cov_u"], dtype=np.float64)
    flat = np.asarray(lap["flat"], dtype=bool)
    if flat.any():
        keep = ~flat
        w, V = np.asarray(lap["eigenvalues"]), np.asarray(lap["eigenvectors"])
        L = np.zeros_like(cov_u)
        L[:, :keep.sum()] = (V[:, keep] / np.sqrt(w[keep])) / np.asarray(lap["scale"])[:, None]
    else:
        L = np.linalg.cholesky(0.5 * (cov_u + cov_u.T))
    lg = _logmask(nsrc)[free]
    seeds = np.atleast_1d(np.asarray(seeds, dtype=np.uint64))
    out = np.tile(np.asarray(th, dtype=np.float64), (seeds.size, 1))
    for k, s in enumerate(seeds):
        z = np.random.RandomState((int(s) + 0x9E3779B9) & 0xFFFFFFFF).standard_normal(L.shape[0])
        du = inflate * (L @ z)
        out[k, free] = np.where(lg, th[free] * np.exp(du), th[free] + du)
    return out


# -- the fit's file (apf_map.py writes it, apf_step2.py -i map reads it) ---------------
MAP_FORMAT = "olpefit-map-1"


def map_doc(lap, res, side: int, settings: dict) -> dict:
    """The content of map_fit.json: the best fit ``res`` (row 0 of a ``fit`` / ``multi_start``
    result) and its Laplace approximation ``lap``."""
    ls = lambda a: np.asarray(a, dtype=np.float64).tolist()    # noqa: E731
    return {"format": MAP_FORMAT, "nsrc": int(lap["nsrc"]), "bkgd_mode": int(lap["bkgd_mode"]),
            "side": int(side), "names": tune.param_names(lap["nsrc"]),
            "theta_hat": ls(lap["theta_hat"]), "chi2": float(lap["chi2"]),
            "status": res["status"][0], "steps": int(res["steps"][0]),
            "evals": int(res["evals"][0]), "history": [float(v) for v in res["history"][0]],
            "free": [bool(v) for v in lap["free"]], "F": ls(lap["F"]), "cov": ls(lap["cov"]),
            "cov_u": ls(lap["cov_u"]), "scale": ls(lap["scale"]), "sigma": ls(lap["sigma"]),
            "corr": ls(np.nan_to_num(lap["corr"])), "eigenvalues": ls(lap["eigenvalues"]),
            "eigenvectors": ls(lap["eigenvectors"]), "flat": [bool(v) for v in lap["flat"]],
            "minima": int(res.get("minima", 1)), "settings": settings}


def load_map(path, nsrc: int, bkgd_mode: int, side: int) -> dict:
    """map_fit.json as ``laplace_draws`` takes it (arrays restored).  ValueError when the
    file's nsrc, bkgd_mode or side differ from the run's."""
    import json
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or doc.get("format") != MAP_FORMAT:
        raise ValueError(f"{path}: not a map-fit file ({MAP_FORMAT})")
    for key, want in (("nsrc", nsrc), ("bkgd_mode", bkgd_mode), ("side", side)):
        if doc.get(key) != want:
            raise ValueError(f"{path}: written for {key} {doc.get(key)}, this run has {key} {want}")
    for key in ("theta_hat", "F", "cov", "cov_u", "scale", "sigma", "eigenvalues",
                "eigenvectors"):
        doc[key] = np.array(doc[key], dtype=np.float64)
    doc["free"] = np.array(doc["free"], dtype=bool)
    doc["flat"] = np.array(doc["flat"], dtype=bool)
    if doc["theta_hat"].shape != (_p(nsrc),) or not np.isfinite(doc["theta_hat"]).all():
        raise ValueError(f"{path}: theta_hat is not {_p(nsrc)} finite values")
    return doc
