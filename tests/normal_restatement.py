"""The Gauss-Newton normal equations (olpe_normal.hip, Sampler.normal_equations) restated in
np.longdouble from the model's formulas, not from the kernel: each Gaussian in its rotated
frame,  u = cos t dx + sin t dy,  v = -sin t dx + cos t dy,  q = u^2 / (2 sx^2) +
v^2 / (2 sy^2),  G = amp exp(-q),  so that

  dq/dx0 = -(u cos t / sx^2 - v sin t / sy^2)    dq/dsx = -u^2 / sx^3
  dq/dy0 = -(u sin t / sx^2 + v cos t / sy^2)    dq/dsy = -v^2 / sy^3
  dq/dt  = u v (1 / sx^2 - 1 / sy^2)             (du/dt = v, dv/dt = -u)

and dG/d. = -G dq/d., dG/damp = exp(-q).  The parameters enter as build_analytical_model
(apf_step2.py:106-124; 3body :106-125) has them: tot = A_s - off, wide = tot ratio at
(x_s + dx, y_s + dy) with set 2, narrow = tot - wide at (x_s, y_s) with set 1, plus the
background's parameter.  J[k] = dM / dtheta_k per pixel;  r = (D - M) / err,  Jw = J / err at
usable pixels, 0 at masked ones;  chi2 = sum r^2,  grad = Jw^T r,  jtj = Jw^T Jw.  No GPU,
nothing of the library.  `normal(frame, nsrc, bkgd_mode)` is the callable olpefit_amd.mapfit
takes in place of the device.
"""
import numpy as np

from lik_restatement import frame  # noqa: F401  (D, err, mask as olpe_create stages them)

LD = np.longdouble
U = 2.0 ** -53


def columns(nsrc):
    """Indices of the layout (apf_step2.py:108; 3body :108): centres, dx, dy, amplitudes,
    ratio, off, (sx, sy, theta) of the narrow and of the wide set, the lognorm list."""
    if nsrc == 2:
        return {"xy": [(0, 1), (2, 3)], "dx": 4, "dy": 5, "amp": [6, 7], "ratio": 8, "off": 9,
                "narrow": (10, 11, 14), "wide": (12, 13, 15), "P": 16,
                "log": (6, 7, 9, 10, 11, 12, 13)}
    if nsrc == 3:
        return {"xy": [(0, 1), (2, 3), (4, 5)], "dx": 6, "dy": 7, "amp": [8, 9, 10],
                "ratio": 11, "off": 12, "narrow": (13, 14, 17), "wide": (15, 16, 18), "P": 19,
                "log": (8, 9, 10, 12, 13, 14, 15, 16)}
    raise ValueError("nsrc must be 2 or 3")


def background_index(nsrc, bkgd_mode):
    return 12 if (nsrc == 3 or bkgd_mode == 0) else 9


def _gauss(x, y, x0, y0, sx, sy, th):
    """(E, dE/dx0, dE/dy0, dE/dsx, dE/dsy, dE/dth) of exp(-q), long double planes."""
    ct, st = np.cos(th), np.sin(th)
    dx, dy = x - x0, y - y0
    u = ct * dx + st * dy
    v = -st * dx + ct * dy
    ix, iy = 1 / (sx * sx), 1 / (sy * sy)
    with np.errstate(all="ignore"):
        E = np.exp(-(u * u * ix / 2 + v * v * iy / 2))
        qx0 = -(u * ct * ix - v * st * iy)
        qy0 = -(u * st * ix + v * ct * iy)
        qsx = -(u * u) * ix / sx
        qsy = -(v * v) * iy / sy
        qth = (u * v) * (ix - iy)
        return E, -E * qx0, -E * qy0, -E * qsx, -E * qsy, -E * qth


def jacobian(p, n, nsrc, bkgd_mode=0):
    """(M [n, n], J [P, n, n]) in long double: the model and dM / dtheta_k."""
    c = columns(nsrc)
    p = np.asarray(p, dtype=np.float64)[:c["P"]].astype(LD)
    yy, xx = np.mgrid[:n, :n]
    x, y = xx.astype(LD), yy.astype(LD)
    M = np.zeros((n, n), LD)
    J = np.zeros((c["P"], n, n), LD)
    ratio, off = p[c["ratio"]], p[c["off"]]
    n_sx, n_sy, n_th = c["narrow"]
    w_sx, w_sy, w_th = c["wide"]
    for (kx, ky), ka in zip(c["xy"], c["amp"]):
        tot = p[ka] - off
        wide, narrow = tot * ratio, tot - tot * ratio
        Ew = _gauss(x, y, p[kx] + p[c["dx"]], p[ky] + p[c["dy"]], p[w_sx], p[w_sy], p[w_th])
        En = _gauss(x, y, p[kx], p[ky], p[n_sx], p[n_sy], p[n_th])
        with np.errstate(all="ignore"):
            M += wide * Ew[0] + narrow * En[0]
            J[kx] += wide * Ew[1] + narrow * En[1]
            J[ky] += wide * Ew[2] + narrow * En[2]
            J[c["dx"]] += wide * Ew[1]
            J[c["dy"]] += wide * Ew[2]
            dtot = ratio * Ew[0] + (1 - ratio) * En[0]
            J[ka] += dtot
            J[c["off"]] -= dtot
            J[c["ratio"]] += tot * (Ew[0] - En[0])
            for k, q in zip(c["wide"], (3, 4, 5)):
                J[k] += wide * Ew[q]
            for k, q in zip(c["narrow"], (3, 4, 5)):
                J[k] += narrow * En[q]
    kb = background_index(nsrc, bkgd_mode)
    M += p[kb]
    J[kb] += 1
    return M, J


def weighted(p, D, err, mask, nsrc, bkgd_mode=0):
    """(r [n, n], Jw [P, n, n]) in long double, exact zeros at masked pixels."""
    n = D.shape[0]
    M, J = jacobian(p, n, nsrc, bkgd_mode)
    w = np.where(mask, LD(0), 1 / np.where(mask, 1.0, err).astype(LD))
    with np.errstate(all="ignore"):
        r = np.where(mask, LD(0), (D.astype(LD) - M) * w)
        Jw = np.where(mask[None], LD(0), J * w[None])
    return r, Jw


def sums(p, D, err, mask, nsrc, bkgd_mode=0):
    """(chi2, grad [P], jtj [P, P]) in long double."""
    r, Jw = weighted(p, D, err, mask, nsrc, bkgd_mode)
    A = Jw.reshape(Jw.shape[0], -1)
    with np.errstate(all="ignore"):
        return (r * r).sum(), A @ r.ravel(), A @ A.T


def normal(fr, nsrc, bkgd_mode=0):
    """`normal(vecs) -> (chi2 [W], grad [W, P], jtj [W, P, P])` in float64 on the frame
    fr = (D, err, mask), as Sampler.normal_equations returns them; a vector with a
    non-finite sum anywhere is NaN throughout."""
    D, err, mask = fr
    P = columns(nsrc)["P"]

    def f(vecs):
        v = np.atleast_2d(np.asarray(vecs, dtype=np.float64))
        chi2, grad, jtj = np.empty(len(v)), np.empty((len(v), P)), np.empty((len(v), P, P))
        for i, p in enumerate(v):
            c, g, a = sums(p, D, err, mask, nsrc, bkgd_mode)
            c, g, a = np.float64(c), g.astype(np.float64), a.astype(np.float64)
            if not (np.isfinite(c) and np.isfinite(g).all() and np.isfinite(a).all()):
                c, g, a = np.nan, np.full(P, np.nan), np.full((P, P), np.nan)
            chi2[i], grad[i], jtj[i] = c, g, a
        return chi2, grad, jtj
    return f
