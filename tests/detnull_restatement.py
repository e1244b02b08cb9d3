"""The null maps of the false-alarm calibration (olpe_detnull.hip, olpefit_amd/detect_null.py)
restated in np.longdouble over detect_restatement (Frame, table, psi and its bound dK):

    y_r,i = eps_r,i (1 / err_i) with the 1 / err rounded to double, 0 if masked
    N_r(c) = sum_i K_i(c) y_r,i,  Q(c) = sum_i w_i K_i(c)^2,  snr_r(c) = scale(c) N_r(c) / sqrt(Q(c))

at chosen candidates, and the bound the GPU tests hold the device to, derived as in
test_gpu_detect's docstring (u = 2^-53):
  y     the product and the rounded 1 / err 2 u, and the deviate itself within the project's
        gauss tolerance 3.2e-15 (test_gpu_parity) when the device draws it:
        |dy| <= (3.2e-15 + 2 u) |y|.
  N     |dN| <= sum (|y| dK + 3 u |y| K) + n^2 u sum |y K| + sum K |dy|; n^2 u is the worst case
        of ANY order of the n^2 fused additions, so it does not depend on how the device
        tiles the sum.
  Q     |dQ| <= sum 2 w K dK + (n^2 + 4) u Q, as in detect_restatement.sample.
  snr   <= scale (dN / sqrt(Q) / (1 - dQ / Q) + |N / sqrt(Q)| (dQ / 2Q / (1 - dQ / Q) + 3 u))
        + u |snr|: the step from N and Q as there, one more rounding for the scale.
No GPU, nothing of the library.
"""
import numpy as np

import detect_restatement as dr

LD = np.longdouble
U = dr.U
GAUSS_TOL = 3.2e-15


def inv_err(fr):
    """The rounded 1 / err the context stages, 0 where masked (double [n][n])."""
    with np.errstate(all="ignore"):
        return np.where(fr.mask, 0.0, 1.0 / np.where(fr.mask, 1.0, fr.err))


def maps_at(fr, row, nsrc, cand, eps, oversample=1, scale=None):
    """eps [R][n][n] -> {"snr" long double [R][C], "bsnr" double [R][C]} at the candidates
    `cand` [C][2] (jy, jx); scale [g][g] or None.  NaN where Q = 0."""
    n = fr.n
    g = oversample * (n - 1) + 1
    ie = inv_err(fr)
    y = np.asarray(eps, dtype=np.float64).astype(LD) * ie.astype(LD)      # [R][n][n]
    yf = np.abs(y).astype(np.float64)
    dy = (GAUSS_TOL + 2 * U) * yf
    R, C = y.shape[0], len(cand)
    snr, bsnr = np.zeros((R, C), LD), np.zeros((R, C))
    tabs = {}
    for k, (jy, jx) in enumerate(cand):
        cy, py = divmod(int(jy), oversample)
        cx, px = divmod(int(jx), oversample)
        if (py, px) not in tabs:
            tabs[(py, px)] = dr.table(row, nsrc, n, oversample, (py, px))
        T, dT = tabs[(py, px)]
        K = T[n - 1 - cy:2 * n - 1 - cy, n - 1 - cx:2 * n - 1 - cx]
        dK = dT[n - 1 - cy:2 * n - 1 - cy, n - 1 - cx:2 * n - 1 - cx]
        Kf = np.abs(K).astype(np.float64)
        N = (y * K).sum(axis=(1, 2))
        Q = (fr.w * K * K).sum()
        dN = (yf * dK + 3 * U * yf * Kf + Kf * dy).sum(axis=(1, 2)) \
            + n * n * U * (yf * Kf).sum(axis=(1, 2))
        dQ = float((2 * fr.wf * Kf * dK).sum() + (n * n + 4) * U * (fr.wf * Kf * Kf).sum())
        sc = 1.0 if scale is None else float(np.asarray(scale).reshape(g, g)[jy, jx])
        with np.errstate(all="ignore"):
            Qf = float(Q)
            rq = dQ / Qf
            grow = 1.0 / (1.0 - rq)
            raw = N / np.sqrt(Q)
            snr[:, k] = LD(sc) * raw
            bsnr[:, k] = sc * (dN / np.sqrt(Qf) * grow
                               + np.abs(raw).astype(np.float64) * (0.5 * rq * grow + 3 * U)) \
                + U * np.abs(snr[:, k]).astype(np.float64)
        if Q == 0:
            snr[:, k] = LD("nan")
    return {"snr": snr, "bsnr": bsnr}
