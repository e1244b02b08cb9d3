"""The definitions of the companion detection map (olpe_detect.hip, olpefit_amd/detect.py)
restated in np.longdouble over the oracle's build_analytical_model and lik_restatement.frame:

    psi(u, v) = (1 - q) g1(u, v) + q g2(u - dx, v - dy),  g_k = exp(-((a_k u^2) + (b_k u) v + c_k v^2))
    z_i = w_i (D_i - M_i),  w_i = (1 / err_i)^2 with the 1 / err rounded to double, 0 if masked
    K_i(c) = psi(x_i - x_c, y_i - y_c),  N = sum z K,  Q = sum w K^2
    A = N / Q,  sigma_A = 1 / sqrt(Q),  snr = N / sqrt(Q)

evaluated at a chosen subset of the candidate lattice (a full long-double map over an
ensemble costs minutes), and finalize's planes from them.  The lattice offsets x_i - x_c are
multiples of 1 / oversample, so psi is evaluated once per distinct offset and read per
candidate: the same arguments, no approximation.  Also the error bounds the GPU tests hold
the device to, derived in test_gpu_detect's docstring.  No GPU, nothing of the library.
"""
import numpy as np

import lik_restatement as lr
from oracle import olpe_oracle

LD = np.longdouble
U = 2.0 ** -53
frame = lr.frame


def shape_of(row, nsrc):
    """(q, dx, dy, (sx, sy, th) narrow, (sx, sy, th) wide) of a parameter row."""
    r = np.asarray(row, dtype=np.float64)
    if nsrc == 2:
        return r[8], r[4], r[5], (r[10], r[11], r[14]), (r[12], r[13], r[15])
    return r[11], r[6], r[7], (r[13], r[14], r[17]), (r[15], r[16], r[18])


def sources_of(row, nsrc):
    r = np.asarray(row, dtype=np.float64)
    return [(r[2 * s], r[2 * s + 1]) for s in range(nsrc)]


def coef(sx, sy, th):
    """Gaussian2D.evaluate's a, b, c in long double."""
    sx, sy, th = LD(sx), LD(sy), LD(th)
    c2, s2, s2t = np.cos(th) ** 2, np.sin(th) ** 2, np.sin(2 * th)
    return (LD(0.5) * (c2 / sx ** 2 + s2 / sy ** 2), LD(0.5) * (s2t / sx ** 2 - s2t / sy ** 2),
            LD(0.5) * (s2 / sx ** 2 + c2 / sy ** 2))


def abs_coef(sx, sy, th):
    """The same with every term's absolute value: what a coefficient's rounding scales with."""
    c2, s2, s2t = np.cos(th) ** 2, np.sin(th) ** 2, abs(np.sin(2 * th))
    return (0.5 * (c2 / sx ** 2 + s2 / sy ** 2), 0.5 * (s2t / sx ** 2 + s2t / sy ** 2),
            0.5 * (s2 / sx ** 2 + c2 / sy ** 2))


# roundings that reach a Gaussian's argument, in units of u times its absolute-valued terms:
# a coefficient (cos or sin 1 ulp, a square, two divisions by squares, a sum, the half) 4, the
# offset's subtraction, square or product and the product with the coefficient 4, the two
# additions 2
ARG_U = 10.0
# exp_neg 2 ulp, then the weights (1 - q), q, two products and the sum
VAL_U = 5.0


def psi(row, nsrc, u, v):
    """(psi, dpsi): the unit PSF at offsets u, v (long double arrays) and how far a double
    evaluation in the project's operation order may lie from it."""
    q, dx, dy, nar, wid = shape_of(row, nsrc)
    u, v = np.asarray(u, dtype=LD), np.asarray(v, dtype=LD)
    a1, b1, c1 = coef(*nar)
    a2, b2, c2 = coef(*wid)
    u2, v2 = u - LD(dx), v - LD(dy)
    g1 = (1 - LD(q)) * np.exp(-(a1 * u * u + b1 * u * v + c1 * v * v))
    g2 = LD(q) * np.exp(-(a2 * u2 * u2 + b2 * u2 * v2 + c2 * v2 * v2))
    A1, B1, C1 = abs_coef(*nar)
    A2, B2, C2 = abs_coef(*wid)
    uf, vf, u2f, v2f = (np.abs(x).astype(np.float64) for x in (u, v, u2, v2))
    t1 = A1 * uf * uf + B1 * uf * vf + C1 * vf * vf
    t2 = A2 * u2f * u2f + B2 * u2f * v2f + C2 * v2f * v2f
    d = U * ((VAL_U + ARG_U * t1) * np.abs(g1).astype(np.float64)
             + (VAL_U + ARG_U * t2) * np.abs(g2).astype(np.float64))
    return g1 + g2, d


def table(row, nsrc, n, oversample=1, phase=(0, 0)):
    """psi and its bound on the offsets a candidate of lattice phase (py, px) sees:
    [2n - 1][2n - 1], entry [d][e] at u = e - (n - 1) - px / os, v = d - (n - 1) - py / os."""
    k = np.arange(-(n - 1), n, dtype=LD)
    u = k - LD(phase[1]) / LD(oversample)
    v = k - LD(phase[0]) / LD(oversample)
    return psi(row, nsrc, u[None, :], v[:, None])


def chosen(n, nsrc, row, mask, oversample=1, seed=0, nrandom=40):
    """The candidates (lattice indices [C][2], (jy, jx)) the tests look at: the four corners,
    the edge midpoints, the fitted sources' nearest lattice points and their 8 neighbours, a
    point next to a masked pixel if there is one, and ``nrandom`` seeded random ones."""
    g = oversample * (n - 1) + 1
    pts = [(0, 0), (0, g - 1), (g - 1, 0), (g - 1, g - 1), (0, g // 2), (g // 2, 0),
           (g - 1, g // 2), (g // 2, g - 1)]
    for x, y in sources_of(row, nsrc):
        jy, jx = int(round(y * oversample)), int(round(x * oversample))
        pts += [(jy + a, jx + b) for a in (-1, 0, 1) for b in (-1, 0, 1)]
    ym, xm = np.nonzero(mask)
    if ym.size:
        pts.append((int(ym[0]) * oversample, int(xm[0]) * oversample))
        pts.append((int(ym.mean().round()) * oversample, int(xm.mean().round()) * oversample))
    rng = np.random.RandomState(seed)
    pts += [tuple(p) for p in rng.randint(0, g, size=(nrandom, 2))]
    out = sorted({(int(a), int(b)) for a, b in pts if 0 <= a < g and 0 <= b < g})
    return np.array(out, dtype=np.int64)


class Frame:
    """(D, err, mask) of an image as the context stages it, and w."""

    def __init__(self, img):
        self.D, self.err, self.mask = frame(img)
        self.n = self.D.shape[0]
        with np.errstate(all="ignore"):
            ie = np.where(self.mask, 0.0, 1.0 / np.where(self.mask, 1.0, self.err))
        self.w = ie.astype(LD) ** 2                   # the rounded 1 / err, squared exactly
        self.wf = self.w.astype(np.float64)


def sample(fr, row, nsrc, cand, oversample=1, bkgd_mode=0, delta=None):
    """One row at the candidates `cand`: dict of N, Q, A, sigma, snr (long double [C]) and
    the bounds bA, bsigma, bsnr (double [C]) of test_gpu_detect's docstring; delta = 1e-13
    max|M| unless given."""
    n = fr.n
    M = olpe_oracle.build_analytical_model(np.asarray(row, dtype=np.float64), n, nsrc, bkgd_mode)
    if delta is None:
        delta = 1e-13 * float(np.abs(M).max())
    r = fr.D.astype(LD) - M.astype(LD)
    z = fr.w * r
    zf, rf = np.abs(z).astype(np.float64), np.abs(r).astype(np.float64)
    C = len(cand)
    N, Q = np.zeros(C, LD), np.zeros(C, LD)
    dN, dQ = np.zeros(C), np.zeros(C)
    tabs = {}
    for k, (jy, jx) in enumerate(cand):
        cy, py = divmod(int(jy), oversample)
        cx, px = divmod(int(jx), oversample)
        # a candidate j = os c + p sits at c + p / os: the phase shifts the offsets
        if (py, px) not in tabs:
            tabs[(py, px)] = table(row, nsrc, n, oversample, (py, px))
        T, dT = tabs[(py, px)]
        K = T[n - 1 - cy:2 * n - 1 - cy, n - 1 - cx:2 * n - 1 - cx]
        dK = dT[n - 1 - cy:2 * n - 1 - cy, n - 1 - cx:2 * n - 1 - cx]
        Kf = np.abs(K).astype(np.float64)
        N[k] = (z * K).sum()
        Q[k] = (fr.w * K * K).sum()
        # z = w (D - M): the model within delta, the subtraction, w (1 / err 1 ulp, squared)
        # and the product 4 u; then the n^2 fused additions
        dN[k] = (fr.wf * delta * Kf + 4 * U * zf * Kf + zf * dK).sum() \
            + n * n * U * (zf * Kf).sum()
        dQ[k] = (2 * fr.wf * Kf * dK).sum() + (n * n + 4) * U * (fr.wf * Kf * Kf).sum()
    with np.errstate(all="ignore"):
        Qf, Nf = Q.astype(np.float64), np.abs(N).astype(np.float64)
        A, sig, snr = N / Q, 1 / np.sqrt(Q), N / np.sqrt(Q)
        rq = dQ / Qf
        grow = 1.0 / (1.0 - rq)
        bA = (dN / Qf + Nf * dQ / Qf ** 2) * grow + 2 * U * np.abs(A).astype(np.float64)
        bsig = sig.astype(np.float64) * (0.5 * rq * grow + 3 * U)
        bsnr = dN / np.sqrt(Qf) * grow + np.abs(snr).astype(np.float64) * (0.5 * rq * grow + 3 * U)
    blind = Q == 0
    for a in (A, sig, snr):
        a[blind] = LD("nan")
    return {"N": N, "Q": Q, "A": A, "sigma": sig, "snr": snr, "bA": bA, "bsigma": bsig,
            "bsnr": bsnr}


def ensemble(fr, rows, nsrc, cand, oversample=1, bkgd_mode=0):
    """`sample` over rows: arrays [S][C] by name, one delta for the whole set."""
    rows = np.atleast_2d(rows)
    delta = 1e-13 * max(float(np.abs(olpe_oracle.build_analytical_model(
        np.asarray(r, dtype=np.float64), fr.n, nsrc, bkgd_mode)).max()) for r in rows)
    per = [sample(fr, r, nsrc, cand, oversample, bkgd_mode, delta) for r in rows]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


def planes(e, S=None, pivot=0):
    """finalize's seven sample planes from the first S rows of an `ensemble`, and their
    bounds about the pivot row: dicts of [C]."""
    S = e["A"].shape[0] if S is None else S
    A, sg, sn = e["A"][:S], e["sigma"][:S], e["snr"][:S]
    out = {"amp_mean": A.mean(axis=0), "amp_std": A.std(axis=0),
           "sigma_stat": np.sqrt((sg * sg).mean(axis=0)), "snr_mean": sn.mean(axis=0),
           "snr_std": sn.std(axis=0)}
    out["sigma_total"] = np.sqrt((sg * sg).mean(axis=0) + A.var(axis=0))
    out["snr_marg"] = out["amp_mean"] / out["sigma_total"]
    f = {k: np.abs(v).astype(np.float64) for k, v in out.items()}
    eA, eS, eR = e["bA"][:S].max(axis=0), e["bsigma"][:S].max(axis=0), e["bsnr"][:S].max(axis=0)
    spA = 2 * S * U * np.abs(A - A[pivot]).max(axis=0).astype(np.float64)
    spR = 2 * S * U * np.abs(sn - sn[pivot]).max(axis=0).astype(np.float64)
    b = {"amp_mean": eA + spA + 2 * U * f["amp_mean"], "amp_std": 2 * eA + spA,
         "snr_mean": eR + spR + 2 * U * f["snr_mean"], "snr_std": 2 * eR + spR}
    sgf = sg.astype(np.float64)
    # mean sigma^2: each term within 2 sigma dsigma, S additions of positive terms
    d_ms = (2 * sgf * e["bsigma"][:S]).max(axis=0) + (S + 2) * U * f["sigma_stat"] ** 2
    d_var = 2 * f["amp_std"] * b["amp_std"] + b["amp_std"] ** 2
    b["sigma_stat"] = d_ms / (2 * f["sigma_stat"]) * 1.01 + 2 * U * f["sigma_stat"]
    b["sigma_total"] = (d_ms + d_var) / (2 * f["sigma_total"]) * 1.01 + 2 * U * f["sigma_total"]
    rt = b["sigma_total"] / f["sigma_total"]
    b["snr_marg"] = (b["amp_mean"] / f["sigma_total"] + f["snr_marg"] * rt) / (1 - rt) \
        + 2 * U * f["snr_marg"]
    return out, b


def inject(n, amp, pos, seed, nsrc=2):
    """(float32 image, truth): synth.truth_params rendered, plus amp x the truth's unit PSF
    at pos = (x, y), with noise drawn as synth.make_image draws it."""
    from olpefit_amd import synth
    p = synth.truth_params(n, nsrc)
    m = synth.render(p, n, nsrc)
    y, x = np.mgrid[:n, :n]
    if amp:
        m = m + amp * psi(p, nsrc, (x - LD(pos[0])), (y - LD(pos[1])))[0].astype(np.float64)
    rng = np.random.RandomState(seed)
    noise = rng.normal(0.0, 1.0, size=(n, n)) * np.sqrt(38.0 ** 2 + np.abs(m))
    return (m + noise).astype(np.float32), p


def full_map(fr, row, nsrc, oversample=1, bkgd_mode=0):
    """(A, sigma, snr) [g][g] of one row over the whole lattice, as doubles rounded from the
    long-double sums (a row of candidates at a time)."""
    n = fr.n
    g = oversample * (n - 1) + 1
    M = olpe_oracle.build_analytical_model(np.asarray(row, dtype=np.float64), n, nsrc, bkgd_mode)
    z = (fr.w * (fr.D.astype(LD) - M.astype(LD))).ravel()
    w = fr.w.ravel()
    N, Q = np.zeros((g, g), LD), np.zeros((g, g), LD)
    for py in range(oversample):
        for px in range(oversample):
            T, _ = table(row, nsrc, n, oversample, (py, px))
            win = np.lib.stride_tricks.sliding_window_view(T, (n, n))
            for cy in range(n):
                jy = oversample * cy + py
                if jy >= g:
                    continue
                cxs = np.arange(n)
                cxs = cxs[oversample * cxs + px < g]
                K = win[n - 1 - cy, n - 1 - cxs].reshape(cxs.size, -1)
                N[jy, oversample * cxs + px] = K @ z
                Q[jy, oversample * cxs + px] = (K * K) @ w
    with np.errstate(all="ignore"):
        out = np.stack([N / Q, 1 / np.sqrt(Q), N / np.sqrt(Q)])
    out[:, Q == 0] = LD("nan")
    return out.astype(np.float64)
