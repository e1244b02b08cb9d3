"""Parameter covariance, error ellipses, conditional widths and the multivariate Gelman-Rubin
statistic of the chains, from cross-column sums folded on the device (include/olpe.h,
olpe_cov_*).

Everything step 3 reports otherwise is per column.  ``Covariance`` keeps the one object the
two-column questions are functions of: about a fixed pivot p, with d = x - p per row,

    n, skipped, S1[j] = sum d_j, S2[j][k] = sum d_j d_k,

and, with ``walkers`` > 0, per walker its row count ``nw`` and its sums ``S1w``.  A row with
a non-finite value in any column is left out whole and counted in ``skipped``.  The sums are
folded on the GPU from a sampler's device chain or from host rows, in an order fixed by the
fold's shape (the same fold of the same rows repeats bit for bit); the state is additive
(``state`` / ``add``) across launches, objects, ranks and checkpoints whose pivots are
bit-equal, and ``rebase`` moves a state to another pivot on the host.

The pivot.  Given, or taken by the first fold from its first row (walker 0, row 0; a
non-finite entry becomes 0.0); it then stays until ``reset``.  An unlucky pivot costs
precision, not correctness: a variance read as (S2 - S1^2 / n) / (n - 1) cancels (mean - p)^2
against sigma^2, so its relative rounding error grows as 1 + (mean - p)^2 / sigma^2.  Any row
of a converged chain, or the column means, keeps that factor at about two.

Everything after the sums is plain NumPy on a state dict and needs no GPU: ``covariance``,
``correlation``, ``rebase``, ``error_ellipse``, ``conditional_sigma``, ``mpsrf``,
``table_lines``, and ``proposal_widths``, which turns the conditional widths into the
sampler's proposal widths (``Sampler.set_widths``, step 2's ``--widths``).

Not covered: sky-frame ellipses (rotation, distortion and refraction are not applied) and a
separation / position-angle correlation, a collective over the state, per-walker covariance
matrices.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._handle import Handle, _pd, _u64, load_npz  # noqa: F401  (load_npz: Covariance.save's reader)
from ._lib import check

MAX_COLS = 24
U = 2.0 ** -53

#: the position columns {x, y of the primary, x, y of the companion} the ellipses are made of:
#: astrometry.PAIR_COLS's pairs
ELLIPSE_COLS = {2: [((0, 1), (2, 3))], 3: [((0, 1), (2, 3)), ((0, 1), (4, 5))]}
ELLIPSE_NAMES = {2: ["companion - star"], 3: ["b - a", "c - a"]}


# -- host arithmetic on a state ----------------------------------------------------------
def _arrays(state):
    n = int(state["n"])
    p = np.asarray(state["pivot"], dtype=np.float64)
    S1 = np.asarray(state["S1"], dtype=np.float64)
    S2 = np.asarray(state["S2"], dtype=np.float64)
    return n, p, S1, S2


def mean(state):
    """p + S1 / n per column (NaN with no row)."""
    n, p, S1, _ = _arrays(state)
    return p + S1 / n if n else np.full(p.shape, np.nan)


def scatter(state):
    """S2 - S1 S1^T / n: the sum of the cross products about the mean."""
    n, _, S1, S2 = _arrays(state)
    return S2 - np.outer(S1, S1) / n if n else np.full(S2.shape, np.nan)


def covariance(state, ddof: int = 1):
    """(S2 - S1 S1^T / n) / (n - ddof), as ``np.cov`` of the rows folded (NaN where n <=
    ddof)."""
    n = int(state["n"])
    if n - ddof <= 0:
        return np.full(np.asarray(state["S2"]).shape, np.nan)
    return scatter(state) / (n - ddof)


def constant_columns(state):
    """True where a column's scatter about its mean is not above the rounding of its own sum,
    4 n 2^-53 S2[j][j] (the bound any summation order meets): no variance can be read from
    such a column."""
    n, _, _, S2 = _arrays(state)
    if not n:
        return np.ones(S2.shape[0], dtype=bool)
    return ~(np.diag(scatter(state)) > 4.0 * n * U * np.diag(S2))


def correlation(state):
    """``(corr, notes)``: the correlation matrix of the rows folded, and per column "" or
    "constant column" -- such a column has NaN in its row and column (its diagonal
    included)."""
    cov = covariance(state)
    const = constant_columns(state)
    sd = np.sqrt(np.where(const, np.nan, np.diag(cov)))
    with np.errstate(invalid="ignore"):
        corr = cov / np.outer(sd, sd)
    corr[~const, ~const] = 1.0
    return corr, ["constant column" if c else "" for c in const]


def rebase(state, new_pivot):
    """The same state about another pivot: with delta = p - new_pivot, S1' = S1 + n delta,
    S2' = S2 + delta S1^T + S1 delta^T + n delta delta^T, S1w' = S1w + nw delta.  Exact
    algebra, host arithmetic, no device: it lets states folded about different automatic
    pivots be merged by ``add``.  It re-introduces the rounding a good pivot avoided: the
    new sums are rounded at their own size, so moving away from the mean by k sigma costs
    the variance a relative 1 + k^2 in rounding, as folding about that pivot would have."""
    n, p, S1, S2 = _arrays(state)
    q = np.asarray(new_pivot, dtype=np.float64)
    if q.shape != p.shape or not np.isfinite(q).all():
        raise ValueError(f"new pivot of shape {q.shape}: {p.shape[0]} finite values")
    out = dict(state)
    out["pivot"] = q.copy()
    out["has_pivot"] = True
    if not state.get("has_pivot", True):
        return out
    d = p - q
    out["S1"] = S1 + n * d
    cross = np.outer(d, S1)
    s2 = S2 + cross + cross.T + n * np.outer(d, d)
    out["S2"] = np.triu(s2) + np.triu(s2, 1).T          # the triangles bit-equal
    if state.get("walkers"):
        nw = np.asarray(state["nw"], dtype=np.float64)
        out["S1w"] = np.asarray(state["S1w"], dtype=np.float64) + nw[:, None] * d[None, :]
    return out


def between_of(state):
    """What ``Covariance.between`` reduces on the device, from a state on the host:
    ``{"B": sum over the walkers with rows of S1w S1w^T / nw, "m", "nw_min", "nw_max"}``."""
    nw = np.asarray(state["nw"], dtype=np.float64)
    S1w = np.asarray(state["S1w"], dtype=np.float64)
    on = nw > 0
    B = (S1w[on].T / nw[on]) @ S1w[on]
    return {"B": B, "m": int(on.sum()), "nw_min": int(nw[on].min()) if on.any() else 0,
            "nw_max": int(nw[on].max()) if on.any() else 0}


def error_ellipse(cov, cols_a, cols_b, pixscale=None):
    """The error ellipse of the offset (x_b - x_a, y_b - y_a) between two sources, from the
    covariance matrix ``cov`` and their (x, y) columns.  Returns ``cov2`` (the offset's 2 x 2
    covariance, C_bb + C_aa - C_ab - C_ba), ``semi_major`` / ``semi_minor`` in px (the square
    roots of its eigenvalues) and, with ``pixscale`` (mas per px), ``semi_major_mas`` /
    ``semi_minor_mas``, ``angle``: the major axis's direction in degrees from +x towards +y in
    [0, 180), and ``rho``, the correlation of the two offsets.

    This is the detector frame: no rotation to the sky, no distortion correction and no
    differential refraction is applied."""
    c = np.asarray(cov, dtype=np.float64)
    a, b = list(cols_a), list(cols_b)
    c2 = c[np.ix_(b, b)] + c[np.ix_(a, a)] - c[np.ix_(a, b)] - c[np.ix_(b, a)]
    c2 = 0.5 * (c2 + c2.T)
    half_tr, half_diff, off = 0.5 * (c2[0, 0] + c2[1, 1]), 0.5 * (c2[0, 0] - c2[1, 1]), c2[0, 1]
    r = np.hypot(half_diff, off)
    major, minor = np.sqrt(half_tr + r), np.sqrt(max(half_tr - r, 0.0))
    angle = float(np.degrees(0.5 * np.arctan2(2.0 * off, 2.0 * half_diff)) % 180.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = float(off / np.sqrt(c2[0, 0] * c2[1, 1]))
    out = {"cov2": c2, "semi_major": float(major), "semi_minor": float(minor),
           "angle": 0.0 if angle == 180.0 else angle, "rho": rho}
    if pixscale is not None:
        out["semi_major_mas"] = float(major * pixscale)
        out["semi_minor_mas"] = float(minor * pixscale)
        out["pixscale"] = float(pixscale)
    return out


def conditional_sigma(cov, cols=None):
    """The width of each parameter given all the others, 1 / sqrt((C^-1)_jj) over ``cols``
    (default: every column): what a one-parameter-at-a-time proposal sees.  It is computed
    through the correlation matrix R of the non-constant columns of ``cols`` (a column with
    no variance conditions nothing and is left out of the inverse; its entries are NaN):
    sigma_cond_j = sigma_j / sqrt((R^-1)_jj).  Returns ``cols``, ``sigma_marginal``,
    ``sigma_cond``, ``efficiency`` = sigma_cond / sigma_marginal in (0, 1] -- small where the
    other parameters pin this one, i.e. where single-parameter moves cannot go far -- and
    ``condition``, R's 2-norm condition number."""
    c = np.asarray(cov, dtype=np.float64)
    cols = list(range(c.shape[0])) if cols is None else [int(k) for k in cols]
    sub = c[np.ix_(cols, cols)]
    var = np.diag(sub)
    live = np.isfinite(var) & (var > 0.0)
    sd = np.sqrt(np.where(live, var, np.nan))
    eff = np.full(len(cols), np.nan)
    cond = float("nan")
    if live.any():
        R = sub[np.ix_(live, live)] / np.outer(sd[live], sd[live])
        R = 0.5 * (R + R.T)
        np.fill_diagonal(R, 1.0)
        eff[live] = 1.0 / np.sqrt(np.diag(np.linalg.inv(R)))
        cond = float(np.linalg.cond(R))
    return {"cols": cols, "sigma_marginal": sd, "sigma_cond": sd * eff, "efficiency": eff,
            "condition": cond}


def proposal_widths(state, nsrc: int, scale: float = 2.38):
    """Proposal widths [P] for the sampler (``Sampler.set_widths``, ``--widths``) from the
    conditional widths of a state whose first P columns are the proposable parameters (the
    chi^2 column, and any after it, is left out of the inverse).  One parameter moves per
    step, given all the others, so the scale of its move is its conditional width: a proposed
    parameter takes ``scale`` sigma_cond (2.38: the one-dimensional optimum of a Gaussian
    target, Gelman, Roberts & Gilks 1996), a log-proposed one ``scale`` sigma_cond / (|mean|
    ln 10), its width in dex about the mean p + S1 / n.  An entry whose sigma_cond is zero or
    not finite (a constant column, too few rows), or whose value in dex is not finite, keeps
    the default.  Host arithmetic, no GPU."""
    from . import tune
    w = tune.default_widths(nsrc)
    P = w.size
    if np.asarray(state["S2"]).shape[0] < P:
        raise ValueError(f"a state of {np.asarray(state['S2']).shape[0]} columns for {P} parameters")
    cov = np.array(covariance(state))
    const = constant_columns(state)
    cov[const, const] = np.nan                  # no variance to read: out of the inverse
    sc = conditional_sigma(cov, range(P))["sigma_cond"]
    mu = mean(state)[:P]
    logp = set(tune.log_params(nsrc))
    for j in range(P):
        if not (np.isfinite(sc[j]) and sc[j] > 0.0):
            continue
        v = scale * sc[j]
        if j in logp:
            with np.errstate(divide="ignore", invalid="ignore"):
                v = v / (abs(mu[j]) * np.log(10.0))
        if np.isfinite(v) and v > 0.0:
            w[j] = v
    return w


def mpsrf(state, between=None, cols=None):
    """Brooks & Gelman's (1998) multivariate potential scale reduction factor for m walkers
    of n rows each, over ``cols`` (default: every column; constant columns are left out).

    With W the mean within-walker covariance (divisor n - 1) and B / n the covariance of the
    walker means (divisor m - 1),

        Rp = (n - 1) / n + (m + 1) / m  lambda_max(W^-1 B / n).

    From the sums: the scatter about the pooled mean is S2 - S1 S1^T / (m n), the between
    term about it is ``between`` - S1 S1^T / (m n) (``between`` = sum_w S1w S1w^T / nw: what
    ``Covariance.between`` reduces on the device, or ``between_of(state)``), and the within
    scatter is their difference, S2 - ``between``.

    Returns a dict: ``mpsrf`` (Rp), ``rhat`` (per column of ``cols`` the univariate value under
    the same convention, (n - 1) / n + (m + 1) / m (B / n)_jj / W_jj; NaN for a constant
    column), ``cols``, ``m``, ``n``, ``note``.  It is defined only when every walker has the
    same count: otherwise, with fewer than two walkers or rows, or with no column left,
    ``mpsrf`` is None and ``note`` says why (giving the min and max of nw)."""
    nC = np.asarray(state["S2"]).shape[0]
    cols = list(range(nC)) if cols is None else [int(k) for k in cols]
    if not state.get("walkers"):
        return {"mpsrf": None, "rhat": np.full(len(cols), np.nan), "cols": cols, "m": 0, "n": 0,
                "note": "no per-walker sums (walkers = 0)"}
    bt = between_of(state) if between is None else between
    m, lo, hi = int(bt["m"]), int(bt["nw_min"]), int(bt["nw_max"])
    out = {"mpsrf": None, "rhat": np.full(len(cols), np.nan), "cols": cols, "m": m, "n": lo,
           "note": ""}
    if lo != hi or m != int(state["walkers"]):
        out["note"] = (f"walkers hold different row counts (nw from "
                       f"{int(np.asarray(state['nw']).min())} to {hi}): not defined")
        return out
    n = lo
    if m < 2 or n < 2:
        out["note"] = f"{m} walkers of {n} rows: not defined"
        return out
    _, _, S1, S2 = _arrays(state)
    B = np.asarray(bt["B"], dtype=np.float64)
    ix = np.ix_(cols, cols)
    Wm = (S2 - B)[ix] / (m * (n - 1.0))
    Bn = (B - np.outer(S1, S1) / (m * n))[ix] / (n * (m - 1.0))
    const = constant_columns(state)[cols] | ~(np.diag(Wm) > 0.0)
    live = ~const
    with np.errstate(invalid="ignore", divide="ignore"):
        out["rhat"] = np.where(live, (n - 1.0) / n + (m + 1.0) / m * np.diag(Bn) / np.diag(Wm),
                               np.nan)
    if not live.any():
        out["note"] = "no column with scatter"
        return out
    # lambda_max of W^-1 B/n as the symmetric problem L^-1 (B/n) L^-T, W = L L^T, after
    # scaling both by W's diagonal
    s = np.sqrt(np.diag(Wm)[live])
    Ws = Wm[np.ix_(live, live)] / np.outer(s, s)
    Bs = Bn[np.ix_(live, live)] / np.outer(s, s)
    try:
        L = np.linalg.cholesky(0.5 * (Ws + Ws.T))
    except np.linalg.LinAlgError:
        out["note"] = "within-walker covariance not positive definite"
        return out
    M = np.linalg.solve(L, np.linalg.solve(L, 0.5 * (Bs + Bs.T)).T)
    lam = float(np.linalg.eigvalsh(0.5 * (M + M.T))[-1])
    out["mpsrf"] = (n - 1.0) / n + (m + 1.0) / m * max(lam, 0.0)
    return out


def summarize(state, labels=None, between=None, k: int = 10, nsrc=None, pixscale=None,
              param_cols=None):
    """Everything above for one state, as ``Covariance.result`` returns it: ``labels``, ``n``,
    ``skipped``, ``mean``, ``cov``, ``corr``, ``notes`` (per column), ``pairs`` (the k largest
    |r|: (label_j, label_k, r)), ``ellipses`` (with ``nsrc`` 2 or 3: companion against star,
    or b and c against a, each ``error_ellipse`` plus its ``name``), ``conditional``
    (``conditional_sigma`` over ``param_cols``), ``mpsrf`` (the ``mpsrf`` dict over
    ``param_cols``)."""
    nC = np.asarray(state["S2"]).shape[0]
    labels = [f"c{i}" for i in range(nC)] if labels is None else [str(s) for s in labels]
    cols = list(range(nC)) if param_cols is None else [int(c) for c in param_cols]
    cov = covariance(state)
    corr, notes = correlation(state)
    iu, ju = np.triu_indices(nC, 1)
    r = corr[iu, ju]
    order = [i for i in np.argsort(-np.abs(np.nan_to_num(r)), kind="stable") if np.isfinite(r[i])]
    pairs = [(labels[iu[i]], labels[ju[i]], float(r[i])) for i in order[:k]]
    ellipses = []
    if nsrc in ELLIPSE_COLS and int(state["n"]) > 1:
        for name, (ca, cb) in zip(ELLIPSE_NAMES[nsrc], ELLIPSE_COLS[nsrc]):
            e = error_ellipse(cov, ca, cb, pixscale)
            e["name"] = name
            ellipses.append(e)
    return {"labels": labels, "n": int(state["n"]), "skipped": int(state["skipped"]),
            "mean": mean(state), "cov": cov, "corr": corr, "notes": notes, "pairs": pairs,
            "ellipses": ellipses, "conditional": conditional_sigma(cov, cols),
            "mpsrf": mpsrf(state, between, cols)}


def table_lines(res):
    """The k largest |r| pairs by label, the ellipses, the conditional widths with their
    efficiency, and the multivariate R-hat."""
    out = [f"{a:>10} {b:<10} r {r:+.6f}" for a, b, r in res["pairs"]]
    for e in res["ellipses"]:
        mas = (f" ({e['semi_major_mas']:.6g} x {e['semi_minor_mas']:.6g} mas)"
               if "semi_major_mas" in e else "")
        out.append(f"ellipse {e['name']}: {e['semi_major']:.6g} x {e['semi_minor']:.6g} px{mas} "
                   f"angle {e['angle']:.4f} deg rho {e['rho']:+.6f} (detector frame)")
    cs = res["conditional"]
    for i, c in enumerate(cs["cols"]):
        note = f" ({res['notes'][c]})" if res["notes"][c] else ""
        out.append(f"{res['labels'][c]:>10} sigma {cs['sigma_marginal'][i]:.6g} conditional "
                   f"{cs['sigma_cond'][i]:.6g} efficiency {cs['efficiency'][i]:.6g}{note}")
    out.append(f"Condition number of the correlation matrix: {cs['condition']:.6g}")
    mp = res["mpsrf"]
    if mp["mpsrf"] is None:
        out.append(f"Multivariate R-hat: not available ({mp['note']})")
    else:
        out.append(f"Multivariate R-hat ({mp['m']} walkers x {mp['n']} rows): {mp['mpsrf']:.9f} "
                   f"(largest univariate {np.nanmax(mp['rhat']):.9f})")
    return out


class Covariance(Handle):
    """One ``olpe_cov``: the cross-column sums of [..., ncols] chains on one GPU.
    1 <= ncols <= 24; ``walkers`` 0 keeps the pooled sums only, the ensemble's walker count
    also each walker's count and sums (what ``mpsrf`` needs); ``pivot`` [ncols] finite, or
    None: the first fold takes its first row (see the module's note on what a pivot costs)."""

    _destroy = "olpe_cov_destroy"

    def __init__(self, ncols: int, walkers: int = 0, pivot=None, labels=None, device: int = 0):
        self.ncols, self.walkers = int(ncols), int(walkers)
        self.labels = ([f"c{i}" for i in range(self.ncols)] if labels is None
                       else [str(s) for s in labels])
        if len(self.labels) != self.ncols:
            raise ValueError(f"{len(self.labels)} labels for {self.ncols} columns")
        p = None
        if pivot is not None:
            p = np.ascontiguousarray(pivot, dtype=np.float64)
            if p.shape != (self.ncols,):
                raise ValueError(f"pivot of shape {p.shape} for {self.ncols} columns")
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.olpe_cov_create(int(device), self.ncols, self.walkers,
                                        None if p is None else _pd(p), C.byref(h)))
        self._h = h

    # -- folding ------------------------------------------------------------------
    def fold(self, sampler, row_step: int = 1):
        """Fold rows 0, row_step, ... of every walker of the sampler's last launch from its
        device chain, in place (once per launch; async on the sampler's stream, no host
        copy)."""
        check(self._lib.olpe_cov_fold_ctx(self._h, sampler._ctx, int(row_step)))

    def fold_rows(self, rows, time_major: bool = False):
        """Fold host rows: [walkers][rows][ncols], or with ``time_major`` [rows][walkers]
        [ncols] as step 3's chains lie; no transposition on the host.  With ``walkers`` 0 the
        first two dimensions are just rows (a 2-D [rows][ncols] array is taken as such)."""
        r = np.ascontiguousarray(rows, dtype=np.float64)
        if r.ndim == 2 and not self.walkers:
            r = r[None]
        if r.ndim != 3 or r.shape[2] != self.ncols:
            raise ValueError(f"rows of shape {r.shape}, expected [walkers][rows][{self.ncols}] "
                             f"(or [rows][walkers][{self.ncols}] with time_major)")
        nw, nr = (r.shape[1], r.shape[0]) if time_major else (r.shape[0], r.shape[1])
        check(self._lib.olpe_cov_fold_rows(self._h, _pd(r), nw, nr, int(bool(time_major))))

    def state(self):
        """``{"ncols", "walkers", "n", "skipped", "has_pivot", "pivot" [ncols], "S1" [ncols],
        "S2" [ncols][ncols]}`` and, with walkers, ``"nw"`` [walkers] (uint64) and ``"S1w"``
        [walkers][ncols]."""
        n, sk, hp = C.c_ulonglong(0), C.c_ulonglong(0), C.c_int(0)
        p, S1 = np.zeros(self.ncols), np.zeros(self.ncols)
        S2 = np.zeros((self.ncols, self.ncols))
        check(self._lib.olpe_cov_get(self._h, C.byref(n), C.byref(sk), C.byref(hp), _pd(p),
                                     _pd(S1), _pd(S2)))
        st = {"ncols": self.ncols, "walkers": self.walkers, "n": int(n.value),
              "skipped": int(sk.value), "has_pivot": bool(hp.value), "pivot": p, "S1": S1,
              "S2": S2}
        if self.walkers:
            nw = np.zeros(self.walkers, dtype=np.uint64)
            S1w = np.zeros((self.walkers, self.ncols))
            check(self._lib.olpe_cov_walkers_get(self._h, _u64(nw), _pd(S1w)))
            st["nw"], st["S1w"] = nw, S1w
        return st

    def between(self):
        """The between-walker term reduced on the device in a fixed order: ``{"B" [ncols]
        [ncols] = sum over the walkers with rows of S1w S1w^T / nw, "m" such walkers,
        "nw_min", "nw_max"}``."""
        B = np.zeros((self.ncols, self.ncols))
        m, lo, hi = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
        check(self._lib.olpe_cov_between(self._h, _pd(B), C.byref(m), C.byref(lo), C.byref(hi)))
        return {"B": B, "m": int(m.value), "nw_min": int(lo.value), "nw_max": int(hi.value)}

    def add(self, state):
        """Merge another object's, rank's or checkpoint's ``state()``: the same ncols and
        walkers and a bit-equal pivot (``rebase`` one state otherwise); anything else is
        refused with the state untouched.  An object without a pivot yet adopts the incoming
        one; a state that never had one holds nothing and adds nothing."""
        if not state.get("has_pivot", True) and not int(state["n"]) and not int(state["skipped"]):
            return
        p = np.ascontiguousarray(state["pivot"], dtype=np.float64)
        S1 = np.ascontiguousarray(state["S1"], dtype=np.float64)
        S2 = np.ascontiguousarray(state["S2"], dtype=np.float64)
        if S2.ndim != 2 or S2.shape[0] != S2.shape[1] or not (S1.shape == p.shape == S2.shape[:1]):
            raise ValueError(f"S2 of shape {S2.shape}, S1 {S1.shape}, pivot {p.shape}")
        walkers = int(state.get("walkers", 0))
        nw = S1w = None
        if walkers:
            nw = np.ascontiguousarray(state["nw"], dtype=np.uint64)
            S1w = np.ascontiguousarray(state["S1w"], dtype=np.float64)
            if nw.shape != (walkers,) or S1w.shape != (walkers, S2.shape[0]):
                raise ValueError(f"nw of shape {nw.shape}, S1w {S1w.shape} for {walkers} walkers")
        check(self._lib.olpe_cov_add(self._h, int(S2.shape[0]), walkers, int(state["n"]),
                                     int(state["skipped"]), _pd(p), _pd(S1), _pd(S2),
                                     None if nw is None else _u64(nw),
                                     None if S1w is None else _pd(S1w)))

    def reset(self):
        """Zero the state; a pivot given at creation stays, an automatic one is forgotten; the
        launch folded last may be folded again."""
        check(self._lib.olpe_cov_reset(self._h))

    # -- results ------------------------------------------------------------------
    def result(self, k: int = 10, nsrc=None, pixscale=None, param_cols=None, state=None):
        """``summarize`` of the state with this object's labels; the between-walker term comes
        from the device."""
        st = self.state() if state is None else state
        bt = self.between() if self.walkers and state is None else None
        return summarize(st, self.labels, bt, k, nsrc, pixscale, param_cols)

    def save(self, path, **kw):
        """One ``.npz`` with the state and the results; returns ``(state, result)``."""
        st = self.state()
        res = summarize(st, self.labels, self.between() if self.walkers else None, **kw)
        save_npz(path, st, res)
        return st, res


def save_npz(path, state, res):
    cs, mp, el = res["conditional"], res["mpsrf"], res["ellipses"]
    extra = {}
    if state.get("walkers"):
        extra = {"nw": state["nw"], "S1w": state["S1w"]}
    with open(path, "wb") as f:
        np.savez(f, labels=np.asarray(res["labels"], dtype="U"), ncols=np.int64(state["ncols"]),
                 walkers=np.int64(state["walkers"]), n=np.uint64(state["n"]),
                 skipped=np.uint64(state["skipped"]), has_pivot=np.bool_(state["has_pivot"]),
                 pivot=state["pivot"], S1=state["S1"], S2=state["S2"], mean=res["mean"],
                 cov=res["cov"], corr=res["corr"], notes=np.asarray(res["notes"], dtype="U"),
                 ellipse_names=np.asarray([e["name"] for e in el], dtype="U"),
                 ellipse_cov2=np.array([e["cov2"] for e in el]).reshape(len(el), 2, 2),
                 ellipse_axes=np.array([[e["semi_major"], e["semi_minor"]] for e in el]
                                       ).reshape(len(el), 2),
                 ellipse_angle=np.array([e["angle"] for e in el]),
                 ellipse_rho=np.array([e["rho"] for e in el]),
                 pixscale=np.float64(el[0].get("pixscale", np.nan) if el else np.nan),
                 param_cols=np.asarray(cs["cols"], dtype=np.int64),
                 sigma_marginal=cs["sigma_marginal"], sigma_cond=cs["sigma_cond"],
                 efficiency=cs["efficiency"], condition=np.float64(cs["condition"]),
                 mpsrf=np.float64(np.nan if mp["mpsrf"] is None else mp["mpsrf"]),
                 rhat=mp["rhat"], mpsrf_note=np.asarray(mp["note"], dtype="U"), **extra)
