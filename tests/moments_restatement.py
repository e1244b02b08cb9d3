"""The whole-run moments fold (olpe_moments_accumulate, olpe_moments.hip) restated in NumPy:
the reference, the error bounds and an emulation of the kernels' float64 operation order
with one switch per wrong variant.  Shared by test_moments_cpu.py, test_gpu_moments.py and
the two moments tests of test_gpu_parity.py.

Rows are [W][n][PS]: walker, recorded row, column.  Per walker and column the fold keeps
mean = sum x / n and M2 = sum (x - mean)^2 over every row folded so far.

Bounds (worst case, derived; u = 2^-53, A = max |x|, R = max |x - mean| over the walker's n
rows of the column):

    |mean - ref| <= 4 n u A
    |M2   - ref| <= 4 n u (M2 + A R)

* Mean: block means (c + s / nb) and merged means (m + delta nb / n) are convex
  combinations of values of magnitude <= A; each of their operations rounds by at most
  u A, and a row's value passes through at most four of them per level (difference, block
  sum, block mean, merge), the errors entering the result with weights that sum to <= n.
* M2, first term: the rounding of the n squared deviations and of their sum -- each
  relative u on a partial sum <= M2, with (d (1 + 2u))^2 for the deviation's own rounding.
* M2, second term: a merge adds delta^2 n_a n_b / n; an error eps <= u A in a block mean
  changes it by 2 |delta| eps n_a n_b / n <= 2 R u A min(n_a, n_b), and the smaller sides
  of the merges (the new block, left to right; then the row groups) sum to <= 2 n.

A column that a walker never changes gives M2 == 0.0 and mean == the value exactly: every
difference in the fold is then exactly 0.

Non-finite rows are out of scope: the sampler records none.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53

K_FOLD_ROWS = 8          # fold_cols_kernel: rows per block
K_WAVE_ROWS = 16         # fold_rows_kernel: rows per block of a lane
K_FOLD_ROWS_MIN = 64     # launches of at least this many rows take fold_rows_kernel

#: the wrong variants the tests must tell from the fold (see ``emulate``)
MUTANTS = ("about_zero", "drop_last_group", "no_guard", "no_delta")


def reference(rows):
    """rows [W][n][PS] -> (mean, M2) [W][PS] in longdouble, two-pass (zeros for n = 0)."""
    x = np.asarray(rows, dtype=np.float64).astype(LD)
    W, n, ps = x.shape
    if n == 0:
        return np.zeros((W, ps), dtype=LD), np.zeros((W, ps), dtype=LD)
    mean = x.sum(axis=1, dtype=LD) / LD(n)
    d = x - mean[:, None, :]
    m2 = (d * d).sum(axis=1, dtype=LD)
    return mean, m2 - d.sum(axis=1, dtype=LD) ** 2 / LD(n)     # (the corrected two-pass)


def bounds(rows):
    """rows [W][n][PS] -> (bound on |mean - ref|, bound on |M2 - ref|) [W][PS], longdouble."""
    x = np.asarray(rows, dtype=np.float64).astype(LD)
    W, n, ps = x.shape
    if n == 0:
        return np.zeros((W, ps), dtype=LD), np.zeros((W, ps), dtype=LD)
    mean, m2 = reference(rows)
    A = np.abs(x).max(axis=1)
    R = np.abs(x - mean[:, None, :]).max(axis=1)
    f = LD(4) * LD(n) * LD(U)
    return f * A, f * (m2 + A * R)


def constant_columns(rows):
    """[W][PS] bool: the walker's column holds one value in every row (n >= 1)."""
    x = np.asarray(rows, dtype=np.float64)
    return (x == x[:, :1, :]).all(axis=1)


# ---------------------------------------------------------------------------------------
# the kernels' arithmetic, float64 operation by operation (vectorised over [W][PS]; the row
# counts are the same for every walker and column, so they are Python floats)

def _fma(a, b, c):
    """fma(a, b, c) to within a double rounding: the product and the sum in longdouble (64-bit
    significand), rounded to float64 once more."""
    return (a.astype(LD) * b.astype(LD) + c.astype(LD)).astype(np.float64)


def _merge(a, b, mutant):
    """chan_merge: the pair b = (mean, M2, n) into a."""
    (m, q, n), (mb, qb, nb) = a, b
    if nb == 0.0:
        return a
    if n == 0.0:
        return b
    nn = n + nb
    delta = mb - m
    m1 = m + delta * (nb / nn)
    q1 = q + qb
    if mutant != "no_delta":
        q1 = q1 + (delta * delta) * (n * nb / nn)
    return m1, q1, nn


def _block(v, nb, mutant):
    """(mean, M2, n) of one register block v [W][PS][width], its first nb slots rows and the
    rest the zero padding: the mean about the first row, then the squared deviations."""
    width = v.shape[-1]
    guard = mutant != "no_guard"
    if mutant == "about_zero":          # sum x and sum x^2: the square sum cancels
        s = np.zeros_like(v[..., 0])
        ss = np.zeros_like(s)
        for i in range(nb):
            s = s + v[..., i]
            ss = _fma(v[..., i], v[..., i], ss)
        fb = float(nb)
        return s / fb, ss - s * s / fb, fb
    c = v[..., 0]
    s = np.zeros_like(c)
    for i in range(width):
        if i < nb or not guard:
            s = s + (v[..., i] - c)
    fb = float(nb)
    mb = c + s / fb
    qb = np.zeros_like(c)
    for i in range(width):
        if i < nb or not guard:
            d = v[..., i] - mb
            qb = _fma(d, d, qb)
    return mb, qb, fb


def _lane(x, width, mutant):
    """One lane's rows x [W][n][PS] in blocks of ``width``, merged left to right."""
    W, n, ps = x.shape
    acc = (np.zeros((W, ps)), np.zeros((W, ps)), 0.0)
    for r0 in range(0, n, width):
        nb = min(width, n - r0)
        v = np.zeros((W, ps, width))
        v[..., :nb] = np.moveaxis(x[:, r0:r0 + nb, :], 1, 2)
        acc = _merge(acc, _block(v, nb, mutant), mutant)
    return acc


def fold_cols(x, mutant=None):
    """fold_cols_kernel: one thread per (walker, column), blocks of 8 rows."""
    return _lane(x, K_FOLD_ROWS, mutant)


def fold_rows(x, ps, mutant=None):
    """fold_rows_kernel: G = 64 // ps row groups, group g taking rows g, g + G, ... in blocks
    of 16, the groups merged into group 0 in group order."""
    G = 64 // ps
    lanes = [_lane(x[:, g::G, :], K_WAVE_ROWS, mutant) for g in range(G)]
    acc = lanes[0]
    for h in range(1, G - 1 if mutant == "drop_last_group" else G):
        acc = _merge(acc, lanes[h], mutant)
    return acc


def emulate(rows, launches, ps=None, mutant=None):
    """The running (n, mean [W][PS], M2 [W][PS]) after folding rows [W][sum(launches)][PS]
    launch by launch as olpe_moments_accumulate does: launches of >= 64 rows through
    fold_rows, shorter ones through fold_cols, an empty one skipped, each launch's pair merged
    into the running pair.  ``mutant``: None or one of MUTANTS --
      "about_zero"       a block's sums about 0 instead of about its first value: mean =
                         sum x / nb, M2 = sum x^2 - (sum x)^2 / nb;
      "drop_last_group"  the last row group left out of the cross-lane merge;
      "no_guard"         the i < nb guards dropped: the zero padding enters;
      "no_delta"         the delta^2 n_a n_b / n term of the merge dropped."""
    x = np.ascontiguousarray(rows, dtype=np.float64)
    W, n, cols = x.shape
    ps = cols if ps is None else ps
    assert cols == ps and sum(launches) == n and (mutant is None or mutant in MUTANTS)
    run = (np.zeros((W, ps)), np.zeros((W, ps)), 0.0)
    r = 0
    for nrec in launches:
        part = x[:, r:r + nrec, :]
        r += nrec
        if nrec == 0:
            continue
        if nrec >= K_FOLD_ROWS_MIN and ps <= 64:
            m, q, _ = fold_rows(part, ps, mutant)
        else:
            m, q, _ = fold_cols(part, mutant)
        # the host counts the launch's rows, whatever the lanes counted
        run = _merge(run, (m, q, float(nrec)), mutant)
    return int(run[2]), run[0], run[1]


# ---------------------------------------------------------------------------------------
# inputs

#: the named series of the tests: name -> f(w, r [n] float64, rng) -> [n] float64
def _gauss_at(ratio):
    return lambda w, r, rng: ratio + rng.normal(size=r.size)


NAMED = {
    "gauss_0": _gauss_at(0.0),
    "gauss_1e2": _gauss_at(1e2),
    "gauss_3e4": _gauss_at(3e4),
    "gauss_1e6": _gauss_at(1e6),
    "gauss_1e9": _gauss_at(1e9),
    "ramp": lambda w, r, rng: 1e6 + 1e-3 * (r + w),
    "step": lambda w, r, rng: 1.0 * (r >= r.size // 2 + w % 7),
    "const_0.1": lambda w, r, rng: np.full(r.size, 0.1 * (w + 1)),
    "spike": lambda w, r, rng: 30.0 + 1.0 * (r == (3 * w + 1) % max(r.size, 1)),
    "alt_1e8": lambda w, r, rng: 1e8 + (-1.0) ** (r + w),
}


def named_rows(W, n, ps, seed=0):
    """([W][n][PS] rows, [PS] names): the named series cycled over the columns, every walker
    its own draw / phase; column PS - 1 is the constant 0.1 (w + 1)."""
    rng = np.random.RandomState(seed)
    names = [list(NAMED)[k % len(NAMED)] for k in range(ps - 1)] + ["const_0.1"]
    r = np.arange(n, dtype=np.float64)
    x = np.empty((W, n, ps))
    for w in range(W):
        for k, name in enumerate(names):
            x[w, :, k] = NAMED[name](w, r, rng)
    return x, names


KINDS = ("gauss", "ramp", "step", "const", "spike", "alt")
OFFSETS = (1e9, 0.0, 1e6, -30.0, 30.0)
SCALES = (1e-3, 1.0, 1e-2, 0.1)


def column_plan(ps):
    """[(kind, offset, scale)] of columns 0 .. PS - 1: the kinds cycle, the offsets and scales
    shift against them (17 columns: Gaussians at 1e9, 30, -30; alternating at 1e9, 30; ramps
    at 0, 1e9, 30; 20 columns add a spike at 1e6, alternating at -30, a Gaussian at 1e6);
    column PS - 1 is constant."""
    plan = [(KINDS[k % 6], OFFSETS[(k + 3 * (k // 6)) % 5], SCALES[k % 4]) for k in range(ps - 1)]
    return plan + [("const", 0.0, 1.0)]


def _series(kind, w, r, rng):
    n = r.size
    if kind == "gauss":
        return rng.normal(size=n)
    if kind == "ramp":
        return r + w
    if kind == "step":
        return 1.0 * (r >= n // 2 + w % 7)
    if kind == "const":
        return np.full(n, 0.1 * (w + 1))
    if kind == "spike":
        return 1.0 * (r == (3 * w + 1) % max(n, 1))
    return (-1.0) ** (r + w)                                     # alt


def chain_rows(W, n, ps, seed=0):
    """[W][n][PS] rows of the GPU tests: column k of walker w holds offset[k] + scale[k] *
    series_k(w, r) by ``column_plan``: no two columns and no two walkers alike, so a lane /
    column or walker mix-up is a gross error."""
    rng = np.random.RandomState(seed)
    plan = column_plan(ps)
    r = np.arange(n, dtype=np.float64)
    x = np.empty((W, n, ps))
    for w in range(W):
        for k, (kind, off, scale) in enumerate(plan):
            x[w, :, k] = off + scale * _series(kind, w, r, rng)
    return x


def check(n, mean, m2, rows, what=""):
    """Assert a fold's (n, mean, M2) against ``reference`` within ``bounds`` over rows, and
    the constant columns exactly.  Returns the largest (mean, M2) error / bound."""
    rows = np.asarray(rows, dtype=np.float64)
    assert n == rows.shape[1], (what, n, rows.shape[1])
    if n == 0:
        assert not np.any(mean) and not np.any(m2), what
        return 0.0, 0.0
    rm, rq = reference(rows)
    bm, bq = bounds(rows)
    em, eq = np.abs(mean.astype(LD) - rm), np.abs(m2.astype(LD) - rq)
    const = constant_columns(rows)
    with np.errstate(invalid="ignore", divide="ignore"):
        fm = np.where(bm > 0, em / bm, np.where(em > 0, np.inf, 0.0)).astype(np.float64)
        fq = np.where(bq > 0, eq / bq, np.where(eq > 0, np.inf, 0.0)).astype(np.float64)
    # (each message carries the largest err / bound of the columns that vary)
    worst = (float(np.max(fm, where=~const, initial=0.0)),
             float(np.max(fq, where=~const, initial=0.0)))
    assert np.all(m2[const] == 0.0), (what, "M2 of a constant column", worst,
                                      np.argwhere(const & (m2 != 0.0))[:4])
    assert np.array_equal(mean[const], rows[:, 0, :][const]), (what, "mean of a constant column",
                                                               worst)
    assert np.all(fm <= 1.0), (what, "mean err / bound", worst, np.argwhere(fm > 1.0)[:4])
    assert np.all(fq <= 1.0), (what, "M2 err / bound", worst, np.argwhere(fq > 1.0)[:4])
    return float(fm.max()), float(fq.max())
