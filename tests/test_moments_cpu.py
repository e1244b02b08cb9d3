"""The moments fold's restatement (tests/moments_restatement.py) checked on a machine
without a GPU: the emulation of the kernels' float64 arithmetic stays within the derived
bounds on the inputs test_gpu_moments.py uploads, and each of the four wrong variants of
the fold breaks the M2 bound or the exactness of a constant column on a named input.  This
keeps the bounds honest (neither so tight that correct rounding breaks them, nor so loose
that a wrong fold passes) and documents what the GPU test is able to catch."""
import numpy as np
import pytest

import moments_restatement as mr

LD = mr.LD
LAUNCHES = (97, 5, 64, 150, 63, 1, 0, 2)
SINGLE = (1, 7, 8, 9, 47, 48, 49, 63, 64, 65, 95, 96, 97, 98, 99, 144, 145)


def fractions(n, mean, m2, rows):
    """(mean err / bound, M2 err / bound, exactness broken) per [W][PS]."""
    rm, rq = mr.reference(rows)
    bm, bq = mr.bounds(rows)
    em, eq = np.abs(mean.astype(LD) - rm), np.abs(m2.astype(LD) - rq)
    with np.errstate(invalid="ignore", divide="ignore"):
        fm = np.where(bm > 0, em / bm, np.where(em > 0, np.inf, 0.0)).astype(np.float64)
        fq = np.where(bq > 0, eq / bq, np.where(eq > 0, np.inf, 0.0)).astype(np.float64)
    const = mr.constant_columns(rows)
    inexact = const & ((m2 != 0.0) | (mean != rows[:, 0, :]))
    return fm, fq, inexact


def test_reference_is_the_two_pass_moments():
    x, names = mr.named_rows(2, 50, 17, 3)
    mean, m2 = mr.reference(x)
    np.testing.assert_allclose(mean.astype(float), x.mean(axis=1), rtol=1e-14)
    k = names.index("gauss_0")                   # (well conditioned: float64 NumPy agrees)
    np.testing.assert_allclose(m2[:, k].astype(float), x[:, :, k].var(axis=1) * 50, rtol=1e-12)
    for f in (mr.reference, mr.bounds):          # no rows: zeros, not NaN
        a, b = f(np.empty((2, 0, 17)))
        assert not a.any() and not b.any()


@pytest.mark.parametrize("ps", [17, 20])
@pytest.mark.parametrize("rows_of", ["named", "chain"])
def test_emulation_within_bounds(ps, rows_of):
    """The kernels' arithmetic stays within both bounds, constant columns exactly, over
    the several-launch sequence (both kernels, ragged blocks and row groups, an empty
    launch) and every single-launch length of the GPU test."""
    make = (lambda W, n, s: mr.named_rows(W, n, ps, s)[0]) if rows_of == "named" else \
        (lambda W, n, s: mr.chain_rows(W, n, ps, s))
    worst = [0.0, 0.0]
    x = make(3, sum(LAUNCHES), 1)
    for launches in (LAUNCHES, (sum(LAUNCHES),), (3, 200, sum(LAUNCHES) - 203)):
        fm, fq = mr.check(*mr.emulate(x, launches, ps), x, what=launches)
        worst = [max(worst[0], fm), max(worst[1], fq)]
    for n in SINGLE:
        y = make(2, n, n)
        fm, fq = mr.check(*mr.emulate(y, (n,), ps), y, what=n)
        worst = [max(worst[0], fm), max(worst[1], fq)]
    print(f"ps {ps} {rows_of}: largest mean err/bound {worst[0]:.3g}, M2 err/bound {worst[1]:.3g}")


#: the named inputs on which each wrong variant must break the M2 bound or exactness
CATCHES = {
    # sum x^2 - (sum x)^2 / nb cancels where mean / R is large; a constant 0.1 sums inexactly
    "about_zero": ("gauss_3e4", "gauss_1e6", "gauss_1e9", "alt_1e8", "ramp", "const_0.1"),
    # a third of a long launch's rows missing: every column that varies
    "drop_last_group": ("gauss_0", "gauss_1e9", "ramp", "step", "spike", "alt_1e8"),
    # zeros among the rows: every column that is not 0 throughout, constants included
    "no_guard": ("gauss_1e2", "gauss_1e9", "ramp", "step", "const_0.1", "alt_1e8"),
    # the between-block part of M2 missing: every column whose block means differ
    "no_delta": ("gauss_0", "gauss_1e9", "ramp", "step", "spike"),
}


@pytest.mark.parametrize("ps", [17, 20])
@pytest.mark.parametrize("mutant", mr.MUTANTS)
def test_mutants_break_the_bounds(mutant, ps):
    x, names = mr.named_rows(3, sum(LAUNCHES), ps, 1)
    fm, fq, inexact = fractions(*mr.emulate(x, LAUNCHES, ps, mutant), x)
    caught = (fq > 1.0) | inexact
    by_name = {nm: float(fq[:, [k for k, m in enumerate(names) if m == nm]].max())
               for nm in dict.fromkeys(names)}
    print(mutant, ps, {k: f"{v:.3g}" for k, v in by_name.items()},
          "inexact:", sorted({names[k] for k in np.nonzero(inexact.any(axis=0))[0]}))
    for nm in CATCHES[mutant]:
        cols = [k for k, m in enumerate(names) if m == nm]
        assert caught[:, cols].any(), (mutant, nm, by_name[nm])


def test_step_input_does_not_catch_about_zero():
    """Why the named inputs need the Gaussian and alternating columns: a step from 0 to 1
    has constant blocks but for one, and sums of 0s and 1s about 0 are exact."""
    x, names = mr.named_rows(3, sum(LAUNCHES), 17, 1)
    _, fq, inexact = fractions(*mr.emulate(x, LAUNCHES, 17, "about_zero"), x)
    k = names.index("step")
    assert fq[:, k].max() <= 1.0 and not inexact[:, k].any()
    assert fq[:, names.index("gauss_1e6")].min() > 1.0 and fq[:, names.index("alt_1e8")].min() > 1.0
