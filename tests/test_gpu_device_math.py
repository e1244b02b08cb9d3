"""The device math primitives against exact values (tests/golden/device_math.npz).

The probe library (tests/c/device_probe.hip) runs the product's own device functions --
ExpTab, exp_neg, sincos_small, make_trig, make_coef, accept_threshold -- elementwise on
the fixture's inputs; errors are measured in ulp of the exact value, (got - hi - lo) /
ulp(hi), never against the code under test.  Bounds are the headers' own claims or are
derived in the test's docstring; measured maxima (MI355X) are recorded there and in
DESIGN.md §5.
"""
import numpy as np
import pytest

import probe_lib as P

pytestmark = pytest.mark.gpu

PI4 = 0.78539816339744830962
DBL_MAX = np.finfo(np.float64).max
DBL_MIN = np.finfo(np.float64).tiny          # smallest normal


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_exptab_accuracy_and_clamps(golden, lib_loaded):
    """ExpTab::operator() against exp(x).  Bound where the result is normal, 1.33 ulp, from
    the operations of ExpTab::raw: the table entry T[j] is rounded (0.5 ulp), the final
    fma rounds (0.5 ulp), the degree-5 polynomial drops r^6/720 <= 3.5e-17 relative at the
    ends of the reduction interval |r| <= ln2/128 (0.315 ulp where the mantissa is near
    2), q = r p carries <= 2.3e-16 |q| (0.011 ulp) and the two-step reduction 2.3e-19
    (0.002 ulp).  The header claimed 1.13 ulp, the maximum tools/gen_exp_table.py --check
    found over uniformly random arguments, which hardly ever lie at the interval ends; an
    exact emulation of the operations gives 1.26 ulp there, as the device does (comment
    and tool corrected with this test).  Where the result is subnormal the ldexp rounds
    a second time: 1.33 + 0.5 in units of 2^-1074.  At and beyond the clamps (x <= -1000,
    x >= 710) the result is exactly 0 / inf, and every x whose exp rounds to inf gives
    inf.  raw(x) equals operator()(x) bit for bit on [-1000, 710].
    Measured (MI355X): normal 1.2599 ulp at x = 700.0515763038038, subnormal 0.50."""
    g = golden("device_math")
    x, hi, lo, lo_ulp = g["exp_x"], g["exp_hi"], g["exp_lo"], g["exp_lo_ulp"]
    got, = P.run(P.OP_EXPTAB, x)
    assert np.all(got[x <= -1000.0] == 0.0) and not np.any(np.signbit(got[x <= -1000.0]))
    assert np.all(got[x >= 710.0] == np.inf)
    over = np.isinf(hi)
    assert np.all(got[over] == np.inf), x[over][got[over] != np.inf][:5]
    fin = ~over
    # an inf where the exact value is finite counts as 2^1024 = DBL_MAX + 1 ulp
    gi = np.isinf(got) & fin
    e = P.ulp_err(np.where(gi, DBL_MAX, got), hi, lo, lo_ulp) + gi
    normal = fin & (hi >= DBL_MIN)
    sub = fin & (hi < DBL_MIN)
    assert sub.sum() > 400 and normal.sum() > 3000
    en, es = np.abs(e[normal]), np.abs(e[sub])
    print(f"ExpTab: normal max {en.max():.4f} ulp at x = {x[normal][en.argmax()]!r}; "
          f"subnormal max {es.max():.4f} x 2^-1074 at x = {x[sub][es.argmax()]!r}")
    assert en.max() <= 1.33
    assert es.max() <= 1.33 + 0.5
    inside = (x >= -1000.0) & (x <= 710.0)
    raw, = P.run(P.OP_EXPTAB_RAW, x[inside])
    np.testing.assert_array_equal(_bits(raw), _bits(got[inside]))


def test_exp_neg_equals_ocml_and_is_within_one_ulp(golden, lib_loaded):
    """exp_neg(q) has the bits of ocml's exp(-q) on every fixture argument (NaN payloads
    may differ) and is within 1 ulp of exp(-q), ocml's documented bound for double exp
    (2^-1074 units where the result is subnormal).  Far below zero (q < -709.78, outside
    what a quadratic form can produce) the header documents NaN where ocml gives inf:
    both are non-finite, so chi^2 rejects.
    Measured (MI355X): 0.8095 ulp, at q = ln2 / 2."""
    g = golden("device_math")
    q, hi = g["expneg_x"], g["expneg_hi"]
    mine, ocml = P.run(P.OP_EXP_NEG, q)
    same = (_bits(mine) == _bits(ocml)) | (np.isnan(mine) & np.isnan(ocml))
    assert np.all(same), q[~same][:8]
    fin = np.isfinite(hi)
    np.testing.assert_array_equal(mine[~fin], hi[~fin])       # NaN -> NaN
    assert np.all(mine[q > 745.2] == 0.0) and mine[q == np.inf][0] == 0.0
    e = np.abs(P.ulp_err(mine, hi, g["expneg_lo"], g["expneg_lo_ulp"])[fin])
    print(f"exp_neg: max {e.max():.4f} ulp at q = {q[fin][e.argmax()]!r}; "
          f"{fin.sum()} arguments, {np.sum(hi[fin] < DBL_MIN)} subnormal or zero results")
    assert e.max() <= 1.0
    mine, ocml = P.run(P.OP_EXP_NEG, g["expneg_far_x"])
    assert np.all(ocml == np.inf) and not np.any(np.isfinite(mine))


def test_sincos_small_within_one_ulp(golden, lib_loaded):
    """sincos_small on [-pi/4, pi/4], end points included: sin and cos within 1 ulp of
    the exact values (the header's "within ~1 ulp"; the Decimal emulation of
    tools/check_sincos.py gives 0.654 / 0.807).
    Measured (MI355X): sin 0.5822 ulp, cos 0.7141 ulp."""
    g = golden("device_math")
    th = g["trig_x"]
    m = np.abs(th) <= PI4
    assert m.sum() > 900 and PI4 in th[m] and -PI4 in th[m]
    s, c = P.run(P.OP_SINCOS, th[m])
    es = np.abs(P.ulp_err(s, g["trig_sin_hi"][m], g["trig_sin_lo"][m]))
    ec = np.abs(P.ulp_err(c, g["trig_cos_hi"][m], g["trig_cos_lo"][m]))
    print(f"sincos_small: sin max {es.max():.4f} ulp at {th[m][es.argmax()]!r}, "
          f"cos max {ec.max():.4f} ulp at {th[m][ec.argmax()]!r}")
    assert es.max() <= 1.0 and ec.max() <= 1.0
    z = th[m] == 0.0
    assert np.all(s[z] == 0.0) and np.all(c[z] == 1.0)


def test_make_trig_fast_against_exact_values(golden, lib_loaded):
    """make_trig<true> on |theta| <= 50: cos^2, sin^2 and sin 2 theta = 2 (s c) each carry
    the two factors' errors (<= 1 ulp each: sincos_small above, ocml's sincos beyond
    pi/4) and one rounding of the product, <= 3.5 ulp of the exact value.  The distance
    to make_trig<false> (ocml sin / cos, sin(2 theta) direct) is recorded; both are within
    3.5 ulp of the same exact value, so it cannot exceed 7.  NaN in gives NaN out.
    Across |theta| = pi/4, where the polynomial hands over to ocml's sincos, the step
    between neighbouring arguments equals the exact function's step within 2 ulp of the
    result (cos^2 and sin^2 themselves move by 1 to 2 ulp per argument there, so the raw
    difference of neighbours, up to 3 ulp, says nothing about the seam).
    Measured (MI355X): against the exact values cos^2 1.68, sin^2 1.97, sin 2t 2.30 ulp;
    FAST against EXACT cos^2 2, sin^2 3, sin 2t 2 ulp (the header said "<= 2 ulp apart":
    corrected); steps at the seam within 1 ulp of the exact step."""
    g = golden("device_math")
    th = g["trig_x"]
    fast = P.run(P.OP_TRIG_FAST, th)
    exact = P.run(P.OP_TRIG_EXACT, th)
    small = np.abs(th) <= PI4
    assert small.sum() > 900 and (~small).sum() > 400
    for k, name in enumerate(("c2", "s2", "s2t")):
        hi, lo = g[f"trig_{name}_hi"], g[f"trig_{name}_lo"]
        e = np.abs(P.ulp_err(fast[k], hi, lo))
        d = np.abs(fast[k] - exact[k]) / P.ulp_of(hi, lo)
        print(f"make_trig<true> {name}: max {e[small].max():.4f} ulp (|th| <= pi/4), "
              f"{e[~small].max():.4f} ulp beyond; FAST vs EXACT {d[small].max():.2f} / "
              f"{d[~small].max():.2f} ulp")
        assert e.max() <= 3.5, (name, th[e.argmax()])
        assert d.max() <= 7.0
    # the seam: the 4 doubles on either side of +-pi/4 and pi/4 itself, in order
    for sgn in (1.0, -1.0):
        b = np.array([sgn * PI4]).view(np.int64)[0]
        nb = (b + np.arange(-4, 5)).view(np.float64)
        idx = np.array([np.nonzero(th == v)[0][0] for v in nb])
        assert np.sum(np.abs(th[idx]) <= PI4) == 5
        for k, name in enumerate(("c2", "s2", "s2t")):
            hi, lo = g[f"trig_{name}_hi"][idx], g[f"trig_{name}_lo"][idx]
            step = np.diff(fast[k][idx])
            true = np.diff(hi) + np.diff(lo)
            u = np.spacing(np.maximum(np.abs(hi[1:]), np.abs(hi[:-1])))
            print(f"seam {sgn:+.0f} pi/4 {name}: steps {np.round(step / u, 2)} ulp, "
                  f"off the exact step by max {np.abs(step - true).max() / u.max():.2f}")
            assert np.all(np.abs(step - true) <= 2.0 * u), (name, sgn)
    bad = P.run(P.OP_TRIG_FAST, np.array([np.nan, 0.3]))
    assert all(np.isnan(v[0]) and np.isfinite(v[1]) for v in bad)


def test_make_coef_fast_against_exact(lib_loaded):
    """make_coef<true> (two reciprocal variances, the polynomial sincos) against
    make_coef<false> (the reference's six divisions, ocml trig) over sigma in
    [0.25, 30]^2 x theta: (a, b, c) agree within 1e-12 / 700 = 1.43e-15 relative to
    max(|a|, |c|).  The exponent of a pixel is a dx^2 + b dx dy + c dy^2, and the guards
    admit exponents up to ~700 (Qb < 700 + ...), so a relative coefficient difference
    eps moves a pixel by at most 700 eps relative: 700 x 1.43e-15 = 1e-12, the FAST model
    tolerance.  Expected from the parts: <= 3 ulp between the trig terms plus one more
    rounding (reciprocal then product instead of one division), ~5e-16.
    Measured (MI355X): a 5.6e-16, b 8.4e-16, c 5.5e-16; x 700 = 5.9e-13."""
    rs = np.random.RandomState(5)
    n = 40000
    sx = np.exp(rs.uniform(np.log(0.25), np.log(30.0), n))
    sy = np.exp(rs.uniform(np.log(0.25), np.log(30.0), n))
    th = np.where(rs.rand(n) < 0.5, rs.uniform(-PI4, PI4, n), rs.uniform(-np.pi, np.pi, n))
    # corners of the sigma range and the trig seam
    sx[:8] = [0.25, 0.25, 30.0, 30.0, 0.25, 30.0, 2.138, 2.138]
    sy[:8] = [0.25, 30.0, 0.25, 30.0, 0.25, 30.0, 2.138, 30.0]
    th[:8] = [PI4, -PI4, np.nextafter(PI4, 1), 0.0, 0.6, -0.6, 0.0, PI4]
    f = np.array(P.run(P.OP_COEF_FAST, sx, sy, th))
    e = np.array(P.run(P.OP_COEF_EXACT, sx, sy, th))
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(e))
    scale = np.maximum(np.abs(e[0]), np.abs(e[2]))
    rel = np.abs(f - e) / scale
    worst = rel.max(axis=1)
    print(f"make_coef FAST vs EXACT rel to max(|a|,|c|): a {worst[0]:.3e}, b {worst[1]:.3e}, "
          f"c {worst[2]:.3e}; x 700 = {700 * worst.max():.3e}")
    assert 700.0 * worst.max() <= 1e-12
    # and against float64 NumPy's form of the reference's expressions, loosely: a wrong
    # formula, not rounding, is what this catches
    a = 0.5 * (np.cos(th) ** 2 / sx ** 2 + np.sin(th) ** 2 / sy ** 2)
    b = 0.5 * (np.sin(2 * th) / sx ** 2 - np.sin(2 * th) / sy ** 2)
    c = 0.5 * (np.sin(th) ** 2 / sx ** 2 + np.cos(th) ** 2 / sy ** 2)
    assert np.max(np.abs(e - np.array([a, b, c])) / scale) <= 4e-15


def test_accept_threshold(golden, lib_loaded):
    """accept_threshold(u) = -2 log(u) within 2 ulp for u > 0 (1 ulp of ocml's log; the
    multiplication by 2 is exact), and exactly the header's constant for u = 0 -- the
    smallest d for which exp(-d/2) rounds to 0 in double (asserted by the fixture's
    generator), so dice = 0 accepts exactly where the reference's dice < exp(-d/2) does.
    For every u and a grid of d around the threshold, d < thr(u) equals the exact
    u < exp(-d/2) except within 4 ulp of -2 ln u, the documented flip zone.
    Measured (MI355X): 0.5737 ulp; 674 of 35,424 decisions differ, all within 1 ulp."""
    g = golden("device_math")
    u, hi, lo = g["log_x"], g["log_hi"], g["log_lo"]
    thr0 = g["thr0"][0]
    thr, = P.run(P.OP_THRESHOLD, u)
    pos = u > 0.0
    assert (~pos).sum() == 1 and thr[~pos][0] == thr0 == 1490.2664382038824
    e = np.abs(P.ulp_err(thr[pos], hi[pos], lo[pos]))
    print(f"accept_threshold: max {e.max():.4f} ulp at u = {u[pos][e.argmax()]!r}")
    assert e.max() <= 2.0
    # u < exp(-d/2)  <=>  d < -2 ln u = hi + lo, decided exactly from the pair
    ks = np.array([-4096, -64, -16, -8, -6, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 8, 16, 64,
                   4096], np.float64)
    up, hp, lp, tp = u[pos], hi[pos], lo[pos], thr[pos]
    ulp = P.ulp_of(hp, lp)
    d = np.concatenate([hp[:, None] + ks[None, :] * ulp[:, None],
                        hp[:, None] * np.array([0.0, 0.5, 0.999, 1.001, 2.0])[None, :],
                        np.full((hp.size, 1), thr0)], axis=1)
    exact = (d < hp[:, None]) | ((d == hp[:, None]) & (lp[:, None] > 0.0))
    dev = d < tp[:, None]
    flip = dev != exact
    dist = np.abs(d - hp[:, None]) / ulp[:, None]
    print(f"accept decisions: {flip.sum()} of {flip.size} differ, all within "
          f"{dist[flip].max() if flip.any() else 0:.0f} ulp of the threshold")
    assert np.all(dist[flip] <= 4.0)
    # dice = 0: the reference accepts iff exp(-d/2) > 0 in double, i.e. d < thr0 (the
    # generator's check_threshold_constant, rerun by tests/test_device_math_golden.py)
    d0 = (np.array([thr0]).view(np.int64)[0] + np.arange(-50, 51)).view(np.float64)
    np.testing.assert_array_equal(d0 < thr[~pos][0], np.arange(-50, 51) < 0)
