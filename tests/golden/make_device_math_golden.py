"""Exact values for the device math primitives: tests/golden/device_math.npz.

For every input the fixture holds ``hi``, the correctly rounded double of the true value,
and ``lo`` = true - hi rounded to a double, both from mpmath at 240 bits; a test measures
an error in ulp as (got - hi - lo) / ulp(hi).  Where the true value is subnormal, lo is
below the smallest double, so the exp fixtures also carry ``lo_ulp`` = (true - hi) in
units of ulp(hi) (2^-1074 there) as float32.

Groups (arrays ``<group>_x`` + values):
  exp     exp(x) for ExpTab: operator() on all of it, raw on [-1000, 710]
  expneg  exp(-q) for exp_neg: the argument classes of tools/micro/exp_check.hip, thinned
  trig    sin, cos, cos^2, sin^2, sin(2 th): |th| <= pi/4 (sincos_small, make_trig<true>)
          and pi/4 < |th| <= 50 (make_trig<true> only)
  log     -2 ln u for accept_threshold

Run from the repository root:  python tests/golden/make_device_math_golden.py
(needs mpmath; the tests read the file with NumPy alone).
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "device_math.npz")
PREC = 240

LN2 = math.log(2.0)
PI4 = 0.78539816339744830962           # the double make_trig compares with
THR0 = 1490.2664382038824              # accept_threshold(0), olpe_device.h


def _mp():
    import mpmath
    mpmath.mp.prec = PREC
    return mpmath


def round_double(v):
    """(hi, lo, lo_ulp) of an mpmath real v: hi the nearest double (ties to even,
    subnormals and overflow to inf included), lo = float(v - hi), lo_ulp = (v - hi) /
    ulp(hi) with ulp(hi) the spacing of doubles at v."""
    mp = _mp()
    v = mp.mpf(v)
    if v == 0:
        return 0.0, 0.0, 0.0
    if mp.isnan(v):
        return math.nan, 0.0, 0.0
    if mp.isinf(v):
        return (math.inf if v > 0 else -math.inf), 0.0, 0.0
    sign, man, exp, bc = v._mpf_
    e2 = exp + bc - 1                       # floor(log2 |v|)
    ue = max(e2 - 52, -1074)                # exponent of the ulp at v
    shift = ue - exp
    if shift <= 0:
        n = man << -shift
    else:
        n, rem = man >> shift, man & ((1 << shift) - 1)
        half = 1 << (shift - 1)
        if rem > half or (rem == half and (n & 1)):
            n += 1
    if ue > 971 or (n >= (1 << 53) and ue == 971):   # at or past 2^1024
        hi = math.inf
    else:
        hi = math.ldexp(float(n), ue)       # n <= 2^53: exact
    if sign:
        hi = -hi
    if math.isinf(hi):
        return hi, 0.0, 0.0
    d = v - mp.mpf(hi)
    return hi, float(d), float(mp.ldexp(d, -ue))


def _table(f, xs):
    out = np.array([round_double(f(x)) for x in xs], dtype=np.float64).reshape(-1, 3)
    return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].astype(np.float32)


def exact_exp(xs):
    mp = _mp()

    def f(x):
        if math.isinf(x):
            return mp.inf if x > 0 else mp.mpf(0)
        if x > 800.0:
            return mp.inf                   # far above the overflow point 709.78
        if x < -900.0:
            return mp.mpf(0)                # far below the underflow point -745.13
        return mp.exp(mp.mpf(x))
    return _table(f, xs)


def exact_expneg(qs):
    mp = _mp()

    def f(q):
        if math.isnan(q):
            return mp.nan
        if q > 900.0:
            return mp.mpf(0)
        if q < -800.0:
            return mp.inf
        return mp.exp(-mp.mpf(q))
    return _table(f, qs)


def exact_trig(ths):
    """{name: (hi, lo)} of sin, cos, cos^2, sin^2, sin(2 th)."""
    mp = _mp()
    fs = {"sin": mp.sin, "cos": mp.cos, "c2": lambda t: mp.cos(t) ** 2,
          "s2": lambda t: mp.sin(t) ** 2, "s2t": lambda t: mp.sin(2 * t)}
    out = {}
    for k, f in fs.items():
        hi, lo, _ = _table(lambda x: f(mp.mpf(x)), ths)
        out[k] = (hi, lo)
    return out


def exact_m2log(us):
    mp = _mp()
    return _table(lambda u: mp.inf if u == 0.0 else -2 * mp.log(mp.mpf(u)), us)


def _steps(x, ks):
    """x moved by k doubles, for k in ks."""
    b = np.array([x], np.float64).view(np.int64)[0]
    out = (b + (np.asarray(ks, np.int64) if x > 0 else -np.asarray(ks, np.int64)))
    return out.view(np.float64)


def exp_inputs():
    rs = np.random.RandomState(20260301)
    x = [rs.uniform(-745.2, 709.8, 2200), rs.uniform(-2.0, 2.0, 300)]
    # reduction boundaries: x = k ln2/64 (r = 0) and (k + 1/2) ln2/64 (rint flips)
    for c in (0.0, 1.0, -1.0, 600.0, -600.0, 700.0, -700.0):
        k0 = int(round(c * 64.0 / LN2))
        for k in range(k0 - 4, k0 + 5):
            for h in (0.0, 0.5):
                b = (k + h) * LN2 / 64.0
                if b != 0.0:
                    x.append(_steps(b, range(-3, 4)))
    # first subnormal result, last nonzero result, overflow point
    ks = np.concatenate([np.arange(-2000, 2001, 16), np.arange(-12, 13)])
    for e in (-708.3964185322641, -745.1332191019411, 709.782712893384):
        x.append(_steps(e, ks))
    x.append([0.0, -0.0, -1000.0, 710.0, np.nextafter(-1000.0, 0), np.nextafter(710.0, 0),
              -1000.5, -1e4, -1e300, -np.inf, 710.5, 1e4, 1e300, np.inf,
              -750.0, -800.0, -999.0, 709.9, 1e-300, -1e-300, 5e-324, 1e-17, -1e-17])
    return np.unique(np.concatenate([np.asarray(a, np.float64).ravel() for a in x]))


def expneg_inputs():
    """tools/micro/exp_check.hip's classes: a dense grid of [0, 1100), random positive
    bit patterns, random [0, 800), the neighbourhoods of the range edges, specials; and
    two arguments far below zero (documented: NaN where ocml gives inf)."""
    rs = np.random.RandomState(20260302)
    q = [1100.0 * np.arange(900) / 900.0]
    bits = rs.randint(0, 2 ** 63 - 1, size=600, dtype=np.int64)
    q.append(bits.view(np.float64))
    q.append(800.0 * rs.randint(0, 2 ** 53, size=1500, dtype=np.int64).astype(np.float64) * 2.0 ** -53)
    ks = np.concatenate([np.arange(-2000, 2001, 40), np.arange(-8, 9)])
    for e in (708.3964185322641, 709.782712893384, 745.1332191019411, 745.1332191019412,
              1000.0, 0.5 * 0.6931471805599453):
        base = np.nextafter(e, np.where(ks < 0, 0.0, 2e3))
        q.append(base + ks.astype(np.float64) * 1e-13 * e)
    q.append([0.0, -0.0, np.inf, np.nan, 1e-300, -1e-300, -1e-12, -1e-6, -0.3, 4.9e-324,
              1e300, 1e308])
    q = np.concatenate([np.asarray(a, np.float64).ravel() for a in q])
    q = q[~np.isnan(q)]
    return np.concatenate([np.unique(q), [np.nan]]), np.array([-710.0, -800.0])


def trig_inputs():
    rs = np.random.RandomState(20260303)
    small = [rs.uniform(-PI4, PI4, 900), [PI4, -PI4], _steps(PI4, range(-4, 0)),
             _steps(-PI4, range(1, 5)),
             [0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 1e-20, -1e-20, 1e-8, -1e-8,
              1e-4, -1e-4, 0.5, -0.5]]
    big = [_steps(PI4, range(1, 5)), _steps(-PI4, range(-4, 0)),
           rs.uniform(PI4, 50.0, 250), -rs.uniform(PI4, 50.0, 250),
           [math.pi / 2, -math.pi / 2, math.pi, 50.0, -50.0, 1.0, -1.0]]
    cat = lambda a: np.concatenate([np.asarray(v, np.float64).ravel() for v in a])
    s, b = cat(small), cat(big)
    assert np.all(np.abs(s) <= PI4) and np.all(np.abs(b) > PI4) and np.all(np.abs(b) <= 50.0)
    return np.concatenate([s, b])


def log_inputs():
    rs = np.random.RandomState(20260304)
    u = [np.arange(1, 65) * 2.0 ** -53, 2.0 ** -np.arange(1, 53.0),
         rs.randint(0, 2 ** 53, size=1200, dtype=np.int64).astype(np.float64) * 2.0 ** -53,
         [1.0 - 2.0 ** -53, 1.0 - 2.0 ** -52, 0.5, 0.0]]
    u = np.concatenate([np.asarray(a, np.float64).ravel() for a in u])
    assert np.all((u >= 0.0) & (u < 1.0))          # rand() of the sampler: [0, 1)
    return np.unique(u)


def check_threshold_constant():
    """accept_threshold(0) is the smallest double d for which exp(-d/2) rounds to 0."""
    mp = _mp()
    assert round_double(mp.exp(-mp.mpf(THR0) / 2))[0] == 0.0
    below = float(np.nextafter(THR0, 0.0))
    assert round_double(mp.exp(-mp.mpf(below) / 2))[0] == 5e-324


def generate():
    check_threshold_constant()
    d = {}
    x = exp_inputs()
    d["exp_x"] = x
    d["exp_hi"], d["exp_lo"], d["exp_lo_ulp"] = exact_exp(x)
    q, qneg = expneg_inputs()
    d["expneg_x"] = q
    d["expneg_hi"], d["expneg_lo"], d["expneg_lo_ulp"] = exact_expneg(q)
    d["expneg_far_x"] = qneg
    th = trig_inputs()
    d["trig_x"] = th
    for k, (hi, lo) in exact_trig(th).items():
        d[f"trig_{k}_hi"], d[f"trig_{k}_lo"] = hi, lo
    u = log_inputs()
    d["log_x"] = u
    d["log_hi"], d["log_lo"], _ = exact_m2log(u)
    d["thr0"] = np.array([THR0])
    return d


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes;",
          ", ".join(f"{k}: {v.size}" for k, v in data.items() if k.endswith("_x")))
    sys.exit(0)
