"""ctypes binding of the tests' device probe (tests/c/device_probe.hip, built by
olpefit_amd/build.py into olpefit_amd/libolpe_probe.so) and the ulp arithmetic of the
exact-value fixture (tests/golden/device_math.npz).  No fallback: a missing probe
library raises, so the GPU tests that need it fail."""
import ctypes as C
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_PATH = os.path.join(REPO, "olpefit_amd", "libolpe_probe.so")

(OP_EXPTAB, OP_EXPTAB_RAW, OP_EXP_NEG, OP_SINCOS, OP_TRIG_FAST, OP_TRIG_EXACT, OP_COEF_FAST,
 OP_COEF_EXACT, OP_THRESHOLD) = range(9)

_probe = None


def load():
    global _probe
    if _probe is None:
        if not os.path.exists(PROBE_PATH):
            raise OSError(f"{PROBE_PATH} not found: build it with `python -m olpefit_amd.build`")
        lib = C.CDLL(PROBE_PATH)
        pd = C.POINTER(C.c_double)
        lib.olpe_probe_nin.argtypes = lib.olpe_probe_nout.argtypes = [C.c_int]
        lib.olpe_probe_run.argtypes = [C.c_int, pd, C.c_longlong, pd]
        lib.olpe_probe_guards.argtypes = [C.c_int, C.c_int, C.c_int, pd, C.c_int,
                                          C.POINTER(C.c_uint32)]
        _probe = lib
    return _probe


def run(op, *inputs):
    """The op's outputs (a tuple of arrays) for equally long input arrays."""
    lib = load()
    assert len(inputs) == lib.olpe_probe_nin(op)
    x = np.ascontiguousarray(np.stack([np.asarray(a, np.float64).ravel() for a in inputs]))
    n = x.shape[1]
    out = np.full((lib.olpe_probe_nout(op), n), np.nan)
    pd = C.POINTER(C.c_double)
    rc = lib.olpe_probe_run(op, x.ctypes.data_as(pd), n, out.ctypes.data_as(pd))
    assert rc == 0, f"probe op {op}: HIP status {rc}"
    return tuple(out)


def guards(nsrc, n, params, bkgd_mode=1):
    """Per parameter vector: (fast3_fails mask, fast3_cols_pass mask over those,
    fast3_amp_ok over those, fast_level) of the FAST model descriptor at cutout size n."""
    lib = load()
    p = np.ascontiguousarray(np.atleast_2d(np.asarray(params, np.float64)))
    assert p.shape[1] == (17 if nsrc == 2 else 20)
    out = np.zeros((p.shape[0], 4), np.uint32)
    rc = lib.olpe_probe_guards(nsrc, n, bkgd_mode, p.ctypes.data_as(C.POINTER(C.c_double)),
                               p.shape[0], out.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 0, f"guard probe: HIP status {rc}"
    return out.astype(np.int64)


def ulp_of(hi, lo):
    """Spacing of the doubles at the true value hi + lo (hi its nearest double): the
    spacing below hi where hi is a power of two and the true value lies below it;
    2^-1074 for subnormals."""
    a = np.abs(hi)
    with np.errstate(invalid="ignore"):
        u = np.spacing(a)
        m, _ = np.frexp(a)
        below = (m == 0.5) & (np.sign(lo) * np.sign(hi) < 0) & (a > 2.2250738585072014e-308)
    return np.where(below, u / 2, u)


def ulp_err(got, hi, lo, lo_ulp=None):
    """(got - hi - lo) / ulp(hi), elementwise; with lo_ulp (the residual in ulp) where
    given, which also serves subnormal values.  Entries whose hi is not finite are NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        u = ulp_of(hi, lo)
        d = (got - hi) / u
        e = d - (lo / u if lo_ulp is None else lo_ulp.astype(np.float64))
    return np.where(np.isfinite(hi), e, np.nan)


def lognormal_proposal_error(r, new, cur, ref_new, ref_cur, lognorm):
    """Relative distance of the traced log-normal proposals from the reference's of the
    same step: |new - ref_new| / |ref_new| where the step starts from the same current
    value, else (the states already differ by rounding) the distance of the ratios
    new / cur.  r, new, cur, ref_new, ref_cur: per step; returns (errors of the
    log-normal steps with a positive current value, their x = ln(ref_new / ref_cur))."""
    r = np.asarray(r).astype(int)
    m = np.isin(r, lognorm) & (ref_cur > 0) & np.isfinite(ref_new)
    new, cur, ref_new, ref_cur = (np.asarray(v, np.float64)[m] for v in (new, cur, ref_new, ref_cur))
    same = cur == ref_cur
    with np.errstate(all="ignore"):
        direct = np.abs(new - ref_new) / np.abs(ref_new)
        ratio = np.abs(new / cur - ref_new / ref_cur) / np.abs(ref_new / ref_cur)
        x = np.log(ref_new / ref_cur)
    return np.where(same, direct, ratio), x
