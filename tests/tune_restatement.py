"""The device tuner's update rule (include/olpe.h, olpe_tune_step) restated in NumPy
scalars, one IEEE double operation per line in the stated order, independent of
olpefit_amd.tune.update: what tests/test_widths_cpu.py pins to exact rationals and the
GPU tests compare the device's log with, bit for bit.
"""
import math

import numpy as np

from oracle import olpe_oracle as ora

CLAMP_LO_DIV, CLAMP_HI_MUL = 1024.0, 64.0


def defaults(nsrc):
    """The reference's widths (apf_step2.py:234; 3body :220-238) as the oracle holds them."""
    return np.array(ora.layout(nsrc)[1], dtype=np.float64)


def gain_at(gain, k):
    """g_k = gain / sqrt(k), formed in double as the host library forms it."""
    return np.float64(gain) / np.float64(math.sqrt(float(k)))


def factor(dT, dA, k, target, gain):
    """f of one parameter with dT > 0."""
    a = np.float64(int(dA)) / np.float64(int(dT))
    d = a - np.float64(target)
    p = gain_at(gain, k) * d
    return np.float64(1.0) + p


def step(w, dT, dA, k, target, gain, dflt):
    """The widths after step k (1-based) from the widths before it and the step's integer
    deltas; a parameter with dT <= 0 keeps its bits."""
    out = np.array(w, dtype=np.float64)
    for j in range(out.size):
        if int(dT[j]) <= 0:
            continue
        v = out[j] * factor(dT[j], dA[j], k, target, gain)
        lo = np.float64(dflt[j]) / np.float64(CLAMP_LO_DIV)
        hi = np.float64(dflt[j]) * np.float64(CLAMP_HI_MUL)
        v = max(v, lo)
        v = min(v, hi)
        out[j] = v
    return out


def replay(w0, dT, dA, target, gain, dflt):
    """The widths after every step of a session [k, P] from its starting widths and its
    logged deltas [k, P]."""
    rows, w = [], np.array(w0, dtype=np.float64)
    for i in range(len(dT)):
        w = step(w, dT[i], dA[i], i + 1, target, gain, dflt)
        rows.append(w.copy())
    return np.array(rows).reshape(len(dT), len(w0))
