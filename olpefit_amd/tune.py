"""The sampler's proposal widths on the host: the reference's defaults, the update rule of
the device tuner restated in NumPy, and the widths file the CLIs exchange.

The widths (apf_step2.py:234; 3body/apf_step2_3body.py:220-238) are the scale of each
parameter's one-dimensional proposal: ``loc + w gauss()`` for a proposed parameter,
``10**(log10 loc + w gauss())`` (w in dex) for a log-proposed one.  A ``Sampler`` carries its
own (``set_widths`` / ``get_widths``) and can adapt them from the ensemble's acceptance
rates between launches (``tune_begin`` / ``tune_step``; include/olpe.h states the rule,
``update`` below is the same arithmetic).

The widths file is JSON::

    {"format": "olpefit-widths-1", "nsrc": 2, "names": [...P names...],
     "widths": [...P values...], "source": "given" | "tuned" | "covariance" | "laplace",
     "history": {"target", "gain", "dT" [k][P], "dA" [k][P], "widths" [k][P]}}   (tuned only)

Values are written with ``repr`` precision (``json`` does), so a file round-trips bit for
bit.  Nothing here needs a GPU.
"""
from __future__ import annotations

import json
import math

import numpy as np

from .step3 import NAMES_2, NAMES_3

FORMAT = "olpefit-widths-1"
SOURCES = ("given", "tuned", "covariance", "laplace")

#: apf_step2.py:234 and 3body/apf_step2_3body.py:220-238 (the device's own copy is
#: olpe.hip's c_widths2 / c_widths3; tests/test_widths_cpu.py compares the two texts)
DEFAULT_WIDTHS_2 = (0.01, 0.01, 0.3, 0.3, 0.08, 0.09, 0.0025, 0.02, 0.001, 0.0008, 0.002, 0.002,
                    0.001, 0.001, 0.008, 0.01)
DEFAULT_WIDTHS_3 = (0.01, 0.01, 0.3, 0.3, 0.3, 0.3, 0.08, 0.09, 0.0025, 0.02, 0.02, 0.001,
                    0.0008, 0.002, 0.002, 0.001, 0.001, 0.008, 0.01)
#: lognorm (apf_step2.py:217; 3body :295): the log-proposed parameters
LOG_PARAMS_2 = (6, 7, 9, 10, 11, 12, 13)
LOG_PARAMS_3 = (8, 9, 10, 12, 13, 14, 15, 16)
#: the tuner's clamps, as factors of the default (powers of two: exact)
CLAMP_LO, CLAMP_HI = 1.0 / 1024.0, 64.0


def _nsrc(nsrc: int) -> int:
    if nsrc not in (2, 3):
        raise ValueError("nsrc must be 2 or 3")
    return nsrc


def default_widths(nsrc: int) -> np.ndarray:
    return np.array(DEFAULT_WIDTHS_2 if _nsrc(nsrc) == 2 else DEFAULT_WIDTHS_3, dtype=np.float64)


def log_params(nsrc: int) -> tuple:
    return LOG_PARAMS_2 if _nsrc(nsrc) == 2 else LOG_PARAMS_3


def param_names(nsrc: int) -> list:
    """The P proposable parameters' names (step 3's column names without chi^2)."""
    return list((NAMES_2 if _nsrc(nsrc) == 2 else NAMES_3)[:-1])


def update(widths, dT, dA, k: int, target: float, gain: float, defaults):
    """Step k (1-based) of the device tuner on the host, bit for bit: for dT_j > 0,
    a = dA_j / dT_j, f = 1 + (gain / sqrt(k)) (a - target), w_j <- min(max(w_j f,
    default_j / 1024), default_j * 64); dT_j <= 0 keeps w_j."""
    w = np.array(widths, dtype=np.float64)
    d = np.asarray(defaults, dtype=np.float64)
    g = np.float64(gain) / np.float64(math.sqrt(float(k)))
    for j in range(w.size):
        if int(dT[j]) > 0:
            a = np.float64(int(dA[j])) / np.float64(int(dT[j]))
            f = np.float64(1.0) + g * (a - np.float64(target))
            v = w[j] * f
            lo, hi = d[j] / np.float64(1024.0), d[j] * np.float64(64.0)
            v = lo if v < lo else v
            v = hi if v > hi else v
            w[j] = v
    return w


def widths_doc(nsrc: int, widths, source: str = "given", history=None) -> dict:
    """The widths file's content.  ``history``: (target, gain, dT, dA, widths) of a tuning
    session, required for -- and only written with -- source "tuned"."""
    w = np.asarray(widths, dtype=np.float64)
    names = param_names(nsrc)
    if w.shape != (len(names),):
        raise ValueError(f"{w.size} widths for {len(names)} parameters (nsrc {nsrc})")
    if source not in SOURCES:
        raise ValueError(f"source must be one of {SOURCES}")
    if not (np.isfinite(w).all() and (w > 0).all()):
        raise ValueError("widths must be finite and > 0")
    doc = {"format": FORMAT, "nsrc": int(nsrc), "names": names, "widths": [float(v) for v in w],
           "source": source}
    if source == "tuned":
        if history is None:
            raise ValueError("a tuned widths file carries its history")
        target, gain, dT, dA, hw = history
        doc["history"] = {"target": float(target), "gain": float(gain),
                          "dT": np.asarray(dT, dtype=np.int64).tolist(),
                          "dA": np.asarray(dA, dtype=np.int64).tolist(),
                          "widths": [[float(v) for v in row] for row in np.asarray(hw)]}
    return doc


def save_widths(path, nsrc: int, widths, source: str = "given", history=None) -> dict:
    doc = widths_doc(nsrc, widths, source, history)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


def load_doc(path, nsrc: int) -> dict:
    """The file's content, checked: the format tag, ``nsrc``, the number of widths and
    their names, finite positive values.  Raises ValueError otherwise."""
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or doc.get("format") != FORMAT:
        raise ValueError(f"{path}: not a widths file ({FORMAT})")
    names = param_names(nsrc)
    if doc.get("nsrc") != nsrc:
        raise ValueError(f"{path}: written for nsrc {doc.get('nsrc')}, this run has nsrc {nsrc}")
    w = doc.get("widths")
    if not isinstance(w, list) or len(w) != len(names):
        raise ValueError(f"{path}: {len(w) if isinstance(w, list) else 'no'} widths, "
                         f"nsrc {nsrc} has {len(names)} parameters")
    if doc.get("names") != names:
        raise ValueError(f"{path}: parameter names differ from {names}")
    w = np.array(w, dtype=np.float64)
    if not (np.isfinite(w).all() and (w > 0).all()):
        raise ValueError(f"{path}: widths must be finite and > 0")
    return doc


def load_widths(path, nsrc: int) -> np.ndarray:
    """The P widths of a widths file for ``nsrc`` sources (ValueError on a wrong length,
    another ``nsrc``, other names or a value that is not finite and > 0)."""
    return np.array(load_doc(path, nsrc)["widths"], dtype=np.float64)
