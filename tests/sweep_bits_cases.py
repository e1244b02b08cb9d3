"""The cases of tests/test_gpu_sweep_bits.py and tools/record_sweep_bits.py: FAST sampler
runs of the three samplers that take the fully unrolled 64-row FAST3 sweep
(olpe_device.h sweep_fast3, NT = 64), whose chains and traces are compared bit for bit
with a recording made once (tests/data/sweep_bits.json).

Every case: 24 walkers (two workgroups of the 12-wave samplers, one and a half of the
16-wave one) from one start vector, seeds 1000.., 300 iterations, stride 1, trace on.
 * step1-*: the step-1 style start (oracle.initial_parameters of the guess) on the
   synthetic frame;
 * edge-*: a frame whose two sources sit at rows 2.3 and 61.7 (the first and the last
   group of 16 shape-table rows carry their cores), started at its truth.
"""
import functools
import hashlib
import json
import os

import numpy as np

from oracle import olpe_oracle as ora

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDING = os.path.join(REPO, "tests", "data", "sweep_bits.json")

N = 64
WALKERS, ITERS = 24, 300
SEEDS = tuple(range(1000, 1000 + WALKERS))
EDGE_ROWS = (2.3, 61.7)

# id -> (sources, start, environment of the run)
CASES = {
    "step1-2src-wpb12": (2, "step1", {"OLPE_WPB": "12"}),
    "step1-2src-wpb16": (2, "step1", {"OLPE_WPB": "16"}),
    "step1-3src": (3, "step1", {}),
    "edge-2src-wpb12": (2, "edge", {"OLPE_WPB": "12"}),
    "edge-2src-wpb16": (2, "edge", {"OLPE_WPB": "16"}),
}

# the shape parameters of the two sets (trace column 0), per source count
NARROW = {2: (10, 11, 14), 3: (13, 14, 17)}       # S1X S1Y T1
WIDE = {2: (12, 13, 15), 3: (15, 16, 18)}         # S2X S2Y T2


@functools.lru_cache(maxsize=None)
def frame(nsrc, start):
    """(image, nan-masked data, err, start vector with its chi^2) of a case's frame."""
    from olpefit_amd import synth
    if start == "step1":
        img, _ = synth.make_image(N, nsrc, 3)
    else:
        p = synth.truth_params(N, nsrc)
        p[1], p[3] = EDGE_ROWS
        m = synth.render(p, N, nsrc)
        noise = np.random.RandomState(3).normal(0.0, 1.0, size=(N, N)) * np.sqrt(38.0 ** 2 + np.abs(m))
        img = (m + noise).astype(np.float32)
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    if start == "step1":
        p0 = ora.initial_parameters(img, synth.guess_values(N, nsrc), nsrc)
    else:
        p0 = np.append(p, 0.0)
    with np.errstate(all="ignore"):
        p0[-1] = float(ora.chi_squared(dm, ora.build_analytical_model(p0, N, nsrc), err))
    assert np.isfinite(p0[-1])
    return img, dm, err, p0


def run_case(cid, setenv, delenv):
    """(chain, trace, final state) of case cid; setenv / delenv set and remove
    environment variables (a test passes its monkeypatch's)."""
    from olpefit_amd.core import Sampler
    nsrc, start, env = CASES[cid]
    for k in ("OLPE_RING", "OLPE_WPB"):
        delenv(k)
    for k, v in env.items():
        setenv(k, v)
    img, _, _, p0 = frame(nsrc, start)
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    try:
        s.set_eval_mode("fast")
        s.seed(np.array(SEEDS))
        s.set_state(np.tile(p0, (WALKERS, 1)))
        s.enable_trace(True)
        chain = s.run(ITERS, burn_in=0, record_stride=1)
        tr = s.trace(ITERS)
        state = s.get_state()[0]
    finally:
        s.close()
    return chain, tr, state


def digest(chain, tr, state):
    """What the recording keeps of a run: SHA-256 of the chain's and the trace's bytes
    and the final states as hexadecimal floats."""
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()
    return dict(chain_sha256=sha(chain), trace_sha256=sha(tr), shape=list(chain.shape),
                final_state=[[float(v).hex() for v in row] for row in state])


def shape_outcomes(nsrc, tr):
    """{(set, accepted): count} of the run's shape proposals."""
    r = tr[:, :, 0].astype(int)
    acc = tr[:, :, 5] > 0.5
    out = {}
    for name, idx in (("narrow", NARROW[nsrc]), ("wide", WIDE[nsrc])):
        m = np.isin(r, idx)
        out[name, True] = int(np.sum(m & acc))
        out[name, False] = int(np.sum(m & ~acc))
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(nsrc, start):
    """The oracle's walkers from the case's start: (chains, accept decisions, drawn
    indices), the first three entries test_gpu_fast_guards.assert_follows_oracle reads."""
    _, dm, err, p0 = frame(nsrc, start)
    chains, acc, r = [], [], []
    for sd in SEEDS:
        wk = ora.Walker(dm, err, p0, sd, nsrc=nsrc)
        rows, a_, r_ = [], [], []
        for _ in range(ITERS):
            rec = wk.step()
            rows.append(wk.parameters.copy())
            r_.append(rec[0])
            a_.append(bool(rec[4]))
        chains.append(rows)
        acc.append(a_)
        r.append(r_)
    return np.array(chains), np.array(acc), np.array(r)


def load_recording():
    with open(RECORDING) as f:
        return json.load(f)
