"""The 64x64 FAST sampler's shape-table slots and step bookkeeping, pinned bit for bit.

The 16-wave sampler keeps one shape-table slot (a shape proposal rebuilds its set in
place, a reject leaves it stale until the next use), the 12-wave sampler two; the step
around the sweep counts tries and accepts by LDS adds (the sum read back only where
accept_min needs it) and reads the accept's dice only for the trace.  Whatever those
paths cache, swap or skip may not change a bit of any result:

 * against the parent: tests/golden/shape_slots_parent.npz holds the run below as the
   commit before the LDS-add counters computed it on an MI355X
   (tools/record_shape_slots_golden.py wrote it) -- chain at stride 1, trace (dice and
   p_accept included), state, counters, RNG state, all equal;
 * across samplers: the 12-wave sampler and 1, 3 and 7 work units per walker (a unit
   start resets every cache, so the slot histories differ);
 * against the oracle at the FAST trajectory tolerance of tests/test_gpu_parity.py;
 * with coverage as a condition: every order of accepted / rejected shape draws and what
   follows them occurs at least 4 times in every walker (the oracle alone meets that with
   these seeds: the smallest class is 4);
 * an accept_min > 0 launch (the counters' returning add), starts whose steps leave
   FAST3 (the fallback sweeps with the slots in play) and a NaN proposal (no sweep).
"""
import contextlib
import os

import numpy as np
import pytest

from oracle import olpe_oracle as ora

pytestmark = pytest.mark.gpu

N, NSRC, W, IT = 64, 2, 8, 400
SEEDS = tuple(range(1000, 1000 + W))
TRAJ_TOL = 1e-9                                # TOL["fast"]["traj"], tests/test_gpu_parity.py
ENV_KNOBS = ("OLPE_UNITS", "OLPE_NO_QUEUE", "OLPE_WPB", "OLPE_RING")
NAMES = ("chain", "trace", "state", "tries", "accepts", "mt", "gauss", "done_at")
GOLDEN = "shape_slots_parent"
NARROW, WIDE = (10, 11, 14), (12, 13, 15)      # Layout<2>: S1X S1Y T1 / S2X S2Y T2


@contextlib.contextmanager
def knobs(env):
    """The sampler-selecting environment (read when a Sampler is created), restored."""
    old = {k: os.environ.pop(k, None) for k in ENV_KNOBS}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in ENV_KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def bench_frame():
    from olpefit_amd import synth
    img, _ = synth.make_image(N, NSRC, 0)
    return img


def bench_start(img):
    """bench.py's start: the step-1 style initial parameters of the synthetic frame with
    the FAST chi^2 of the device."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    p0 = np.array(initial_parameters(img, synth.guess_values(N, NSRC), NSRC), np.float64)
    with knobs({}):
        s = Sampler(img, 1.0, 1, 1, 2, nsrc=NSRC)
        p0[-1] = s.chi_squared(p0)
        s.close()
    return p0


def run(img, p0, env, seeds=SEEDS, n_it=IT, accept_min=0, start_chi=False):
    """{name: array} of one launch of n_it iterations, trace on, chain at stride 1
    (start_chi: the start's chi^2 slot is filled by the device first)."""
    from olpefit_amd.core import Sampler
    with knobs(env):
        s = Sampler(img, 1.0, 1, 1, 2, nsrc=NSRC)
        try:
            s.set_eval_mode("fast")
            if start_chi:
                p0 = np.array(p0, np.float64)
                p0[-1] = s.chi_squared(p0)
            s.seed(np.array(seeds))
            s.set_state(np.tile(p0, (len(seeds), 1)))
            s.enable_trace(True)
            chain = s.run(n_it, burn_in=0, record_stride=1, accept_min=accept_min)
            out = (chain, s.trace(n_it)) + s.get_state() + s.rng_state() + (s.done_at(),)
            units = s.last_units()
        finally:
            s.close()
    if "OLPE_UNITS" in env:
        assert units == int(env["OLPE_UNITS"])
    return dict(zip(NAMES, out))


def assert_same(a, b, what, names=NAMES):
    for k in names:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


def slot_classes(tr):
    """Per walker, the counts of the slot histories a run [W, IT, 6] of trace rows holds."""
    r, acc = tr[:, :, 0].astype(int), tr[:, :, 5] > 0.5
    nar, wid = np.isin(r, NARROW), np.isin(r, WIDE)
    shape = nar | wid
    s0, a0 = shape[:, :-1], acc[:, :-1]
    same = (nar[:, :-1] & nar[:, 1:]) | (wid[:, :-1] & wid[:, 1:])
    other = (nar[:, :-1] & wid[:, 1:]) | (wid[:, :-1] & nar[:, 1:])
    nxt = {"a non-shape draw": ~shape[:, 1:], "the same set": same, "the other set": other}
    out = {"accepted narrow-set draw": (nar & acc).sum(axis=1),
           "accepted wide-set draw": (wid & acc).sum(axis=1)}
    for flag, word in ((~a0, "rejected"), (a0, "accepted")):
        for name, m in nxt.items():
            out[f"{word} shape draw, then {name}"] = (s0 & flag & m).sum(axis=1)
    return out


@pytest.fixture(scope="module")
def frame(lib_loaded):
    return bench_frame()


@pytest.fixture(scope="module")
def parent(golden):
    return golden(GOLDEN)


@pytest.fixture(scope="module")
def w16(frame, parent):
    return run(frame, parent["p0"], {"OLPE_WPB": "16"})


@pytest.fixture(scope="module")
def oracle_runs(frame, parent):
    dm, err, _, _ = ora.noise_model(frame, 1.0, 1, 1, 2)
    out = []
    for sd in SEEDS:
        wk = ora.Walker(dm, err, parent["p0"], sd)
        chain, tr = wk.run(IT, trace=True)
        out.append((chain, tr, wk.total_tries.copy()))
    return out


def test_start_is_the_bench_start(frame, parent):
    p0 = bench_start(frame)
    np.testing.assert_array_equal(p0[:-1], parent["p0"][:-1])
    np.testing.assert_allclose(p0[-1], parent["p0"][-1], rtol=1e-11)


def test_bitwise_equal_to_the_parent(w16, parent):
    """Every array of the 16-wave run, the trace's dice and p_accept columns included."""
    assert_same(w16, parent, "16 waves against the parent commit's fixture")


def test_every_slot_history_occurs(w16):
    for name, cnt in slot_classes(w16["trace"]).items():
        print(f"SLOTS {name}: per walker {cnt.tolist()}")
        assert cnt.min() >= 4, (name, cnt.tolist())


@pytest.mark.parametrize("env", [{"OLPE_WPB": "12"}] +
                         [{"OLPE_WPB": "16", "OLPE_UNITS": str(u)} for u in (1, 3, 7)],
                         ids=["wpb12", "units1", "units3", "units7"])
def test_equal_across_samplers(frame, parent, w16, env):
    assert_same(w16, run(frame, parent["p0"], env), str(env))


def test_follows_the_oracle(w16, oracle_runs):
    tr = w16["trace"]
    for w, (chain, rtr, _) in enumerate(oracle_runs):
        assert np.array_equal(tr[w, :, 0].astype(int), np.array([t[0] for t in rtr]))
        assert np.array_equal(tr[w, :, 3], np.array([t[3] for t in rtr]))
        assert np.array_equal(tr[w, :, 5] > 0.5, np.array([t[4] for t in rtr], bool))
        np.testing.assert_allclose(w16["chain"][w], chain, rtol=TRAJ_TOL, atol=0,
                                   err_msg=f"walker {w}")


def test_accept_min_launch(frame, parent, oracle_runs):
    """accept_min > 0: the tries come back from the counter's add; done_at is the first
    count at which every parameter has been tried accept_min times."""
    a = run(frame, parent["p0"], {"OLPE_WPB": "16"}, accept_min=5)
    b = run(frame, parent["p0"], {"OLPE_WPB": "12"}, accept_min=5)
    assert_same(a, b, "accept_min=5, 16 against 12 waves")
    assert np.all(a["done_at"] > 0) and np.all(a["done_at"] <= IT)
    for w, (_, rtr, tries) in enumerate(oracle_runs):
        np.testing.assert_array_equal(a["tries"][w], tries)
        r = np.array([t[0] for t in rtr])
        cnt = np.cumsum(r[:, None] == np.arange(16)[None, :], axis=0)
        assert a["done_at"][w] == 1 + int(np.argmax(cnt.min(axis=1) >= 5))


def fallback_start(which):
    """(frame, start, seeds) of the two guard-edge runs, from tests/test_gpu_fast_guards.py.
    "fast2": the narrow core of case q2-64x2, 1.2 % beyond the row-step limit of the FAST3
    guard and well inside FAST2's (the companion half a pixel off the centre row): the
    walkers drift back to FAST3 through proposals on both sides, and with these seeds the
    oracle's refused proposals all take FAST2, which the 12- and 16-wave samplers share.
    "exact": the inside member of row-narrow-64x2, whose refused proposals are of
    fast_level 1 -- the V-table sweep at 12 waves, the exact sweep at 16 (which has no
    V table), so those steps' chi^2 differ between the two by rounding in the parent too."""
    import test_gpu_fast_guards as G
    if which == "fast2":
        case = G.BY_ID["q2-64x2"]
        p, seeds = case.make(0.5 * (case.n - 1) + 0.5), (900, 907, 908, 909)
    else:
        case = G.BY_ID["row-narrow-64x2"]
        p, seeds = case.pair()[0], case.seeds[:4]
    img, _, _ = G.frame(case.n, case.nsrc)
    return img, G.start_vector(p, case.n, case.nsrc), seeds


def sweeps_taken(p0, a):
    """Per walker and step: 3 where the proposal passes the FAST3 guard, otherwise its
    fast_level (the restatement of tests/test_gpu_fast_guards.py)."""
    import test_gpu_fast_guards as G
    props, _ = G.proposals(p0, a["chain"], a["trace"][:, :, 0], a["trace"][:, :, 1])
    out = np.empty(props.shape[:2], int)
    for idx in np.ndindex(*out.shape):
        st = G.guard_state(props[idx], N, NSRC)
        out[idx] = 3 if st["fast3"] else st["level"]
    return out


def test_fast2_fallback_with_the_slots(lib_loaded):
    """FAST3 steps and FAST2 steps alternate around accepted and rejected shape draws;
    16 and 12 waves are equal bit for bit."""
    img, p0, seeds = fallback_start("fast2")
    a = run(img, p0, {"OLPE_WPB": "16"}, seeds, 200)
    b = run(img, p0, {"OLPE_WPB": "12"}, seeds, 200)
    lvl = sweeps_taken(p0, a)
    print(f"FALLBACK fast2: per walker {(lvl == 3).sum(axis=1).tolist()} proposals take "
          f"FAST3, {(lvl == 2).sum(axis=1).tolist()} FAST2")
    assert np.all((lvl == 3) | (lvl == 2))
    assert np.all((lvl == 3).sum(axis=1) >= 10) and np.all((lvl == 2).sum(axis=1) >= 10)
    shape = np.isin(a["trace"][:, :, 0].astype(int), NARROW + WIDE)
    acc = a["trace"][:, :, 5] > 0.5
    for flag in (acc, ~acc):                     # shape draws of both outcomes, both sweeps
        assert np.any(shape & flag & (lvl == 3)) and np.any(shape & flag & (lvl == 2))
    assert_same(a, b, "FAST2 fallback, 16 against 12 waves")


def test_exact_fallback_with_the_slots(lib_loaded, parent):
    """FAST3 steps and steps of the 16-wave sampler's exact sweep alternate; equal to the
    parent commit's 16-wave run of the fixture bit for bit (see fallback_start for why
    not to the 12-wave sampler)."""
    img, p0, seeds = fallback_start("exact")
    np.testing.assert_allclose(p0, parent["edge_p0"], rtol=1e-12, atol=0)
    p0 = parent["edge_p0"]                       # (the host's chi^2 of the start, as recorded)
    a = run(img, p0, {"OLPE_WPB": "16"}, seeds, 200)
    lvl = sweeps_taken(p0, a)
    print(f"FALLBACK exact: per walker {(lvl == 3).sum(axis=1).tolist()} proposals take "
          f"FAST3, {(lvl < 2).sum(axis=1).tolist()} the exact sweep")
    assert (lvl == 3).sum() >= 10 and (lvl < 2).sum() >= 10
    assert np.any(a["accepts"][:, list(NARROW + WIDE)] > 0)
    assert_same(a, {k: parent["edge_" + k] for k in NAMES}, "guard edge against the parent")


def test_nan_proposals_leave_the_slots(frame, parent):
    """A background start below 0 proposes NaN at every draw of it: no sweep."""
    p0 = parent["p0"].copy()
    p0[9] = -abs(p0[9]) - 1.0
    a = run(frame, p0, {"OLPE_WPB": "16"}, SEEDS[:2], 100, start_chi=True)
    b = run(frame, p0, {"OLPE_WPB": "12"}, SEEDS[:2], 100, start_chi=True)
    r, nv = a["trace"][:, :, 0].astype(int), a["trace"][:, :, 1]
    assert np.any(r == 9) and np.all(np.isnan(nv[r == 9])) and not np.any(np.isnan(nv[r != 9]))
    assert_same(a, b, "NaN proposals, 16 against 12 waves")
