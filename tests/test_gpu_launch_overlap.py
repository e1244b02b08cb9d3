"""Consecutive sampler launches overlap ("Launch overlap"): results unchanged.

With ``OLPE_OVERLAP`` on (the default) launch k+1 starts on the other sampler stream
while launch k's tail still runs; chunk 0 of every walker waits for the tag the walker's
last chunk of launch k published.  With ``OLPE_OVERLAP=0`` every launch waits for its
predecessor's end.  Both arms must leave the same bits: the last launch's chain, states,
tries, accepts, RNG state and cached deviate, ``done_at`` and ``moments_summary`` (the
running moments cover every launch's rows, which cannot be read back between launches
without serialising them), and whatever a scenario reads on the way.

Each arm runs in a fresh child process (this file run as a script: the switch is read when
a context is created).  The child reports how many launches overlapped
(``olpe_test_overlaps``): the overlap arm must have overlapped exactly where the rules
allow it -- queue launches over the same walkers with nothing main-class between them --
and the serial arm nowhere.  ``olpe_sync`` at the end of every scenario raises if a
hand-off poll reached its time limit, so a child that exits 0 had a clear error word.

"Chain order": ``chain()`` reads the last launch enqueued; with two launches queued back
to back whose row counts differ, it must return the second one's rows (each launch parity
has a chain buffer of its own), and reading after every launch must return that launch's
rows.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED0 = 9100
LAUNCHES = [[7, 3]] * 5          # 5 launches of 7 iterations at stride 3
BURN = 2
MAIN_OPS = ("get_state", "set_state", "seed", "widths_set", "tune_step", "chain")
KNOBS = ("OLPE_UNITS", "OLPE_NO_QUEUE", "OLPE_WPB", "OLPE_RING", "OLPE_OVERLAP",
         "OLPE_WAIT_TICKS")


def spec(case="c32", mode="fast", W=13, env=None, launches=None, accept_min=0, between=None,
         fold=True, hold=False, read_each=False):
    return dict(case=case, mode=mode, W=W, env=env or {}, launches=launches or LAUNCHES,
                burn_in=BURN, accept_min=accept_min, between=between, fold=fold, hold=hold,
                read_each=read_each)


# ---------------------------------------------------------------------------------------
# the child: runs the scenarios of one arm and writes what they left
# ---------------------------------------------------------------------------------------
def _start(sp, seed0=SEED0):
    from olpefit_amd.core import Sampler
    with np.load(os.path.join(REPO, "tests", "golden", sp["case"] + ".npz")) as z:
        image, nsrc, p0 = z["image"], int(z["nsrc"]), np.array(z["p_init"], dtype=np.float64)
    s = Sampler(image, 1.0, 1, 1, 2, nsrc=nsrc)
    s.set_eval_mode(sp["mode"])
    p0[-1] = s.chi_squared(p0)
    W = sp["W"]
    s.seed(seed0 + np.arange(W))
    s.set_state(np.tile(p0, (W, 1)))
    if sp["hold"]:
        s.hold_handoff(True)
    if sp["between"] == "tune_step":
        s.tune_begin()
    return s, p0


def _between(s, sp, p0, i, out):
    op, W = sp["between"], sp["W"]
    if op == "get_state":
        out[f"mid{i}_state"], out[f"mid{i}_tries"], out[f"mid{i}_acc"] = s.get_state()
    elif op == "set_state":
        s.set_state(np.tile(p0, (W, 1)))
    elif op == "seed":
        s.seed(SEED0 + 1000 * (i + 1) + np.arange(W))
    elif op == "widths_set":
        w = s.get_widths() if i == 0 else None
        s.set_widths(None if w is None else w * np.where(np.arange(w.size) % 2, 0.25, 4.0))
    elif op == "tune_step":
        s.tune_step()
    elif op == "chain":
        out[f"mid{i}_chain"] = s.chain()
    elif op == "moments_accumulate":
        s.moments_accumulate()
    elif op == "sync2" and i % 2 == 1:
        s.sync()


def _step(s, sp, p0, i, out):
    it, stride = sp["launches"][i]
    nrec = s.run_async(it, sp["burn_in"], stride, sp["accept_min"])
    if sp["fold"]:
        s.moments_accumulate()
    if sp["read_each"]:
        out[f"chain{i}"] = s.chain() if nrec else np.empty((sp["W"], 0, s.ps))
    if sp["between"] and i + 1 < len(sp["launches"]):
        _between(s, sp, p0, i, out)
    return nrec


def _finish(s, sp, nrec, out):
    n = len(sp["launches"])
    out["overlaps"] = np.int64(s.overlaps())
    out["kernel_ms"] = s.kernel_times(n)
    out["last_units"] = np.int64(s.last_units())
    s.sync()                                   # raises if a hand-off poll timed out
    out["waits"] = np.int64(s.unit_stats()[0])
    out["chain"] = s.chain() if nrec else np.empty((sp["W"], 0, s.ps))
    out["state"], out["tries"], out["acc"] = s.get_state()
    out["mt"], out["gauss"] = s.rng_state()
    out["done_at"] = s.done_at()
    out["moments"] = s.moments_summary()
    if sp["between"] == "tune_step":
        s.tune_end()
    s.close()


def run_scenario(sp):
    out = {}
    s, p0 = _start(sp)
    nrec = 0
    for i in range(len(sp["launches"])):
        nrec = _step(s, sp, p0, i, out)
    _finish(s, sp, nrec, out)
    return out


def run_two_contexts(sp_a, sp_b):
    """two contexts on one device, their launches interleaved"""
    outs = ({}, {})
    (a, pa), (b, pb) = _start(sp_a), _start(sp_b, SEED0 + 500)
    na = nb = 0
    for i in range(len(sp_a["launches"])):
        na = _step(a, sp_a, pa, i, outs[0])
        nb = _step(b, sp_b, pb, i, outs[1])
    _finish(a, sp_a, na, outs[0])
    _finish(b, sp_b, nb, outs[1])
    return outs


def child_main(spec_path, out_path):
    sys.path.insert(0, REPO)
    with open(spec_path) as f:
        job = json.load(f)
    arrays = {}
    if job["kind"] == "two":
        for j, o in enumerate(run_two_contexts(*job["specs"])):
            arrays.update({f"{j}.{k}": v for k, v in o.items()})
    else:
        for j, sp in enumerate(job["specs"]):
            arrays.update({f"{j}.{k}": v for k, v in run_scenario(sp).items()})
    np.savez(out_path, **arrays)


# ---------------------------------------------------------------------------------------
# the parent: both arms, compared bit for bit
# ---------------------------------------------------------------------------------------
def _arm(tmp_path, job, overlap):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(job["specs"][0]["env"])
    env["OLPE_OVERLAP"] = str(overlap)
    sp, out = tmp_path / f"job{overlap}.json", tmp_path / f"out{overlap}.npz"
    sp.write_text(json.dumps(job))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(sp), str(out)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"OLPE_OVERLAP={overlap} child failed:\n{r.stdout}\n{r.stderr}"
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


ARM_OWN = ("overlaps", "kernel_ms", "waits")      # differ between the arms by design


def expected_overlaps(sp):
    """launches after the first overlap unless a main-class call lies before them"""
    n = len(sp["launches"])
    if sp["between"] == "sync2":
        return n - 1 - (n - 1) // 2
    return 0 if sp["between"] in MAIN_OPS or sp["read_each"] else n - 1


def both_arms(tmp_path, specs, kind="each"):
    job = dict(kind=kind, specs=specs)
    off, on = _arm(tmp_path, job, 0), _arm(tmp_path, job, 1)
    assert sorted(off) == sorted(on)
    for k in sorted(on):
        j, name = k.split(".", 1)
        sp = specs[int(j)]
        if name in ARM_OWN:
            continue
        assert on[k].shape == off[k].shape and on[k].dtype == off[k].dtype, k
        assert on[k].tobytes() == off[k].tobytes(), f"{k} differs between the arms ({sp})"
    for j, sp in enumerate(specs):
        n = len(sp["launches"])
        assert int(off[f"{j}.overlaps"]) == 0
        assert int(on[f"{j}.overlaps"]) == expected_overlaps(sp), sp
        for arm in (off, on):
            ms = arm[f"{j}.kernel_ms"]
            assert ms.shape == (n,) and np.all(ms > 0), ms      # n positive times
            assert int(arm[f"{j}.last_units"]) >= 1
            assert int(arm[f"{j}.waits"]) >= 0
            assert arm[f"{j}.moments"][0] > 0                    # rows were folded
    return off, on


@pytest.mark.parametrize("accept_min", [0, 1])
@pytest.mark.parametrize("W", [13, 100, 1001])
def test_launch_shapes(tmp_path, lib_loaded, W, accept_min):
    off, on = both_arms(tmp_path, [spec(W=W, accept_min=accept_min)])
    done = on["0.done_at"]
    total = sum(it for it, _ in LAUNCHES)
    if accept_min == 0:
        assert np.all(done < 0)
    elif W >= 100:
        # some walkers have tried every parameter once before the run's last iteration
        assert np.any((done > 0) & (done < total)), done


@pytest.mark.parametrize("units", [1, 2, 7])
def test_forced_chunking(tmp_path, lib_loaded, units):
    """OLPE_UNITS=7: a launch's chunk 0 waits on the previous launch's chunk 6"""
    off, on = both_arms(tmp_path, [spec(W=100, env={"OLPE_UNITS": str(units)})])
    assert int(on["0.last_units"]) == units == int(off["0.last_units"])


INSTANCES = {
    "2src-32": dict(case="c32"),
    "2src-64-wpb12": dict(case="c64", env={"OLPE_WPB": "12"}),
    "2src-64-wpb16": dict(case="c64", env={"OLPE_WPB": "16"}),
    "3src-64": dict(case="c64_3"),
    "2src-64-exact": dict(case="c64", mode="exact"),
    "3src-64-exact": dict(case="c64_3", mode="exact"),
    "3src-128-ring-13": dict(case="c128_3", W=13),
    "3src-128-ring-7": dict(case="c128_3", W=7),       # fewer than one batch of 12
}


@pytest.mark.parametrize("inst", list(INSTANCES))
def test_sampler_instantiations(tmp_path, lib_loaded, inst):
    both_arms(tmp_path, [spec(**INSTANCES[inst])])


def test_changing_launches(tmp_path, lib_loaded):
    """consecutive launches that differ in iterations and stride (and one without rows)"""
    both_arms(tmp_path, [spec(W=100, launches=[[7, 3], [12, 1], [3, 5], [20, 4], [1, 1], [9, 2]])])


@pytest.mark.parametrize("op", MAIN_OPS + ("moments_accumulate",))
def test_interleaved_calls(tmp_path, lib_loaded, op):
    """a main-class call between launches: today's order, no overlap; the fold alone
    between launches keeps the overlap"""
    both_arms(tmp_path, [spec(W=100, between=op, fold=op != "moments_accumulate")])


def test_chain_order(tmp_path, lib_loaded):
    back_to_back = spec(W=100, launches=[[7, 1], [9, 3]])
    every = spec(W=100, read_each=True)
    off, on = both_arms(tmp_path, [back_to_back, every])
    assert on["0.chain"].shape[1] == 3        # counts 8..16 past burn-in 2 at stride 3: 3 rows
    for i in range(len(LAUNCHES)):
        assert on[f"1.chain{i}"].shape[1] >= 2
    assert on["1.chain4"].tobytes() == on["1.chain"].tobytes()


@pytest.mark.parametrize("inst", ["2src-64-wpb16", "2src-32"])
def test_pairs_that_start_on_an_idle_device(tmp_path, lib_loaded, inst):
    """A launch and its overlapping successor enqueued onto an idle device (after every
    olpe_sync), with more walkers than the device has wave slots: whichever of the two
    the hardware serves first, the successor's persistent grid must not take the device
    before the launch it waits on has a resident wave (the gate of launch_gibbs_t)."""
    both_arms(tmp_path, [spec(W=8192, between="sync2", launches=[[7, 3]] * 6, **INSTANCES[inst])])


def test_two_contexts(tmp_path, lib_loaded):
    both_arms(tmp_path, [spec(case="c32", W=100), spec(case="c64", W=40)], kind="two")


def test_hold_handoff(tmp_path, lib_loaded):
    """the hold hook: hand-offs wait by construction, and the sequence still finishes"""
    off, on = both_arms(tmp_path, [spec(W=100, env={"OLPE_UNITS": "3"}, hold=True)])
    assert int(on["0.waits"]) > 0 and int(off["0.waits"]) > 0


if __name__ == "__main__":
    child_main(sys.argv[1], sys.argv[2])
