"""The acceptance-rate tuner of the proposal widths (olpe_tune_*, Sampler.tune_*) and the
step-2 CLI's --tune-widths / --widths.

The device's log is compared with the NumPy restatement of the rule
(tests/tune_restatement.py) bit for bit, its integer sums with the counters read back
from the device, and the sampler's decisions under the changing widths with the oracle
following the logged schedule.
"""
import json
import os
import re

import numpy as np
import pytest

import tune_restatement as tr
from oracle import olpe_oracle as ora
from olpefit_amd import _lib, step2, synth, tune
from test_gpu_desc_patch import SEED0, _set_env

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sampler(g, mode, W, trace=False):
    from olpefit_amd.core import Sampler
    s = Sampler(g["image"], 1.0, 1, 1, 2, nsrc=int(g["nsrc"]))
    s.set_eval_mode(mode)
    s.seed(SEED0 + np.arange(W))
    s.set_state(np.tile(g["p_init"], (W, 1)))
    s.enable_trace(trace)
    return s


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _sums(s):
    _, t, a = s.get_state()
    return t.astype(np.int64).sum(0), a.astype(np.int64).sum(0)


# -- 7. against the restatement and the oracle ----------------------------------------------
@pytest.mark.parametrize("mode", ["fast", "exact"])
def test_tuner_matches_restatement_and_oracle(golden, lib_loaded, monkeypatch, mode):
    _set_env(monkeypatch, {})
    g = golden("c32")
    W, steps, n_it, target, gain = 6, 6, 240, 0.44, 2.0
    d = tr.defaults(2)
    # synchronised after every call, counters read back in between
    s = _sampler(g, mode, W, trace=True)
    s.tune_begin(target, gain)
    sums = [_sums(s)]
    acc0 = []
    for _ in range(steps):
        s.run(n_it, burn_in=0, record_stride=0)
        acc0.append(s.trace(n_it)[0, :, 5] > 0.5)
        sums.append(_sums(s))
        s.tune_step()
    dT, dA, hw = s.tune_history()
    assert dT.shape == dA.shape == hw.shape == (steps, 16) and dT.dtype == np.int64
    for i in range(steps):
        np.testing.assert_array_equal(dT[i], sums[i + 1][0] - sums[i][0])
        np.testing.assert_array_equal(dA[i], sums[i + 1][1] - sums[i][1])
    assert np.all(dT.sum(1) == W * n_it)
    want = tr.replay(d, dT, dA, target, gain, d)
    assert np.array_equal(_bits(hw), _bits(want))
    assert np.array_equal(_bits(s.get_widths()), _bits(hw[-1]))
    assert not np.array_equal(hw[-1], d) and not np.array_equal(hw[0], hw[-1])
    for i in range(steps):                             # olpefit_amd.tune.update is the same rule
        prev = d if i == 0 else hw[i - 1]
        assert np.array_equal(_bits(tune.update(prev, dT[i], dA[i], i + 1, target, gain, d)),
                              _bits(hw[i]))
    s.tune_end()
    assert np.array_equal(_bits(s.get_widths()), _bits(hw[-1]))       # the widths stay
    final = s.get_state() + s.rng_state()
    s.close()
    # the same sequence queued without a host sync until the end
    s = _sampler(g, mode, W)
    s.tune_begin(target, gain)
    for _ in range(steps):
        s.run_async(n_it)
        s.tune_step()
    dT2, dA2, hw2 = s.tune_history()
    np.testing.assert_array_equal(dT2, dT)
    np.testing.assert_array_equal(dA2, dA)
    assert np.array_equal(_bits(hw2), _bits(hw))
    for x, y in zip(final, s.get_state() + s.rng_state()):
        np.testing.assert_array_equal(x, y)
    assert np.array_equal(_bits(s.get_widths()), _bits(hw[-1]))
    s.close()
    # walker 0 under the logged schedule
    dm, err, _, _ = ora.noise_model(g["image"], 1.0, 1, 1, 2)
    w = ora.Walker(dm, err, g["p_init"], SEED0)
    for i in range(steps):
        w.widths = d if i == 0 else hw[i - 1]
        _, rtr = w.run(n_it, trace=True)
        np.testing.assert_array_equal(acc0[i], np.array([t[4] for t in rtr], dtype=bool),
                                      err_msg=f"step {i}")


# -- 8. edges ------------------------------------------------------------------------------
def test_tuner_edges(golden, lib_loaded, monkeypatch):
    from olpefit_amd.core import OlpeError
    _set_env(monkeypatch, {})
    g = golden("c32")
    d = tr.defaults(2)
    # one walker, and a launch of 3 iterations: at most 3 parameters tried, the others keep
    # their bits
    s = _sampler(g, "fast", 1)
    w0 = d * np.float64(1.234567)
    s.set_widths(w0)
    s.tune_begin(0.44, 2.0)
    s.run_async(3)
    s.tune_step()
    dT, dA, hw = s.tune_history()
    assert dT.sum() == 3 and np.count_nonzero(dT[0]) <= 3
    idle = dT[0] == 0
    assert idle.sum() >= 13 and np.array_equal(_bits(hw[0][idle]), _bits(w0[idle]))
    assert np.array_equal(_bits(hw), _bits(tr.replay(w0, dT, dA, 0.44, 2.0, d)))
    s.tune_end()
    s.close()
    # the upper clamp: target 0.01, stepped from x 32 -- every parameter whose rate is at
    # least 0.03 has f = 1 + 50 (a - 0.01) >= 2 and lands on default x 64 exactly
    s = _sampler(g, "fast", 6)
    s.set_widths(d * 32.0)
    s.tune_begin(0.01, 50.0)
    s.run_async(480)
    s.tune_step()
    dT, dA, hw = s.tune_history()
    assert np.array_equal(_bits(hw), _bits(tr.replay(d * 32.0, dT, dA, 0.01, 50.0, d)))
    high = dA[0] >= 0.03 * dT[0]
    print("upper clamp: rates", np.round(dA[0] / dT[0], 3))
    assert high.any() and np.array_equal(_bits(hw[0][high]), _bits((d * 64.0)[high]))
    assert np.all(hw[0] <= d * 64.0)
    s.tune_end()
    s.close()
    # the lower clamp: from default / 1024 x 1.01, target 0.9, gain 1.  Sampled rates first
    # (whatever they are, the restatement's bits); then counters uploaded so that every
    # rate is 1/2: f = 1 - 0.4 / sqrt(2) = 0.72 at k = 2, below the clamp for every parameter
    s = _sampler(g, "fast", 6)
    w0 = d / 1024.0 * 1.01
    s.set_widths(w0)
    s.tune_begin(0.9, 1.0)
    s.run_async(240)
    s.tune_step()
    st, t, a = s.get_state()
    s.set_state(st, t + 100.0, a + 50.0)               # 6 walkers: dT = 600, dA = 300
    s.set_widths(w0)
    s.tune_step()
    dT, dA, hw = s.tune_history()
    print("lower clamp: sampled rates", np.round(dA[0] / np.maximum(dT[0], 1), 3))
    assert np.array_equal(_bits(hw[0]), _bits(tr.step(w0, dT[0], dA[0], 1, 0.9, 1.0, d)))
    low = (dT[0] > 0) & (dA[0] <= 0.89 * dT[0])
    assert np.array_equal(_bits(hw[0][low]), _bits((d / 1024.0)[low]))
    assert np.all(dT[1] == 600) and np.all(dA[1] == 300)
    assert np.array_equal(_bits(hw[1]), _bits(d / 1024.0))
    assert np.array_equal(_bits(hw[1]), _bits(tr.step(w0, dT[1], dA[1], 2, 0.9, 1.0, d)))
    s.tune_end()
    # out of order, out of domain
    with pytest.raises(OlpeError) as e:
        s.tune_step()
    assert e.value.code == _lib.ESTATE
    with pytest.raises(OlpeError) as e:
        s.tune_end()
    assert e.value.code == _lib.ESTATE
    for target, gain in ((0.5, 2.0), (0.44, 2.3), (0.0, 1.0), (1.0, 0.5), (0.44, 0.0),
                         (0.44, -1.0), (np.nan, 1.0)):
        with pytest.raises(OlpeError) as e:
            s.tune_begin(target, gain)
        assert e.value.code == _lib.EINVAL, (target, gain)
    with pytest.raises(OlpeError) as e:                # the refused begin opened no session
        s.tune_step()
    assert e.value.code == _lib.ESTATE
    s.close()
    from olpefit_amd.core import Sampler
    s = Sampler(g["image"], 1.0, 1, 1, 2, nsrc=2)      # no ensemble yet
    with pytest.raises(OlpeError) as e:
        s.tune_begin(0.44, 2.0)
    assert e.value.code == _lib.ESTATE
    s.close()


# -- 9. sums past the kernel's caps ---------------------------------------------------------
def _const(text, name):
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % re.escape(name), text)
    assert m, name
    return int(m.group(1))


def _caps():
    with open(os.path.join(REPO, "olpefit_amd", "csrc", "olpe_tune.hip")) as f:
        text = f.read()
    assert ("std::min<long long>(((long long)c->W + kThreads - 1) / kThreads, kMaxBlocks)"
            in text)
    assert "w < W; w += step" in text and "(long long)gridDim.x * kThreads" in text
    return _const(text, "kThreads"), _const(text, "kMaxBlocks")


def test_tuner_sums_past_the_caps(golden, lib_loaded, monkeypatch):
    """Counters uploaded through set_state after tune_begin (known integers, no sampling):
    one walker, one below / at / one above the block size, and the smallest count that
    gives a thread a second walker under the grid cap.  The sums are exact -- they pass
    2^32 -- and the widths are the restatement's."""
    from olpefit_amd.core import Sampler
    _set_env(monkeypatch, {})
    T, B = _caps()
    assert T == 256 and T * B <= 1 << 16, (T, B)       # the largest case stays a small ensemble
    g = golden("c32")
    d = tr.defaults(2)
    rs = np.random.RandomState(9)
    s = Sampler(g["image"], 1.0, 1, 1, 2, nsrc=2)
    for W in (1, T - 1, T, T + 1, T * B + 1):
        s.seed(np.arange(W))
        s.set_state(np.tile(g["p_init"], (W, 1)))
        s.tune_begin(0.44, 2.0)
        tries = rs.randint(0, 2 ** 32, size=(W, 16), dtype=np.uint64)
        tries[0] = 2 ** 32 - 1
        acc = (tries * rs.uniform(0.0, 1.0, size=(W, 16))).astype(np.uint64)
        tries[:, 5] = 0                                # an untried parameter
        acc[:, 5] = 0
        s.set_state(np.tile(g["p_init"], (W, 1)), tries.astype(np.float64), acc.astype(np.float64))
        s.tune_step()
        dT, dA, hw = s.tune_history()
        wantT = np.array([int(sum(int(v) for v in tries[:, j])) for j in range(16)])
        wantA = np.array([int(sum(int(v) for v in acc[:, j])) for j in range(16)])
        np.testing.assert_array_equal(dT[0], wantT, err_msg=f"W={W}")
        np.testing.assert_array_equal(dA[0], wantA, err_msg=f"W={W}")
        if W > 1:
            assert dT[0].max() > 2 ** 32
        assert np.array_equal(_bits(hw[0]), _bits(tr.step(d, wantT, wantA, 1, 0.44, 2.0, d)))
        assert hw[0][5] == d[5]
        # counters set back below the baseline: negative deltas, every width kept
        s.set_state(np.tile(g["p_init"], (W, 1)))
        s.tune_step()
        dT, dA, hw = s.tune_history()
        np.testing.assert_array_equal(dT[1], -wantT)
        assert np.array_equal(_bits(hw[1]), _bits(hw[0]))
        s.tune_end()
        s.set_widths(None)
    s.close()


# -- 10. CLI ---------------------------------------------------------------------------------
RUN = ["--walkers", "4", "--seed", "31", "--burn-in", "480", "--iters", "600", "-q"]
TUNE = ["--tune-widths", "480", "--tune-every", "240"]


def _files(out, walkers=4):
    names = [f"{w}_{kind}" for w in range(walkers)
             for kind in ("finalarray_mpi.csv", "acceptance_rate.csv")]
    return {n: open(out + n, "rb").read() for n in names + ["proposal_widths.json"]}


@pytest.fixture(scope="module")
def tuned_run(tmp_path_factory):
    path = synth.write_case(str(tmp_path_factory.mktemp("tuned")), 32, 2)
    return step2.main([path, *RUN, *TUNE, "--checkpoint-every", "1"])


def test_cli_tuning_writes_widths_that_follow_its_history(tuned_run, lib_loaded):
    doc = tune.load_doc(tuned_run + "proposal_widths.json", 2)
    assert doc["source"] == "tuned"
    h = doc["history"]
    dT, dA = np.array(h["dT"]), np.array(h["dA"])
    assert dT.shape == (2, 16) and np.all(dT.sum(1) == 4 * 240)
    d = tr.defaults(2)
    want = tr.replay(d, dT, dA, h["target"], h["gain"], d)
    assert np.array_equal(_bits(np.array(h["widths"])), _bits(want))
    assert np.array_equal(_bits(np.array(doc["widths"])), _bits(want[-1]))
    assert (h["target"], h["gain"]) == (0.44, 2.0)
    got = np.genfromtxt(tuned_run + "0_finalarray_mpi.csv", delimiter=",")
    assert got.shape == (600 - 480 + 2, 17)
    assert not os.path.exists(tuned_run + "step2_checkpoint.npz")


def test_cli_widths_file_equals_widths_through_sampler(tuned_run, tmp_path, lib_loaded):
    """--widths with the tuned file, the same seed and no tuning: the chain files of a run
    that is handed the same widths through Sampler.set_widths."""
    path = synth.write_case(str(tmp_path / "given"), 32, 2)
    out = step2.main([path, *RUN, "--widths", tuned_run + "proposal_widths.json"])
    w = tune.load_widths(tuned_run + "proposal_widths.json", 2)
    doc = tune.load_doc(out + "proposal_widths.json", 2)
    assert doc["source"] == "given" and np.array_equal(_bits(np.array(doc["widths"])), _bits(w))
    from olpefit_amd import fitsio, pipeline
    from olpefit_amd.core import Sampler
    image, hdr = fitsio.getdata_header(path)
    directory, frame, _ = pipeline.image_paths(path)
    p0 = pipeline.initial_parameters(image, pipeline.read_guess(directory + frame + "_initialguess"), 2)
    s = Sampler(image, hdr["ITIME"], hdr["COADDS"], hdr["MULTISAM"], hdr["SAMPMODE"], nsrc=2)
    with np.errstate(all="ignore"):
        p0[-1] = s.chi_squared(p0)
    s.seed(31 + np.arange(4))
    s.set_state(np.tile(p0, (4, 1)))
    s.set_widths(w)
    chain = s.run(600, burn_in=480, record_stride=1)
    s.close()
    for k in range(4):
        got = np.genfromtxt(out + f"{k}_finalarray_mpi.csv", delimiter=",")
        assert np.all(np.isnan(got[0])) and np.array_equal(_bits(got[1:]), _bits(chain[k]))
    # and not the default widths' chains
    path2 = synth.write_case(str(tmp_path / "plain"), 32, 2)
    plain = step2.main([path2, *RUN])
    assert not os.path.exists(plain + "proposal_widths.json")
    assert open(plain + "0_finalarray_mpi.csv", "rb").read() != \
        open(out + "0_finalarray_mpi.csv", "rb").read()


def test_cli_resume_after_tuning(tuned_run, tmp_path, monkeypatch, lib_loaded):
    """Killed after tuning (at the second checkpoint; none is written while tuning) and
    continued with --resume: every file byte-equal to the uninterrupted run's."""
    path = synth.write_case(str(tmp_path / "cut"), 32, 2)
    run = [*RUN, *TUNE, "--checkpoint-every", "1", "--chunk", "40"]
    ref_path = synth.write_case(str(tmp_path / "ref"), 32, 2)
    ref = step2.main([ref_path, *run])
    calls = {"n": 0, "counts": []}
    orig = step2.save_checkpoint

    def dying(path_, shards, out, count, *a, **k):
        calls["n"] += 1
        calls["counts"].append(count)
        if calls["n"] == 2:
            raise KeyboardInterrupt("killed")
        orig(path_, shards, out, count, *a, **k)
    monkeypatch.setattr(step2, "save_checkpoint", dying)
    with pytest.raises(KeyboardInterrupt):
        step2.main([path, *run])
    monkeypatch.setattr(step2, "save_checkpoint", orig)
    assert min(calls["counts"]) > 480                  # no checkpoint during the tuning phase
    with np.load(_ckpt_of(path)) as z:
        assert "widths" in z.files
        cfg = json.loads(str(z["config"]))
        assert cfg["tune"] == [480, 240, 0.44, 2.0] and "widths" not in cfg
    cut = step2.main([path, *run, "--resume"])
    assert _files(cut) == _files(ref)
    # the chunked reference equals the module's unchunked tuned run as well
    assert _files(ref) == _files(tuned_run)


def _ckpt_of(path):
    from olpefit_amd import pipeline
    return step2.checkpoint_path(pipeline.image_paths(path)[2], "2")


def test_step3_widths_out_closes_the_loop(tmp_path, lib_loaded, capsys):
    """apf_step3.py --covariance --widths-out FILE writes covariance.proposal_widths of the
    fold it has just made (source "covariance"); step 2 takes the file through --widths.
    Without --covariance the flag is an argument error."""
    from olpefit_amd import covariance as cv, fitsio, step3
    d = tmp_path / "2014_test"
    path = synth.write_case(str(d), 32, 2)
    img, _ = synth.make_image(32, 2, 0)
    fitsio.write(path, img, {**synth.HEADER, "KOAID": "N2.20250127.00001.fits", "PARANG": 12.5,
                             "ROTPPOSN": 100.25, "INSTANGL": 0.7, "EL": 55.0, "AZ": 200.0,
                             "ROTMODE": "position angle", "PARANTEL": -20.0, "ITIME": 1.0,
                             "COADDS": 1, "MULTISAM": 1, "SAMPMODE": 2})
    out = step2.main([path, "--walkers", "8", "--seed", "3", "--iters", "420", "--burn-in", "20",
                      "-q"])
    wfile = str(tmp_path / "from_step3.json")
    with pytest.raises(SystemExit):
        step3.main([path, "sys", "-s", "8", "-q", "--widths-out", wfile])
    capsys.readouterr()
    step3.main([path, "sys", "-s", "8", "-q", "--covariance", "--widths-out", wfile])
    doc = tune.load_doc(wfile, 2)
    assert doc["source"] == "covariance" and "history" not in doc
    st = cv.load_npz(out + "00001_covariance.npz")
    want = cv.proposal_widths(st, 2)
    assert np.array_equal(_bits(np.array(doc["widths"])), _bits(want))
    assert not np.array_equal(want, tune.default_widths(2))
    path2 = synth.write_case(str(tmp_path / "next"), 32, 2)
    out2 = step2.main([path2, "--walkers", "2", "--seed", "3", "--iters", "40", "--burn-in", "0",
                       "-q", "--widths", wfile])
    got = tune.load_doc(out2 + "proposal_widths.json", 2)
    assert got["source"] == "given" and got["widths"] == doc["widths"]
