"""olpefit_amd.mapfit through the device's Gauss-Newton sums (Sampler.normal_equations), and
the command lines built on it: apf_map.py, apf_step2.py -i map [--start-scatter S].

The chain files' first data row is the state after iteration 1 (apf_step2.py:342: the count
is incremented before the burn-in check), and an iteration proposes one parameter: a walker
that started at theta has a first row equal to theta in every parameter but at most one --
the form test_cli_gpu uses for -i 2a.
"""
import functools
import json
import os
import shutil

import numpy as np
import pytest

import normal_restatement as nr
from olpefit_amd import mapcli, mapfit, step2, synth, tune
from olpefit_amd.core import Sampler
from olpefit_amd.pipeline import initial_parameters

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRAMES = {"y64": (64, 2), "y64_3": (64, 3), "y33": (33, 2)}


@functools.lru_cache(maxsize=None)
def frame(name):
    n, nsrc = FRAMES[name]
    img, truth = synth.make_image(n, nsrc, 0)
    return img, nsrc, initial_parameters(img, synth.guess_values(n, nsrc), nsrc)[:-1], truth


@pytest.mark.parametrize("name", list(FRAMES))
def test_fit_on_the_device_equals_the_cpu_fit(lib_loaded, name):
    """From the step-1 guess: chi^2 <= chi^2(truth) within 20 accepted steps, and theta_hat
    equal to the fit over the long-double restatement to 1e-8 relative in every free
    parameter."""
    img, nsrc, p0, truth = frame(name)
    with Sampler(img, nsrc=nsrc) as s:
        s.set_eval_mode("exact")
        res = mapfit.fit(s.normal_equations, p0, nsrc)
        chi_truth = s.chi_squared(truth)
    cpu = mapfit.fit(nr.normal(nr.frame(img), nsrc, 0), p0, nsrc)
    print(name, res.history[0], "truth", chi_truth, res.status, res.steps, res.evals)
    assert res.status == ["converged"] and res.steps[0] <= 20
    assert res.chi2[0] <= chi_truth
    free = res.free
    rel = np.abs(res.theta[0, free] - cpu.theta[0, free]) / np.abs(cpu.theta[0, free])
    print(name, "largest relative difference from the CPU fit", rel.max())
    assert rel.max() <= 1e-8
    assert np.array_equal(res.theta[0, ~free], p0[~free])
    assert list(res.steps) == list(cpu.steps)


def test_eight_starts_find_one_minimum(lib_loaded):
    """An 8-start multi_start with scatter 1 (seed 0, the command line's default) finds one
    minimum -- on the 3-source frame.  The frame matters: a scattered start has sigma_x and
    sigma_y of a set nearly equal, theta's column is nearly zero there, and the first step
    turns the set by radians, so the fit ends on any of the copies theta + k pi / 2 (sigmas
    exchanged for odd k).  With three sources these are one model and `canonical` counts them
    as one minimum.  In the 2-source layout with bkgd_mode 0 the wide set's sigma_x is the
    background as well, so its quarter-turn copy is another model: a second, genuinely
    distinct minimum (next test).  The copies differ by 1e-10 in chi^2 at most."""
    img, nsrc, p0, _ = frame("y64_3")
    with Sampler(img, nsrc=nsrc) as s:
        ms = mapfit.multi_start(s.normal_equations, p0, nsrc, starts=8, scatter=1.0, seed=0)
    print("multi-start", ms.status, list(ms.steps), list(ms.evals), list(ms.chi2))
    assert ms.status == ["converged"] * 8 and ms.minima == 1
    assert ms.chi2[-1] - ms.chi2[0] <= 1e-9 * ms.chi2[0]
    assert np.ptp(ms.theta[:, 18]) > 1.0          # the copies were reached, and folded


def test_two_source_mode_0_has_the_quarter_turn_copy_as_a_second_minimum(lib_loaded):
    """The same eight starts on the 2-source frame (bkgd_mode 0): every start converges, to
    the minimum the step-1 guess leads to or to the one with the wide set turned by pi / 2 and
    its sigmas exchanged, whose background (p[12], the wide sigma_x) is the other sigma: two
    distinct minima, 1.79 apart in chi^2 on this frame (3853.965 and 3855.757; on the
    33 x 33 frame the turned one is the lower, 1006.443 against 1006.594).  With
    bkgd_mode 1 the turn is a symmetry again and one minimum is left."""
    img, nsrc, p0, _ = frame("y64")
    with Sampler(img, nsrc=nsrc) as s:
        ms = mapfit.multi_start(s.normal_equations, p0, nsrc, starts=8, scatter=1.0, seed=0)
    with Sampler(img, nsrc=nsrc, bkgd_mode=1) as s:
        m1 = mapfit.multi_start(s.normal_equations, p0, nsrc, starts=8, scatter=1.0, seed=0,
                                bkgd_mode=1)
    print("multi-start, mode 0", list(ms.chi2), "mode 1", list(m1.chi2))
    assert ms.status == ["converged"] * 8 and 1 <= ms.minima <= 2
    c = mapfit.canonical(ms.theta, 2, 0, ms.free)
    main = c[0]
    for row in c:
        same = mapfit.same_minimum(row, main, 2, ms.free)
        turned = (abs(row[12] - main[13]) < 1e-2 and abs(row[13] - main[12]) < 1e-2
                  and abs(abs(row[15] - main[15]) - np.pi / 2) < 1e-2)
        assert same or turned, row
    assert m1.status == ["converged"] * 8 and m1.minima == 1


def rows(out, w):
    a = np.genfromtxt(out + f"{w}_finalarray_mpi.csv", delimiter=",")
    assert np.all(np.isnan(a[0]))
    return a[1:]


def started_at(first_row, theta):
    return np.count_nonzero(first_row[:len(theta)] != theta) <= 1


def test_command_lines(lib_loaded, tmp_path):
    """apf_map.py on a 64 x 64 frame, then apf_step2.py -i map: every walker starts at
    theta_hat; with --start-scatter 1 walker w starts at laplace_draws(...)[w], two 2-walker
    runs (seeds 1, 2 and 3, 4) give the 4-walker run's chains (seeds 1 .. 4), and a run whose
    background mode differs from the file's is refused."""
    path = synth.write_case(str(tmp_path / "a"), 64, 2)
    out = mapcli.main([path, "-q"])
    with open(out + "map_fit.json") as f:
        doc = json.load(f)
    img, nsrc, p0, truth = frame("y64")
    with Sampler(img, nsrc=2) as s:
        res = mapfit.fit(s.normal_equations, p0, 2)
        chi_truth = s.chi_squared(truth)
    theta = np.array(doc["theta_hat"])
    assert np.array_equal(theta, mapfit.canonical(res.theta[0], 2, 0, res.free))
    assert doc["status"] == "converged" and doc["chi2"] <= chi_truth
    assert doc["nsrc"] == 2 and doc["side"] == 64 and doc["bkgd_mode"] == 0
    assert doc["free"] == [k != 9 for k in range(16)] and not any(doc["flat"])
    wdoc = tune.load_doc(out + "map_widths.json", 2)
    assert wdoc["source"] == "laplace"
    fit = mapfit.load_map(out + "map_fit.json", 2, 0, 64)
    assert np.array_equal(wdoc["widths"],
                          mapfit.proposal_widths(fit["F"], theta, 2, fit["free"]))
    sig = np.array(doc["sigma"])
    assert np.all(np.abs(theta - truth)[fit["free"]] <= 5 * sig[fit["free"]])

    common = ["-i", "map", "--iters", "20", "--burn-in", "0", "-q"]
    step2.main([path, *common, "--walkers", "4", "--seed", "1"])
    for w in range(4):
        r = rows(out, w)
        assert r.shape == (20, 17) and started_at(r[0], theta), w
    # every walker at its own draw
    step2.main([path, *common, "--walkers", "4", "--seed", "1", "--start-scatter", "1"])
    draws = mapfit.laplace_draws(fit, [1, 2, 3, 4], 1.0)
    whole = [rows(out, w) for w in range(4)]
    for w in range(4):
        assert started_at(whole[w][0], draws[w]), w
        assert not started_at(whole[w][0], theta)
    assert len({tuple(r[0]) for r in whole}) == 4
    for k, seed in enumerate((1, 3)):
        sub = tmp_path / f"s{k}"
        p2 = synth.write_case(str(sub), 64, 2)
        o2 = step2.pipeline.image_paths(p2)[2]
        os.makedirs(o2, exist_ok=True)
        shutil.copy(out + "map_fit.json", o2 + "map_fit.json")
        step2.main([p2, *common, "--walkers", "2", "--seed", str(seed), "--start-scatter", "1"])
        for w in range(2):
            assert np.array_equal(rows(o2, w), whole[2 * k + w]), (k, w)
    # the file's layout, background mode and side are checked
    with pytest.raises(ValueError):
        step2.main([path, *common, "--walkers", "2", "--seed", "1", "--fixed-bkgd"])
    with pytest.raises(SystemExit):
        step2.main([path, "--iters", "20", "--walkers", "2", "--start-scatter", "1", "-q"])


def test_three_source_command_lines(lib_loaded, tmp_path):
    path = synth.write_case(str(tmp_path), 64, 3)
    out = mapcli.main([path, "-q", "--starts", "3"], nsrc=3)
    fit = mapfit.load_map(out + "map_fit.json", 3, 0, 64)
    assert fit["status"] == "converged" and fit["minima"] == 1 and fit["free"].all()
    step2.main([path, "-i", "map", "--iters", "20", "--walkers", "2", "--seed", "5", "-q"], nsrc=3)
    for w in range(2):
        assert started_at(rows(out, w)[0], fit["theta_hat"])


def test_step_1_start_is_what_the_parent_commit_wrote(lib_loaded, tmp_path):
    """Without the new flags step 2 writes what it wrote before them: -i 1 --iters 20
    --walkers 4 --seed 1 --burn-in 0 on synth.write_case(..., 64) against the files the
    parent commit's sources wrote for the same command (tests/golden/map_cli_parent)."""
    path = synth.write_case(str(tmp_path), 64, 2)
    out = step2.main([path, "-i", "1", "--iters", "20", "--burn-in", "0", "--walkers", "4",
                      "--seed", "1", "-q"])
    for w in range(4):
        for name in (f"{w}_finalarray_mpi.csv", f"{w}_acceptance_rate.csv"):
            with open(out + name, "rb") as f, \
                    open(os.path.join(GOLDEN, "map_cli_parent", name), "rb") as g:
                assert f.read() == g.read(), name


def test_resume_of_a_map_start(lib_loaded, tmp_path, monkeypatch):
    """A run from -i map --start-scatter 1 killed before its third checkpoint resumes to the
    uninterrupted run's files; --resume with another S, or against a map_fit.json that holds
    another best fit, is refused."""
    ref_path = synth.write_case(str(tmp_path / "ref"), 64, 2)
    cut_path = synth.write_case(str(tmp_path / "cut"), 64, 2)
    out = mapcli.main([ref_path, "-q"])
    cut = step2.pipeline.image_paths(cut_path)[2]
    os.makedirs(cut, exist_ok=True)
    shutil.copy(out + "map_fit.json", cut + "map_fit.json")
    run = ["-i", "map", "--walkers", "3", "--seed", "21", "--burn-in", "10", "--chunk", "40",
           "--iters", "205", "--checkpoint-every", "1", "-q"]
    ref = step2.main([ref_path, *run, "--start-scatter", "1"])
    calls = {"n": 0}
    orig = step2.save_checkpoint

    def dying(*a, **k):
        calls["n"] += 1
        if calls["n"] == 3:
            raise KeyboardInterrupt("killed")
        orig(*a, **k)
    monkeypatch.setattr(step2, "save_checkpoint", dying)
    with pytest.raises(KeyboardInterrupt):
        step2.main([cut_path, *run, "--start-scatter", "1"])
    monkeypatch.setattr(step2, "save_checkpoint", orig)
    with pytest.raises(ValueError, match="other settings"):
        step2.main([cut_path, *run, "--start-scatter", "2", "--resume"])
    with pytest.raises(ValueError, match="other settings"):
        step2.main([cut_path, *run, "--resume"])
    with open(cut + "map_fit.json") as f:
        doc = json.load(f)
    good = json.dumps(doc)
    doc["theta_hat"][0] += 1e-9
    with open(cut + "map_fit.json", "w") as f:
        json.dump(doc, f)
    with pytest.raises(ValueError, match="another best fit"):
        step2.main([cut_path, *run, "--start-scatter", "1", "--resume"])
    with open(cut + "map_fit.json", "w") as f:
        f.write(good)
    step2.main([cut_path, *run, "--start-scatter", "1", "--resume"])
    for w in range(3):
        for name in (f"{w}_finalarray_mpi.csv", f"{w}_acceptance_rate.csv"):
            with open(ref + name, "rb") as f, open(cut + name, "rb") as h:
                assert f.read() == h.read(), name
