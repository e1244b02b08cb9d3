"""Autocorrelation lag sums on the device (olpe_acf.hip, olpefit_amd/autocorr.py) against the
NumPy restatement in np.longdouble (tests/acf_restatement.py).

Bound.  Per lag, |C[k] - ref[k]| <= 4 (W N) 2^-53 ref[0]: the worst-case bound of recursive
summation of W N terms, which any summation order meets; the sum of the terms' magnitudes
is at most C[0] by Cauchy-Schwarz, and the factor 4 covers the roundings of the products, of
the deviations and of the mean.  Each comparison prints its largest ratio to that bound.
Where the same operations run on the same values (a repeated fold, the device chain against
its read-back) the comparison is np.array_equal.

Shapes (W, N, ncols, L): a two-row series, fewer rows than a tile, N < L (lags >= N are
exactly 0.0), more series than fit a slot, 24 and 20 columns (three and two column groups),
several time tiles with a ragged last one, and both lag passes of L = 1024.  Those stay
under 1024 units, one a workgroup; the shapes of tests/fold_scale_cases.py give a workgroup
two or five.
"""
import functools
import json
import os

import numpy as np
import pytest

import acf_restatement as ar
import fold_scale_cases as fc
from olpefit_amd import _lib, autocorr, step2, step3, synth
from olpefit_amd.autocorr import Autocorr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SHAPES = [(1, 2, 17, 64), (3, 63, 17, 64), (2, 40, 17, 128), (257, 65, 24, 64),
          (48, 257, 20, 128), (5, 773, 17, 256), (4, 1100, 17, 1024)]
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def case(W, N, ncols, L):
    """The rows [W][N][ncols] of a shape and their restated lag sums, computed once."""
    rows = ar.chain_like(W, N, ncols, 100 * W + N)
    rows.setflags(write=False)
    ref = ar.lag_sums(rows, L)
    ref["C"].setflags(write=False)
    return rows, ref


def ratio(C, ref, terms):
    """max over columns and lags of |C - ref| / (4 terms 2^-53 ref[0])."""
    refC = ref["C"] if isinstance(ref, dict) else ref
    dev = np.abs(np.asarray(C, dtype=np.longdouble) - refC)
    return float((dev / (4.0 * terms * U * refC[:, :1])).max())


def check(state, ref, terms, label=""):
    r = ratio(state["C"], ref, terms)
    print(f"{label} max |C - ref| / bound = {r:.3e}")
    assert r <= 1.0, (label, r)
    return r


@pytest.mark.parametrize("time_major", [False, True])
@pytest.mark.parametrize("W, N, ncols, L", SHAPES)
def test_lag_sums_equal_the_restatement(lib_loaded, W, N, ncols, L, time_major):
    rows, ref = case(W, N, ncols, L)
    data = np.ascontiguousarray(np.swapaxes(rows, 0, 1)) if time_major else rows
    with Autocorr(ncols, L) as a:
        a.fold_rows(data, time_major=time_major)
        st = a.state()
    assert (st["n"], st["series"], st["skipped"]) == (W * N, W, 0)
    assert st["C"].shape == (ncols, L + 1)
    check(st, ref, W * N, f"{(W, N, ncols, L)} time_major={time_major}")
    if N <= L:
        assert np.all(st["C"][:, N:] == 0.0)            # exactly, not to rounding
    assert np.all(st["C"][:, 0] > 0.0)


@pytest.mark.parametrize("tile", ["64", "128", None])
@pytest.mark.parametrize("W, N, ncols, L", [(5, 773, 17, 256), (257, 65, 24, 64)])
def test_tile_edges(lib_loaded, monkeypatch, W, N, ncols, L, tile):
    """OLPE_ACF_TILE sets the time tile's rows: 773 rows are 13 tiles of 64 with 5 rows in
    the last, 7 of 128, or the default's; 65 rows leave one row for a second tile of 64."""
    if tile is None:
        monkeypatch.delenv("OLPE_ACF_TILE", raising=False)
    else:
        monkeypatch.setenv("OLPE_ACF_TILE", tile)
    rows, ref = case(W, N, ncols, L)
    with Autocorr(ncols, L) as a:
        a.fold_rows(rows)
        st = a.state()
    assert (st["n"], st["series"], st["skipped"]) == (W * N, W, 0)
    check(st, ref, W * N, f"{(W, N, ncols, L)} tile {tile}")


def test_same_fold_same_bits(lib_loaded):
    rows, _ = case(48, 257, 20, 128)
    out = []
    for _ in range(2):
        with Autocorr(20, 128) as a:
            a.fold_rows(rows)
            out.append(a.state())
    assert np.array_equal(out[0]["C"], out[1]["C"]) and out[0]["n"] == out[1]["n"]


def test_non_finite_series_are_left_out_whole(lib_loaded):
    rows, _ = case(48, 257, 20, 128)
    bad = rows.copy()
    bad[7, 100, 3] = np.nan
    bad[31, 0, 19] = np.inf
    keep = [w for w in range(48) if w not in (7, 31)]
    ref = ar.lag_sums(rows[keep], 128)
    for tm in (False, True):
        data = np.ascontiguousarray(np.swapaxes(bad, 0, 1)) if tm else bad
        with Autocorr(20, 128) as a:
            a.fold_rows(data, time_major=tm)
            st = a.state()
        assert (st["skipped"], st["series"], st["n"]) == (2, 46, 46 * 257)
        assert np.isfinite(st["C"]).all()
        check(st, ref, 46 * 257, f"non-finite, time_major={tm}")
    assert ar.lag_sums(bad, 128)["skipped"] == 2


def test_state_is_additive(lib_loaded):
    """20 + 28 walkers over two objects merged by add, and over two fold_rows calls of one
    object: the counters are exact and C is within the bound of one fold's reference."""
    rows, ref = case(48, 257, 20, 128)
    with Autocorr(20, 128) as a, Autocorr(20, 128) as b, Autocorr(20, 128) as c, \
            Autocorr(20, 64) as other:
        a.fold_rows(rows[:20])
        b.fold_rows(rows[20:])
        sa = a.state()
        assert (sa["n"], sa["series"]) == (20 * 257, 20)
        a.add(b.state())
        c.fold_rows(rows[:20])
        c.fold_rows(rows[20:])
        for name, st in (("add", a.state()), ("two folds", c.state())):
            assert (st["n"], st["series"], st["skipped"]) == (48 * 257, 48, 0)
            check(st, ref, 48 * 257, name)
        with pytest.raises(_lib.OlpeError) as e:
            a.add(other.state())                         # another max_lag
        assert e.value.code == _lib.EINVAL and "max_lag 64" in str(e.value)
        assert a.state()["n"] == 48 * 257
        a.reset()
        st = a.state()
        assert (st["n"], st["series"], st["skipped"]) == (0, 0, 0) and not st["C"].any()


# ---------------------------------------------------------------------------------------
# Several units per workgroup (tests/fold_scale_cases.py; test_fold_plans_cpu.py asserts the
# plans).  Above 1024 (series, time tile) units a workgroup of acf_fold_kernel walks a run of
# them, re-staging its LDS per unit with the accumulators kept, and skips the units of an
# unusable series ahead of its barrier.

def knob(monkeypatch, tile):
    if tile is None:
        monkeypatch.delenv("OLPE_ACF_TILE", raising=False)
    else:
        monkeypatch.setenv("OLPE_ACF_TILE", tile)


@pytest.mark.parametrize("time_major", [False, True])
@pytest.mark.parametrize("name", list(fc.ACF))
def test_several_units_per_workgroup(lib_loaded, monkeypatch, name, time_major):
    """The shapes of fold_scale_cases.ACF: 2 or 5 units a workgroup, a last workgroup of one
    unit, the two-pass kernel, workgroups whose units are of two series."""
    W, N, ncols, L, tile = fc.ACF[name]
    knob(monkeypatch, tile)
    rows, ref = case(W, N, ncols, L)
    data = np.ascontiguousarray(np.swapaxes(rows, 0, 1)) if time_major else rows
    with Autocorr(ncols, L) as a:
        a.fold_rows(data, time_major=time_major)
        st = a.state()
    assert (st["n"], st["series"], st["skipped"]) == (W * N, W, 0)
    check(st, ref, W * N, f"{name} {(W, N, ncols, L)} tile {tile} time_major={time_major}")
    if N <= L:
        assert np.all(st["C"][:, N:] == 0.0)
    assert np.all(st["C"][:, 0] > 0.0)


def test_unused_units_inside_a_run(lib_loaded, monkeypatch):
    """1100 series x 200 rows in tiles of 64: 4 units a series, 5 a workgroup.  Series 10, 11
    and 21 hold a non-finite value: workgroup 8 (units 40 .. 44) has no used unit and must
    leave zeros, not stale memory, in its partial sums; workgroup 9 begins with three unused
    units and ends with two used ones; workgroup 16 ends with an unused unit.  Twice the same
    bits; and the state equals the add of two half folds (other runs of units, so another
    order of the same terms) within twice the bound."""
    W, N, ncols, L, tile = fc.ACF_SKIP
    knob(monkeypatch, tile)
    rows, _ = case(W, N, ncols, L)
    bad = rows.copy()
    for k, s in enumerate(fc.ACF_BAD_SERIES):
        bad[s, (0, N - 1, 77)[k], (3, 16, 9)[k]] = (np.nan, np.inf, -np.inf)[k]
    ref = ar.lag_sums(bad, L)
    assert (ref["skipped"], ref["series"], ref["n"]) == (3, W - 3, (W - 3) * N)
    out = []
    for tm in (False, False, True):
        data = np.ascontiguousarray(np.swapaxes(bad, 0, 1)) if tm else bad
        with Autocorr(ncols, L) as a:
            # a fold of every series first, so that the partial sums of every workgroup hold
            # numbers when the fold under test begins
            a.fold_rows(rows)
            a.reset()
            a.fold_rows(data, time_major=tm)
            st = a.state()
        assert (st["n"], st["series"], st["skipped"]) == (ref["n"], ref["series"], ref["skipped"])
        assert np.isfinite(st["C"]).all()
        check(st, ref, ref["n"], f"unused units, time_major={tm}")
        out.append(st)
    assert np.array_equal(out[0]["C"], out[1]["C"])
    with Autocorr(ncols, L) as a, Autocorr(ncols, L) as b:
        a.fold_rows(bad[:W // 2])
        b.fold_rows(bad[W // 2:])
        a.add(b.state())
        halves = a.state()
    assert (halves["n"], halves["series"], halves["skipped"]) == \
        (ref["n"], ref["series"], ref["skipped"])
    check(halves, ref, ref["n"], "two half folds added")
    dev = np.abs(out[0]["C"].astype(np.longdouble) - halves["C"].astype(np.longdouble))
    r = float((dev / (4.0 * ref["n"] * U * ref["C"][:, :1])).max())
    print(f"one fold against two half folds: max |dC| / bound = {r:.3e}")
    assert r <= 2.0


def test_sampler_device_chain(lib_loaded):
    """fold(sampler) reads a launch's device chain [W][nrec][PS] in place; fold_rows of the
    chain read back runs the same kernels on the same values in the same layout: the same
    bits.  Once per launch, the right PS, and a second launch adds its series."""
    from olpefit_amd.core import Sampler
    with np.load(os.path.join(GOLDEN, "c64.npz"), allow_pickle=False) as z:
        img, nsrc, p0 = z["image"], int(z["nsrc"]), z["p_init"].copy()
    W = 48
    with Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc) as s, Autocorr(s.ps, 128) as dev, \
            Autocorr(s.ps, 128) as host, Autocorr(s.ps + 1, 128) as wrong:
        p0[-1] = s.chi_squared(p0)
        s.seed(np.arange(1, W + 1))
        s.set_state(np.tile(p0, (W, 1)))
        with pytest.raises(_lib.OlpeError) as e:
            dev.fold(s)                                  # nothing launched yet
        assert e.value.code == _lib.ESTATE
        assert s.run_async(300, 0, 1) == 300
        dev.fold(s)                                      # behind the launch, no sync
        s.sync()
        chain = s.chain()
        assert chain.shape == (W, 300, s.ps)
        host.fold_rows(chain)
        a, b = dev.state(), host.state()
        assert (a["n"], a["series"], a["skipped"]) == (b["n"], b["series"], b["skipped"]) \
            == (W * 300, W, 0)
        ref = ar.lag_sums(chain, 128)
        moving = ref["C"][:, 0] > 0                       # a column may never have moved
        assert moving.sum() >= 10
        r = ratio(a["C"][moving], ref["C"][moving], W * 300)
        print(f"device chain max |C - ref| / bound = {r:.3e}")
        assert r <= 1.0
        assert np.array_equal(a["C"], b["C"])
        with pytest.raises(_lib.OlpeError) as e:
            dev.fold(s)                                  # the same launch twice
        assert e.value.code == _lib.ESTATE and "already folded" in str(e.value)
        with pytest.raises(_lib.OlpeError) as e:
            wrong.fold(s)                                # another PS
        assert e.value.code == _lib.EINVAL and "PS" in str(e.value)
        s.run_async(300, 0, 1)
        dev.fold(s)
        st = dev.state()
        assert (st["series"], st["n"]) == (96, 96 * 300)
        res = dev.result()
        assert res["record_stride"] == 1
        assert np.array_equal(res["tau_iterations"], res["tau"], equal_nan=True)


def test_end_to_end_tau(lib_loaded):
    """The CPU test's AR(1) case (64 x 2,000, phi = 0.5 and white noise, L = 512): the
    device's window equals the restatement's, tau agrees to 1e-9, and the chains are long
    enough; phi = 0.97 over 773 rows is not (tau = 66, 50 tau > 773)."""
    rows = ar.ar1([0.5, 0.0], 64, 2000, 4)
    ref = ar.lag_sums(rows, 512)
    with Autocorr(2, 512, labels=["ar", "white"]) as a:
        a.fold_rows(rows)
        res = a.result()
    for k in range(2):
        tau, m, windowed, reliable, ess = ar.integrated_time(ref["C"][k], ref["n"], 64)
        print(res["labels"][k], "tau", res["tau"][k], "restated", tau, "window", m)
        assert res["window"][k] == m and res["windowed"][k] == windowed
        assert abs(res["tau"][k] - tau) <= 1e-9 * tau
        assert res["reliable"][k] and reliable
        assert abs(res["ess"][k] - ess) <= 1e-9 * ess
    assert res["min_ess"] == res["ess"].min() and res["tau_iterations"] is None
    rows, _ = case(5, 773, 17, 256)                      # column 16: phi = 0.97
    with Autocorr(17, 256) as a:
        a.fold_rows(rows)
        res = a.result()
    assert not res["reliable"][16]
    assert res["reliable"][0]                            # white noise: 773 >= 50 x 1


def test_cli_autocorr(tmp_path, lib_loaded, capsys):
    """apf_step3.py --autocorr on a small step-2 output (8 walkers x 400 rows): the .npz and
    the summary's "autocorr" key are written, the printed tau is Autocorr's from Python;
    without the flag the summary has no such key and is otherwise the same."""
    d = tmp_path / "2014_test"
    path = synth.write_case(str(d), 32, 2)
    out = step2.main([path, "--walkers", "8", "--seed", "3", "--iters", "420", "--burn-in", "20",
                      "-q"])
    plain = step3.main([path, "sys", "-s", "8", "-q"])
    with open(out + "step3_summary.json", "rb") as f:
        before = f.read()
    assert "autocorr" not in plain and before == json.dumps(plain, indent=1).encode()
    assert not os.path.exists(out + "00001_autocorr.npz")
    capsys.readouterr()
    got = step3.main([path, "sys", "-s", "8", "--autocorr", "--autocorr-max-lag", "128"])
    text = capsys.readouterr().out
    chains = step3.load_chains(out, 8, 1)                # [N][8][17], the seed row dropped
    assert chains.shape[0] >= 399 and chains.shape[1:] == (8, 17)
    with Autocorr(17, 128, labels=step3.NAMES_2) as a:
        a.fold_rows(chains, time_major=True)
        st, res = a.state(), a.result()
    assert (st["n"], st["series"], st["skipped"]) == (chains.shape[0] * 8, 8, 0)
    lines = autocorr.table_lines(res)
    assert len(lines) == 17
    for line in lines:
        assert line in text
    assert "Smallest effective sample size: " + str(res["min_ess"]) in text
    z = autocorr.load_npz(out + "00001_autocorr.npz")
    assert z["labels"].tolist() == step3.NAMES_2 and int(z["max_lag"]) == 128
    assert np.array_equal(z["C"], st["C"]) and int(z["n"]) == st["n"]
    assert np.array_equal(z["tau"], res["tau"], equal_nan=True)
    assert np.array_equal(z["window"], res["window"])
    with open(out + "step3_summary.json") as f:
        saved = json.load(f)
    cols = saved["autocorr"]["columns"]
    assert list(cols) == step3.NAMES_2 and saved["autocorr"]["series"] == 8
    for k, name in enumerate(step3.NAMES_2):
        t = res["tau"][k]
        assert cols[name]["tau"] == (float(t) if np.isfinite(t) else None)
        assert cols[name]["window"] == int(res["window"][k])
    assert got["autocorr"]["file"] == out + "00001_autocorr.npz"
    assert {k: v for k, v in saved.items() if k != "autocorr"} == json.loads(before)
