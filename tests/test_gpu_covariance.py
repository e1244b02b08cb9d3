"""Cross-column sums on the device (olpe_cov.hip, olpefit_amd/covariance.py) against the
NumPy restatement in np.longdouble (tests/cov_restatement.py).

Bounds, with u = 2^-53 and n the rows folded:
    |S2[j][k] - ref| <= 4 n u sqrt(ref[j][j] ref[k][k])
    |S1[j]    - ref| <= 4 n u sqrt(n ref[j][j])
and per walker likewise with that walker's count and its own sum of squares.  They are the
worst-case bound of recursive summation of n terms, which any summation order meets; the sum
of the terms' magnitudes is bounded by Cauchy-Schwarz, and the factor 4 covers the roundings
of the differences and of the products.  Each comparison prints its largest ratio to the
bound.  Where the same operations run on the same values (a repeated fold, the device chain
against its read-back) the comparison is np.array_equal.

Shapes (W, N, ncols): one row; fewer rows than any tile; one under and one over 64 rows; one
16-column block exactly; one and two columns; 24 columns with a ragged last tile; many walkers
of few rows.  Those stay under 2048 tiles, one a workgroup; the shapes of
tests/fold_scale_cases.py give a workgroup two or three (the second half of this file).
"""
import functools
import json
import os

import numpy as np
import pytest

import acf_restatement as ar
import cov_restatement as cr
import fold_scale_cases as fc
from olpefit_amd import _lib, covariance as cv, fitsio, step2, step3, synth
from olpefit_amd.covariance import Covariance

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SHAPES = [(1, 1, 17), (1, 3, 17), (3, 63, 17), (2, 65, 20), (4, 64, 16), (7, 130, 1),
          (3, 40, 2), (5, 257, 24), (257, 5, 17)]
POOLED = [(3, 63, 17), (5, 257, 24), (257, 5, 17)]
RAGGED = [(3, 63, 17), (2, 65, 20), (5, 257, 24), (257, 5, 17)]
U = 2.0 ** -53
LD = np.longdouble


@functools.lru_cache(maxsize=None)
def case(W, N, ncols):
    """The rows [W][N][ncols] of a shape and their restated sums (automatic pivot), once."""
    rows = ar.chain_like(W, N, ncols, 100 * W + N)
    rows.setflags(write=False)
    return rows, cr.sums(rows)


def worst(dev, bound):
    """max |dev| / bound, a zero bound demanding a zero deviation."""
    dev, bound = np.abs(np.asarray(dev, dtype=LD)), np.asarray(bound, dtype=LD)
    r = np.where(dev == 0, LD(0), dev / np.where(bound > 0, bound, LD(1)))
    r = np.where((bound == 0) & (dev > 0), LD(np.inf), r)
    return float(r.max()) if r.size else 0.0


def check(st, ref, label="", diag=None):
    """The pooled sums, and the walkers' where the state has them, against the restatement;
    ``diag`` replaces the reference's S2 diagonal in the bounds."""
    n = ref["n"]
    d = np.diag(ref["S2"]) if diag is None else np.asarray(diag, dtype=LD)
    r2 = worst(st["S2"] - ref["S2"], 4 * n * U * np.sqrt(np.outer(d, d)))
    r1 = worst(st["S1"] - ref["S1"], 4 * n * U * np.sqrt(n * d))
    print(f"{label} max |S2 - ref| / bound = {r2:.3e}, |S1 - ref| / bound = {r1:.3e}")
    assert r2 <= 1.0 and r1 <= 1.0, (label, r2, r1)
    assert (st["n"], st["skipped"]) == (ref["n"], ref["skipped"]), label
    assert np.array_equal(st["S2"], st["S2"].T), label
    if st["walkers"]:
        nw = ref["nw"].astype(LD)[:, None]
        rw = worst(st["S1w"] - ref["S1w"], 4 * nw * U * np.sqrt(nw * ref["S2w"]))
        print(f"{label} max |S1w - ref| / bound = {rw:.3e}")
        assert rw <= 1.0, (label, rw)
        assert np.array_equal(st["nw"], ref["nw"]), label


def lay(rows, time_major):
    return np.ascontiguousarray(np.swapaxes(rows, 0, 1)) if time_major else rows


@pytest.mark.parametrize("time_major", [False, True])
@pytest.mark.parametrize("W, N, ncols", SHAPES)
def test_sums_equal_the_restatement(lib_loaded, W, N, ncols, time_major):
    rows, ref = case(W, N, ncols)
    with Covariance(ncols, walkers=W) as c:
        c.fold_rows(lay(rows, time_major), time_major=time_major)
        st, bt = c.state(), c.between()
    assert st["has_pivot"] and np.array_equal(st["pivot"], rows[0, 0])
    check(st, ref, f"{(W, N, ncols)} time_major={time_major}")
    assert (bt["m"], bt["nw_min"], bt["nw_max"]) == (W, N, N)
    # the between term: W terms S1w_j S1w_k / nw, each within the S1w bounds of its reference
    d = np.sqrt(N * ref["S2w"])                                  # >= |S1w| by Cauchy-Schwarz
    bound = (8 * N + 4 * W) * U * (d[:, :, None] * d[:, None, :]).sum(axis=0) / N
    rb = worst(bt["B"] - ref["between"], bound)
    print(f"{(W, N, ncols)} max |B - ref| / bound = {rb:.3e}")
    assert rb <= 1.0 and np.array_equal(bt["B"], bt["B"].T)


@pytest.mark.parametrize("time_major", [False, True])
@pytest.mark.parametrize("W, N, ncols", POOLED)
def test_pooled_only(lib_loaded, W, N, ncols, time_major):
    """walkers = 0: the first two dimensions are just rows; no per-walker state."""
    rows, ref = case(W, N, ncols)
    with Covariance(ncols) as c:
        c.fold_rows(lay(rows, time_major), time_major=time_major)
        st = c.state()
        with pytest.raises(_lib.OlpeError) as e:
            c.between()
        assert e.value.code == _lib.ESTATE
    assert "nw" not in st and st["walkers"] == 0
    check(st, ref, f"{(W, N, ncols)} pooled time_major={time_major}")


@pytest.mark.parametrize("tile", ["64", "128"])
@pytest.mark.parametrize("W, N, ncols", RAGGED)
def test_tile_edges(lib_loaded, monkeypatch, W, N, ncols, tile):
    """OLPE_COV_TILE sets the tile's rows (256 by default, above): 257 rows are 5 tiles of 64
    with one row in the last, or 3 of 128; 63 and 65 rows sit either side of a 64-row tile."""
    monkeypatch.setenv("OLPE_COV_TILE", tile)
    rows, ref = case(W, N, ncols)
    with Covariance(ncols, walkers=W) as c:
        c.fold_rows(rows)
        check(c.state(), ref, f"{(W, N, ncols)} tile {tile}")


def test_same_fold_same_bits(lib_loaded):
    rows, _ = case(5, 257, 24)
    out = []
    for _ in range(2):
        with Covariance(24, walkers=5) as c:
            c.fold_rows(rows)
            out.append((c.state(), c.between()))
    for k in ("S1", "S2", "S1w", "nw", "pivot"):
        assert np.array_equal(out[0][0][k], out[1][0][k]), k
    assert out[0][0]["n"] == out[1][0]["n"] and np.array_equal(out[0][1]["B"], out[1][1]["B"])


def test_non_finite_rows_are_left_out_whole(lib_loaded):
    rows, _ = case(5, 257, 24)
    bad = rows.copy()
    bad[2, 128, 7] = np.nan                      # the middle of a walker
    bad[3, 0, 23] = np.inf                       # row 0 of another
    bad[0, 0, 4] = np.nan                        # the automatic pivot's row
    ref = cr.sums(bad)
    assert ref["skipped"] == 3 and ref["pivot"][4] == 0.0
    for tm in (False, True):
        with Covariance(24, walkers=5) as c:
            c.fold_rows(lay(bad, tm), time_major=tm)
            st, res = c.state(), c.result()
        assert st["pivot"][4] == 0.0 and np.array_equal(st["pivot"], ref["pivot"])
        assert st["skipped"] == 3 and st["n"] == 5 * 257 - 3
        assert st["nw"].tolist() == [256, 257, 256, 256, 257]
        for k in ("S1", "S2", "S1w"):
            assert np.isfinite(st[k]).all(), k
        check(st, ref, f"non-finite, time_major={tm}")
        assert res["mpsrf"]["mpsrf"] is None
        assert "256" in res["mpsrf"]["note"] and "257" in res["mpsrf"]["note"]


def test_state_is_additive(lib_loaded):
    """Rows 0 .. 99 and 100 .. 256 of every walker over two objects merged by add, and over
    two fold_rows calls of one object, about one pivot: within the bound of one fold's
    reference.  A state of another pivot, ncols or walkers is refused, untouched."""
    rows, _ = case(5, 257, 24)
    p = rows[0, 0].copy()
    ref = cr.sums(rows, p)
    with Covariance(24, 5, pivot=p) as a, Covariance(24, 5, pivot=p) as b, \
            Covariance(24, 5, pivot=p) as c, Covariance(24, 5, pivot=p + 1e-9) as other_p, \
            Covariance(20, 5) as other_c, Covariance(24, 4, pivot=p) as other_w:
        a.fold_rows(rows[:, :100])
        b.fold_rows(rows[:, 100:])
        assert a.state()["n"] == 500
        a.add(b.state())
        c.fold_rows(rows[:, :100])
        c.fold_rows(rows[:, 100:])
        for name, st in (("add", a.state()), ("two folds", c.state())):
            check(st, ref, name)
        before = a.state()
        other_p.fold_rows(rows[:, :100])
        other_c.fold_rows(rows[:, :100, :20])
        other_w.fold_rows(rows[:4, :100])
        for other, word in ((other_p, "pivot"), (other_c, "ncols"), (other_w, "walkers")):
            with pytest.raises(_lib.OlpeError) as e:
                a.add(other.state())
            assert e.value.code == _lib.EINVAL and word in str(e.value), word
        after = a.state()
        for k in ("S1", "S2", "S1w", "nw", "pivot"):
            assert np.array_equal(before[k], after[k]), k
        assert after["n"] == before["n"] == 5 * 257
        a.reset()
        st = a.state()
        assert (st["n"], st["skipped"]) == (0, 0) and st["has_pivot"]      # a given pivot stays
        assert not st["S1"].any() and not st["S2"].any() and not st["S1w"].any()
        assert not st["nw"].any()
        a.fold_rows(rows)
        check(a.state(), ref, "after reset")


def test_rebase_merges_automatic_pivots(lib_loaded):
    """Two objects with automatic pivots (row 0 and row 100 of walker 0): the second state
    rebased to the first's pivot, then added, agrees with one fold about that pivot to the S2
    bound evaluated at the worse pivot (the larger sum of squares per column)."""
    rows, _ = case(5, 257, 24)
    with Covariance(24, 5) as a, Covariance(24, 5) as b:
        a.fold_rows(rows[:, :100])
        b.fold_rows(rows[:, 100:])
        sa, sb = a.state(), b.state()
        assert np.array_equal(sa["pivot"], rows[0, 0]) and np.array_equal(sb["pivot"], rows[0, 100])
        with pytest.raises(_lib.OlpeError) as e:
            a.add(sb)
        assert e.value.code == _lib.EINVAL and "pivot" in str(e.value)
        a.add(cv.rebase(sb, sa["pivot"]))
        st = a.state()
        a.reset()
        assert not a.state()["has_pivot"]                       # an automatic pivot is forgotten
    ref = cr.sums(rows, sa["pivot"])
    worse = np.maximum(np.diag(ref["S2"]), np.diag(cr.sums(rows, sb["pivot"])["S2"]))
    n = ref["n"]
    r2 = worst(st["S2"] - ref["S2"], 4 * n * U * np.sqrt(np.outer(worse, worse)))
    print(f"rebase + add max |S2 - ref| / bound = {r2:.3e}")
    assert r2 <= 1.0 and st["n"] == n and np.array_equal(st["nw"], ref["nw"])
    assert np.array_equal(st["S2"], st["S2"].T)


def test_sampler_device_chain(lib_loaded):
    """fold(sampler) reads a launch's device chain [W][nrec][PS] in place; fold_rows of the
    chain read back runs the same kernels on the same values in the same layout: the same
    bits.  Once per launch, and again after reset; the right PS and walker count, a second
    launch adds its rows,
    and row_step folds every 7th row."""
    from olpefit_amd.core import Sampler
    with np.load(os.path.join(GOLDEN, "c64.npz"), allow_pickle=False) as z:
        img, nsrc, p0 = z["image"], int(z["nsrc"]), z["p_init"].copy()
    W = 48
    with Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc) as s, Covariance(s.ps, W) as dev, \
            Covariance(s.ps, W) as host, Covariance(s.ps + 1, W) as wrong_ps, \
            Covariance(s.ps, W + 1) as wrong_w, Covariance(s.ps, W) as thin:
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
        a = dev.state()
        assert np.array_equal(a["pivot"], chain[0, 0])
        with Covariance(s.ps, W, pivot=a["pivot"]) as given:
            given.fold_rows(chain)
            g = given.state()
        host.fold_rows(chain)                            # its automatic pivot is the same row
        b = host.state()
        for k in ("S1", "S2", "S1w", "nw", "pivot"):
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], g[k]), k
        assert (a["n"], a["skipped"]) == (b["n"], b["skipped"]) == (W * 300, 0)
        ref = cr.sums(chain)
        assert (np.diag(ref["S2"]) > 0).sum() >= 10      # a column may never have moved
        check(a, ref, "device chain")
        with pytest.raises(_lib.OlpeError) as e:
            dev.fold(s)                                  # the same launch twice
        assert e.value.code == _lib.ESTATE and "already folded" in str(e.value)
        dev.reset()                                      # the same launch may be folded again
        z = dev.state()
        assert (z["n"], z["skipped"]) == (0, 0) and not z["has_pivot"]
        assert not z["S2"].any() and not z["S1w"].any() and not z["nw"].any()
        dev.fold(s)
        again = dev.state()
        assert again["has_pivot"] and (again["n"], again["skipped"]) == (W * 300, 0)
        for k in ("S1", "S2", "S1w", "nw", "pivot"):
            assert np.array_equal(again[k], a[k]), k
        with pytest.raises(_lib.OlpeError) as e:
            dev.fold(s)                                  # and only once
        assert e.value.code == _lib.ESTATE and "already folded" in str(e.value)
        with pytest.raises(_lib.OlpeError) as e:
            wrong_ps.fold(s)
        assert e.value.code == _lib.EINVAL and "PS" in str(e.value)
        with pytest.raises(_lib.OlpeError) as e:
            wrong_w.fold(s)
        assert e.value.code == _lib.EINVAL and "walkers" in str(e.value)
        with pytest.raises(_lib.OlpeError) as e:
            thin.fold(s, row_step=0)
        assert e.value.code == _lib.EINVAL and "row_step" in str(e.value)
        s.run_async(300, 0, 1)
        dev.fold(s)
        thin.fold(s, row_step=7)
        s.sync()
        chain2 = s.chain()
        st = dev.state()
        assert st["n"] == 2 * W * 300 and st["nw"].tolist() == [600] * W
        check(st, cr.sums(np.concatenate([chain, chain2], axis=1), a["pivot"]), "two launches")
        t = thin.state()
        assert t["n"] == W * 43 and t["nw"].tolist() == [43] * W      # ceil(300 / 7)
        assert np.array_equal(t["pivot"], chain2[0, 0])
        check(t, cr.sums(chain2[:, ::7]), "row_step 7")


# ---------------------------------------------------------------------------------------
# Several tiles per workgroup (tests/fold_scale_cases.py; test_fold_plans_cpu.py asserts
# the plans).  Above 2048 tiles a workgroup of cov_fold_kernel walks a run of tiles: the next
# tile's loads are in flight during a walk, the non-finite flags and the waves' column sums
# alternate between two buffers, and a tile's sums are written one tile late.

def between_check(bt, ref, W, label):
    """test_sums_equal_the_restatement's bound on the between term, with every walker's own
    row count (a walker may have lost rows) and m terms."""
    nw = ref["nw"].astype(LD)
    on = ref["nw"] > 0
    d = np.sqrt(nw[:, None] * ref["S2w"])[on]                    # >= |S1w| by Cauchy-Schwarz
    nmax, m = int(ref["nw"].max()), int(on.sum())
    bound = (8 * nmax + 4 * m) * U * (d[:, :, None] * d[:, None, :] / nw[on][:, None, None]
                                      ).sum(axis=0)
    rb = worst(bt["B"] - ref["between"], bound)
    print(f"{label} max |B - ref| / bound = {rb:.3e}")
    assert rb <= 1.0 and np.array_equal(bt["B"], bt["B"].T), (label, rb)
    assert (bt["m"], bt["nw_min"], bt["nw_max"]) == (ref["m"], ref["nw_min"], ref["nw_max"])


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("time_major", [False, True])
@pytest.mark.parametrize("name", list(fc.COV))
def test_several_tiles_per_workgroup(lib_loaded, monkeypatch, name, time_major, pooled):
    """The shapes of fold_scale_cases.COV, each with more than 2048 tiles in the per-walker
    form (2 or 3 a workgroup), in both layouts, per walker and pooled, under the bounds of
    test_sums_equal_the_restatement.  Pooled, the rows are one walker's: only the 1100 x 257
    case then still has more tiles than workgroups (4,418 of 64 rows, 3 a workgroup)."""
    W, N, ncols, tile = fc.COV[name]
    if tile is None:
        monkeypatch.delenv("OLPE_COV_TILE", raising=False)
    else:
        monkeypatch.setenv("OLPE_COV_TILE", tile)
    rows, ref = case(W, N, ncols)
    label = f"{name} {(W, N, ncols)} tile {tile} time_major={time_major} pooled={pooled}"
    with Covariance(ncols, walkers=0 if pooled else W) as c:
        c.fold_rows(lay(rows, time_major), time_major=time_major)
        st = c.state()
        bt = None if pooled else c.between()
    assert st["has_pivot"] and np.array_equal(st["pivot"], rows[0, 0])
    assert st["walkers"] == (0 if pooled else W)
    check(st, ref, label)
    if not pooled:
        between_check(bt, ref, W, label)


@functools.lru_cache(maxsize=None)
def pipeline_case():
    """fold_scale_cases.COV_PIPE with non-finite rows where the tile pipeline turns (the
    positions come from the plan), the explicit pivot and the restated sums."""
    W, N, ncols, tile = fc.COV_PIPE
    plan = fc.cov_plan(W, N, tile)
    rows, _ = case(W, N, ncols)
    bad = rows.copy()
    spots, gone = fc.cov_bad_rows(plan, W, N)
    for k, (w, r) in enumerate(spots):
        bad[w, r, (5 * k + 3) % ncols] = (np.nan, np.inf, -np.inf, np.nan)[k]
    bad[gone, :, 11] = np.nan
    bad.setflags(write=False)
    pivot = rows[0, 0].copy()
    return bad, pivot, cr.sums(bad, pivot), plan, spots, gone


def test_non_finite_rows_against_the_tile_pipeline(lib_loaded, monkeypatch):
    """1100 walkers x 257 rows in tiles of 64: 3 tiles a workgroup.  A non-finite row in the
    first tile of a run (its flag must be gone when the buffer is used again two tiles on), in
    the second and the third tile of one run at the same row of the tile (one flag per
    buffer), in a walker's last tile of one row, and a walker without a finite row (nw = 0:
    the between term has W - 1 terms and nw_min is the others')."""
    monkeypatch.setenv("OLPE_COV_TILE", "64")
    bad, pivot, ref, plan, spots, gone = pipeline_case()
    W, N, ncols, _ = fc.COV_PIPE
    assert ref["skipped"] == len(spots) + N and ref["n"] == W * N - ref["skipped"]
    assert ref["nw"][gone] == 0 and (ref["m"], ref["nw_min"], ref["nw_max"]) == (W - 1, N - 2, N)
    for tm in (False, True):
        with Covariance(ncols, walkers=W, pivot=pivot) as c:
            c.fold_rows(lay(bad, tm), time_major=tm)
            st, bt = c.state(), c.between()
        assert np.array_equal(st["pivot"], pivot)
        assert (st["n"], st["skipped"]) == (ref["n"], ref["skipped"])
        for k in ("S1", "S2", "S1w"):
            assert np.isfinite(st[k]).all(), k
        assert not st["S1w"][gone].any() and st["nw"][gone] == 0
        check(st, ref, f"pipeline non-finite, time_major={tm}")
        between_check(bt, ref, W, f"pipeline non-finite, time_major={tm}")


def test_walker_sums_do_not_depend_on_the_tiles_per_workgroup(lib_loaded, monkeypatch):
    """A tile's column sums are the eight waves' in wave order, a walker's its tiles' in tile
    order, whatever run of tiles a workgroup took: S1w and nw of the 3-tiles-a-workgroup fold
    equal, bit for bit, those of the same rows folded 409 walkers at a time (2045 tiles, one a
    workgroup: the path the small shapes pin), non-finite rows included.  The pooled sums add
    in another order and stay under the bound; a repeated fold repeats every bit."""
    monkeypatch.setenv("OLPE_COV_TILE", "64")
    bad, pivot, ref, plan, _, _ = pipeline_case()
    W, N, ncols, _ = fc.COV_PIPE
    big = []
    for _ in range(2):
        with Covariance(ncols, walkers=W, pivot=pivot) as c:
            c.fold_rows(bad)
            big.append((c.state(), c.between()))
    for k in ("S1", "S2", "S1w", "nw", "pivot"):
        assert np.array_equal(big[0][0][k], big[1][0][k]), k
    assert np.array_equal(big[0][1]["B"], big[1][1]["B"]) and big[0][0]["n"] == big[1][0]["n"]
    per = fc.COV_MAX_SLOTS // plan["tpw"]
    assert per == 409 and fc.cov_plan(per, N, "64")["chunk"] == 1
    s1w, nw, n, skipped = [], [], 0, 0
    S1, S2 = np.zeros(ncols, dtype=LD), np.zeros((ncols, ncols), dtype=LD)
    for w0 in range(0, W, per):
        part = bad[w0:w0 + per]
        with Covariance(ncols, walkers=part.shape[0], pivot=pivot) as c:
            c.fold_rows(part)
            st = c.state()
        s1w.append(st["S1w"])
        nw.append(st["nw"])
        n, skipped = n + st["n"], skipped + st["skipped"]
        S1, S2 = S1 + st["S1"], S2 + st["S2"]
    st = big[0][0]
    assert np.array_equal(np.concatenate(s1w), st["S1w"])
    assert np.array_equal(np.concatenate(nw), st["nw"])
    assert (n, skipped) == (st["n"], st["skipped"]) == (ref["n"], ref["skipped"])
    check(st, ref, "3 tiles a workgroup")
    check({"S1": S1, "S2": S2, "n": n, "skipped": skipped, "walkers": 0}, ref,
          "1 tile a workgroup, three objects")


def test_sampler_device_chain_several_tiles(lib_loaded, monkeypatch):
    """fold(sampler) of a device chain [1100][130][17] in tiles of 64: 3 tiles a walker, 3,300
    tiles, 2 a workgroup, every third workgroup with tiles of two walkers.  The same bits as
    fold_rows of the same rows, and under the bounds."""
    from olpefit_amd.core import Sampler
    monkeypatch.setenv("OLPE_COV_TILE", "64")
    W, N, _ = fc.COV_CHAIN
    img, _ = synth.make_image(32, 2, 0)
    with Sampler(img, 1.0, 1, 1, 2, nsrc=2) as s:
        assert s.ps == 17
        rows, ref = case(W, N, s.ps)
        s.seed(np.arange(1, W + 1))
        s.test_chain_set(rows)
        with Covariance(s.ps, W) as dev, Covariance(s.ps, W) as host:
            dev.fold(s)
            host.fold_rows(rows)
            a, b = dev.state(), host.state()
    for k in ("S1", "S2", "S1w", "nw", "pivot"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["n"], a["skipped"]) == (b["n"], b["skipped"]) == (W * N, 0)
    check(a, ref, "device chain, 2 tiles a workgroup")


L4 = np.array([[1.0, 0.0, 0.0, 0.0], [0.8, 0.6, 0.0, 0.0], [-0.3, 0.2, 0.5, 0.0],
               [0.1, -0.7, 0.2, 0.4]])


@functools.lru_cache(maxsize=None)
def mixed(offset):
    """8 walkers x 500 rows of z L4^T at 512.3, scale 1e-2; walker 5's column 2 moved by
    `offset` sigma of that column."""
    z = np.random.RandomState(11).normal(size=(8, 500, 4))
    rows = 512.3 + 1e-2 * (z @ L4.T)
    rows[5, :, 2] += offset * 1e-2 * np.sqrt((L4[2] ** 2).sum())
    rows.setflags(write=False)
    return rows


def test_end_to_end_covariance_and_rhat(lib_loaded):
    """covariance() of the device's sums, pivot = the column means, against np.cov in
    longdouble: |cov - ref| <= 32 n u sqrt(ref_jj ref_kk).

    Derivation.  With the pivot within one sigma of the mean, S2_jj <= (n - 1) s_j^2 + n
    s_j^2 <= 2 n s_j^2 and |S1_j| <= n s_j (s the sample sigma).  The sums' bounds above give
    |dS2_jk| <= 4 n u sqrt(S2_jj S2_kk) <= 8 n u (n s_j s_k) and |dS1_j| <= 4 n u sqrt(n
    S2_jj) <= 4 sqrt(2) n u (n s_j), hence |d(S1_j S1_k / n)| <= 2 x 4 sqrt(2) n u (n s_j
    s_k) = 11.4 n u (n s_j s_k) to first order.  Their sum, 19.4 n u (n s_j s_k), divided by
    n - 1 is about 20 n u s_j s_k; the subtraction and the division add 2 u.  Rounded up: 32.

    One walker moved by 3 sigma in one column raises Rp and that column's univariate value
    over the unmoved case; both equal the restatement's to 1e-9 relative (the tolerance of
    derived statistics)."""
    out = {}
    for offset in (0.0, 3.0):
        rows = mixed(offset)
        with Covariance(4, walkers=8, pivot=rows.mean(axis=(0, 1))) as c:
            c.fold_rows(rows)
            st, res = c.state(), c.result()
        ref = cr.cov(rows)
        n = st["n"]
        assert n == 4000
        d = np.sqrt(np.diag(ref))
        r = worst(cv.covariance(st) - ref, 32 * n * U * np.outer(d, d))
        print(f"offset {offset}: max |cov - np.cov| / bound = {r:.3e}")
        assert r <= 1.0
        want, rhat = cr.mpsrf(rows)
        mp = res["mpsrf"]
        print(f"offset {offset}: Rp {mp['mpsrf']!r} restated {want!r}; rhat {mp['rhat']}")
        assert (mp["m"], mp["n"]) == (8, 500)
        assert abs(mp["mpsrf"] - want) <= 1e-9 * want
        assert np.allclose(mp["rhat"], rhat, rtol=1e-9, atol=0)
        out[offset] = mp
        if offset == 0.0:
            true = 1e-4 * (L4 @ L4.T)
            assert np.allclose(res["cov"], true, rtol=0, atol=0.1 * 1e-4)   # 4000 samples
    assert out[3.0]["mpsrf"] > out[0.0]["mpsrf"] and out[3.0]["rhat"][2] > out[0.0]["rhat"][2]
    assert out[3.0]["rhat"][2] > 1.2 and out[0.0]["mpsrf"] < 1.05


HEADER = {"KOAID": "N2.20250127.00001.fits", "PARANG": 12.5, "ROTPPOSN": 100.25,
          "INSTANGL": 0.7, "EL": 55.0, "AZ": 200.0, "ROTMODE": "position angle",
          "PARANTEL": -20.0, "ITIME": 1.0, "COADDS": 1, "MULTISAM": 1, "SAMPMODE": 2}


def test_cli_covariance(tmp_path, lib_loaded, capsys):
    """apf_step3.py --covariance on a small step-2 output (8 walkers x 400 rows): the .npz and
    the summary's "covariance" key are written, the printed lines are table_lines of a Python
    fold of load_chains; without the flag the summary has no such key, no file is written
    and the summary is byte-identical to what it was."""
    d = tmp_path / "2014_test"
    path = synth.write_case(str(d), 32, 2)
    img, _ = synth.make_image(32, 2, 0)
    fitsio.write(path, img, {**synth.HEADER, **HEADER})
    out = step2.main([path, "--walkers", "8", "--seed", "3", "--iters", "420", "--burn-in", "20",
                      "-q"])
    plain = step3.main([path, "sys", "-s", "8", "-q"])
    with open(out + "step3_summary.json", "rb") as f:
        before = f.read()
    assert "covariance" not in plain and before == json.dumps(plain, indent=1).encode()
    assert not os.path.exists(out + "00001_covariance.npz")
    capsys.readouterr()
    got = step3.main([path, "sys", "-s", "8", "--covariance"])
    text = capsys.readouterr().out
    chains = step3.load_chains(out, 8, 1)                # [N][8][17], the seed row dropped
    assert chains.shape[0] >= 399 and chains.shape[1:] == (8, 17)
    pivot = np.array([plain["parameters"][k]["mean"] for k in step3.NAMES_2[:-1]]
                     + [float(np.mean(chains[..., -1]))])
    with Covariance(17, walkers=8, pivot=pivot, labels=step3.NAMES_2) as c:
        c.fold_rows(chains, time_major=True)
        st = c.state()
        res = c.result(nsrc=2, pixscale=9.952, param_cols=range(16))
    assert (st["n"], st["skipped"]) == (chains.shape[0] * 8, 0)
    lines = cv.table_lines(res)
    assert len(lines) == 10 + 1 + 16 + 2
    for line in lines:
        assert line in text, line
    z = cv.load_npz(out + "00001_covariance.npz")
    assert z["labels"].tolist() == step3.NAMES_2 and int(z["walkers"]) == 8
    for k in ("S1", "S2", "S1w", "nw", "pivot"):
        assert np.array_equal(z[k], st[k]), k
    assert int(z["n"]) == st["n"]
    assert np.array_equal(z["cov"], res["cov"]) and np.array_equal(z["corr"], res["corr"],
                                                                   equal_nan=True)
    assert np.array_equal(z["sigma_cond"], res["conditional"]["sigma_cond"], equal_nan=True)
    assert z["ellipse_names"].tolist() == ["companion - star"]
    assert float(z["mpsrf"]) == res["mpsrf"]["mpsrf"]
    with open(out + "step3_summary.json") as f:
        saved = json.load(f)
    sc = saved["covariance"]
    assert sc["file"] == got["covariance"]["file"] == out + "00001_covariance.npz"
    assert sc["n"] == st["n"] and sc["walkers"] == 8 and sc["pixscale"] == 9.952
    assert list(sc["columns"]) == step3.NAMES_2[:-1]
    assert sc["mpsrf"] == res["mpsrf"]["mpsrf"]
    e = res["ellipses"][0]
    assert sc["ellipses"]["companion - star"]["semi_major_mas"] == e["semi_major"] * 9.952
    assert {k: v for k, v in saved.items() if k != "covariance"} == json.loads(before)


def test_cli_covariance_three_sources(tmp_path, lib_loaded):
    d = tmp_path / "2016_test"
    path = synth.write_case(str(d), 64, 3)
    img, _ = synth.make_image(64, 3, 0)
    fitsio.write(path, img, {**synth.HEADER, **HEADER})
    out = step2.main([path, "--walkers", "3", "--seed", "5", "--iters", "100", "--burn-in", "20",
                      "-q"], nsrc=3)
    got = step3.main([path, "sys", "-s", "3", "-q", "--covariance", "--covariance-thin", "2"],
                     nsrc=3)["covariance"]
    chains = step3.load_chains(out, 3, 1)
    assert list(got["ellipses"]) == ["b - a", "c - a"] and got["pixscale"] == 9.971
    assert got["n"] == len(chains[::2]) * 3 and got["thin"] == 2
    z = cv.load_npz(out + "00001_covariance.npz")
    assert z["ellipse_names"].tolist() == ["b - a", "c - a"] and z["S2"].shape == (20, 20)
    assert list(got["columns"]) == step3.NAMES_3[:-1]
