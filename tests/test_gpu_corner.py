"""Corner histograms on the device (olpe_corner.hip, olpefit_amd/corner.py) against NumPy.

Every comparison is np.array_equal on integer counts against np.histogram(col, bins=edges)
and np.histogram2d(ci, cj, bins=[ei, ej]) with the same explicit edges: the bin rule is
NumPy's, so no tolerance exists or is needed.  The shapes are the smallest at which the
kernels can go wrong: sample counts that are no multiple of a wave or a block, a bin count
that is no power of two, pair histograms that do not fit one workgroup's LDS (pair tiles),
both limits, values on and one ulp around every edge.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fold_scale_cases as fc
from olpefit_amd import _lib, corner, fitsio, step2, step3, synth
from olpefit_amd.corner import Corner

pytestmark = pytest.mark.gpu


def numpy_counts(rows, fine, coarse):
    """(h1, h2) of rows [..., C] as NumPy counts them."""
    r = np.asarray(rows, dtype=np.float64)
    r = r.reshape(-1, r.shape[-1])
    h1 = np.stack([np.histogram(r[:, c], bins=fine[c])[0] for c in range(r.shape[1])])
    h2 = np.stack([np.histogram2d(r[:, i], r[:, j], bins=[coarse[i], coarse[j]])[0]
                   for i, j in corner.pairs_of(r.shape[1])])
    assert np.array_equal(h2, np.round(h2))
    return h1.astype(np.uint64), h2.astype(np.uint64)


def check_counts(got, rows, fine, coarse):
    r = np.asarray(rows).reshape(-1, np.asarray(rows).shape[-1])
    h1, h2 = numpy_counts(r, fine, coarse)
    assert got["n"] == r.shape[0]
    assert got["h1"].dtype == np.uint64 and got["h2"].dtype == np.uint64
    assert np.array_equal(got["h1"], h1), np.argwhere(got["h1"] != h1)[:5]
    assert np.array_equal(got["h2"], h2), np.argwhere(got["h2"] != h2)[:5]
    assert np.array_equal(got["outside1"], np.uint64(r.shape[0]) - h1.sum(axis=1))
    assert np.array_equal(got["outside2"], np.uint64(r.shape[0]) - h2.sum(axis=(1, 2)))


def same(a, b):
    return (a["n"] == b["n"] and np.array_equal(a["h1"], b["h1"])
            and np.array_equal(a["h2"], b["h2"]))


def posterior_rows(shape, ncols, seed):
    """Concentrated columns of different centres and widths, a few repeated rows (a
    rejected proposal repeats the row) and some values beyond the ranges used below."""
    rng = np.random.RandomState(seed)
    r = rng.normal(0.0, 1.0, size=tuple(shape) + (ncols,)) * (0.01 + 0.3 * np.arange(ncols)) \
        + 10.0 * np.arange(ncols) - 30.0
    flat = r.reshape(-1, ncols)
    flat[1::5] = flat[0::5][:flat[1::5].shape[0]]
    return r


def ranges_for(rows, shrink=0.9):
    r = Corner.ranges_of(rows)
    if shrink == 1.0:
        return r
    mid, half = r.mean(axis=1), 0.5 * (r[:, 1] - r[:, 0])
    return np.stack([mid - shrink * half, mid + shrink * half], axis=1)


@pytest.mark.parametrize("ncols, nb2, nb1, shape", [
    (5, 2, 2, (3,)),                  # 10 pairs, the smallest histograms
    (17, 20, 2048, (67, 3)),          # the 2-source defaults; 201 samples
    (20, 33, 4096, (130, 5)),         # 33 bins; 190 x 1,089 x 4 B = 828 KB: pair tiles
    (24, 64, 4096, (65,)),            # both limits
])
def test_host_rows_equal_numpy(lib_loaded, ncols, nb2, nb1, shape):
    rows = posterior_rows(shape, ncols, 100 + ncols)
    n = rows.size // ncols
    # three samples: the full range, so that they sit on the first and the last edge;
    # otherwise a narrower one, so that some fall outside
    with Corner(ranges_for(rows, 0.9 if n >= 10 else 1.0), bins=nb2, fine_bins=nb1) as c:
        assert (c.ncols, c.bins, c.fine_bins, c.npairs) == (ncols, nb2, nb1,
                                                            ncols * (ncols - 1) // 2)
        c.fold_rows(rows)
        got = c.counts()
        check_counts(got, rows, c.fine_edges, c.edges)
        assert (got["outside1"].sum() > 0) == (n >= 10)
        assert got["h1"].sum() > 0 and got["h2"].sum() > 0


@pytest.mark.parametrize("form", ["sample", "pair"])
@pytest.mark.parametrize("ncols, nb2, nsamp", [
    (24, 2, 131),        # 276 pairs in one tile: more pairs than lanes
    (20, 33, 650),       # several tiles, 10 to 11 pairs each: several samples per pass
    (6, 64, 513),        # three pairs per tile: 21 samples per pass; one beyond a block
])
def test_both_lane_layouts_equal_numpy(lib_loaded, monkeypatch, form, ncols, nb2, nsamp):
    """OLPE_CORNER_FORM selects the 2-D kernel's lane layout (DESIGN.md §7c's A/B): both
    count what NumPy counts, whatever the number of pairs per tile."""
    monkeypatch.setenv("OLPE_CORNER_FORM", form)
    rows = posterior_rows((nsamp,), ncols, 7 * ncols)
    with Corner(ranges_for(rows), bins=nb2, fine_bins=64) as c:
        c.fold_rows(rows)
        check_counts(c.counts(), rows, c.fine_edges, c.edges)
    monkeypatch.setenv("OLPE_CORNER_FORM", "both")
    with pytest.raises(_lib.OlpeError) as e:
        Corner(ranges_for(rows), bins=nb2, fine_bins=64)
    assert e.value.code == _lib.EINVAL and "OLPE_CORNER_FORM" in str(e.value)


def test_values_on_and_around_every_edge(lib_loaded):
    """Every edge value of both edge sets and one ulp to either side of it, the last edge
    itself, values beyond both ends, NaN, +-inf and -0.0 against a first edge of +0.0, in
    every column, each column's list rotated so that the pairs mix them."""
    ncols, nb2, nb1 = 6, 7, 48
    lo = np.array([0.0, -3.0, 1e-3, -1e6, 0.0, 2.0])
    hi = np.array([1.0, 5.0, 7.0, 1e6, 1e-9, 2.0 + 1e-9])
    coarse = np.stack([np.linspace(a, b, nb2 + 1) for a, b in zip(lo, hi)])
    fine = np.stack([np.linspace(a, b, nb1 + 1) for a, b in zip(lo, hi)])
    assert np.signbit(coarse[0, 0]) == np.signbit(0.0) and coarse[0, 0] == 0.0
    cols = []
    for c in range(ncols):
        e = np.concatenate([coarse[c], fine[c]])
        v = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
                            [e[-1], lo[c] - 1.0, hi[c] + 1.0, -1e300, 1e300, np.nan, np.inf,
                             -np.inf, -0.0, 0.0, 0.5 * (lo[c] + hi[c])]])
        cols.append(np.roll(v, 13 * c))
    rows = np.stack(cols, axis=1)
    assert rows.shape == (3 * (nb2 + nb1 + 2) + 11, ncols)
    with Corner(None, edges=coarse, fine_edges=fine) as c:
        c.fold_rows(rows)
        got = c.counts()
    check_counts(got, rows, fine, coarse)
    assert got["n"] == rows.shape[0] and np.all(got["outside1"] >= 6)
    # -0.0 is in the first bin of a column whose first edge is +0.0 (as NumPy has it)
    with Corner(None, edges=coarse, fine_edges=fine) as c:
        c.fold_rows(np.array([[-0.0, 0.0, 1.0, 0.0, -0.0, 2.0]]))
        one = c.counts()
    assert one["h1"][0, 0] == 1 and one["h1"][4, 0] == 1 and one["outside1"].tolist() == [0] * 6
    assert one["h2"][corner.pairs_of(6).index((0, 4)), 0, 0] == 1


def test_non_uniform_edges(lib_loaded):
    """Any strictly increasing edges: a log-spaced column, a column with a bin 1e-12 wide
    (the first guess is wrong there; the comparisons with the edges decide)."""
    nb2, nb1 = 12, 300
    rng = np.random.RandomState(5)
    thin = lambda n: np.concatenate([[0.0, 1.0, 1.0 + 1e-12], np.linspace(2.0, 9.0, n - 2)])
    coarse = np.stack([np.logspace(-3, 3, nb2 + 1), thin(nb2), np.linspace(-1, 1, nb2 + 1),
                       np.sort(rng.uniform(-5, 5, nb2 + 1))])
    fine = np.stack([np.logspace(-3, 3, nb1 + 1), thin(nb1), np.linspace(-1, 1, nb1 + 1),
                     np.sort(rng.uniform(-5, 5, nb1 + 1))])
    n = 333
    rows = np.stack([10.0 ** rng.uniform(-3.5, 3.5, n), rng.uniform(-0.5, 9.5, n),
                     rng.normal(0, 0.4, n), rng.uniform(-6, 6, n)], axis=1)
    rows[:8, 1] = [1.0, 1.0 + 1e-12, 1.0 + 5e-13, np.nextafter(1.0, 0), 1.0 + 2.5e-13,
                   np.nextafter(1.0 + 1e-12, 0), np.nextafter(1.0 + 1e-12, 2), 0.0]
    with Corner(None, edges=coarse, fine_edges=fine) as c:
        c.fold_rows(rows)
        got = c.counts()
    check_counts(got, rows, fine, coarse)
    assert got["h1"][1, 1] >= 4                  # the 1e-12 wide bin holds its samples


def test_counts_do_not_depend_on_the_split(lib_loaded):
    rows = posterior_rows((211,), 17, 9)
    rg = ranges_for(rows)
    with Corner(rg, bins=20, fine_bins=2048) as one, Corner(rg, bins=20, fine_bins=2048) as seven, \
            Corner(rg, bins=20, fine_bins=2048) as single:
        one.fold_rows(rows)
        cuts = [0, 1, 4, 64, 65, 130, 200, 211]
        for a, b in zip(cuts, cuts[1:]):
            seven.fold_rows(rows[a:b])
        for r in rows:
            single.fold_rows(r)
        a, b, c = one.counts(), seven.counts(), single.counts()
        check_counts(a, rows, one.fine_edges, one.edges)
        assert same(a, b) and same(a, c)
        # reset, then a fold: a fresh object
        seven.reset()
        z = seven.counts()
        assert z["n"] == 0 and not z["h1"].any() and not z["h2"].any()
        seven.fold_rows(rows[:100])
        check_counts(seven.counts(), rows[:100], one.fine_edges, one.edges)
        # empty folds are fine
        seven.fold_rows(rows[:0])
        assert seven.counts()["n"] == 100


def test_two_upload_pieces(lib_loaded):
    """fold_rows uploads pieces of 2^18 samples: 2^18 + 513 are two, the second one short
    (513 samples: a block and one).  The counts are NumPy's and those of the two halves folded
    one after the other."""
    n, ncols, nb2, nb1 = fc.CORNER_PIECES
    rows = posterior_rows((n,), ncols, 23)
    rg = ranges_for(rows)
    with Corner(rg, bins=nb2, fine_bins=nb1) as one, Corner(rg, bins=nb2, fine_bins=nb1) as two:
        one.fold_rows(rows)
        two.fold_rows(rows[:n // 2])
        two.fold_rows(rows[n // 2:])
        a, b = one.counts(), two.counts()
        check_counts(a, rows, one.fine_edges, one.edges)
    assert same(a, b) and a["outside1"].sum() > 0


def test_more_chunks_than_the_grid_takes(lib_loaded):
    """24 columns, 64 and 4,096 bins: 138 pair tiles, so launch_fold takes at most 2048 / 138
    = 14 chunks of the samples; 57,345 samples (the smallest multiple of 512, plus one, with
    more than 14 chunks of 4096) are cut into 13 chunks of 4,608, the last one short."""
    n, ncols, nb2, nb1 = fc.CORNER_CHUNKS
    want, cap, chunks = fc.corner_plan(n, fc.corner_tiles(ncols, nb2, nb1))
    assert want > cap and chunks > 1
    rows = posterior_rows((n,), ncols, 29)
    with Corner(ranges_for(rows), bins=nb2, fine_bins=nb1) as c:
        c.fold_rows(rows)
        got = c.counts()
        check_counts(got, rows, c.fine_edges, c.edges)
    assert got["outside1"].sum() > 0 and got["h2"].sum() > 0


def test_merge_equals_one_object(lib_loaded):
    rows = posterior_rows((150,), 5, 17)
    rg = ranges_for(rows)
    with Corner(rg, bins=9, fine_bins=100) as a, Corner(rg, bins=9, fine_bins=100) as b, \
            Corner(rg, bins=9, fine_bins=100) as whole:
        a.fold_rows(rows[:77])
        b.fold_rows(rows[77:])
        whole.fold_rows(rows)
        a.add(b.counts())
        assert same(a.counts(), whole.counts())
        check_counts(a.counts(), rows, whole.fine_edges, whole.edges)
        with pytest.raises(ValueError):
            a.add({"n": 1, "h1": np.zeros((5, 99), np.uint64), "h2": b.counts()["h2"]})


def test_counters_are_64_bit(lib_loaded):
    big = 2 ** 32 - 2
    with Corner([[0.0, 1.0], [0.0, 1.0]], bins=2, fine_bins=2) as c:
        h1 = np.zeros((2, 2), np.uint64)
        h2 = np.zeros((1, 2, 2), np.uint64)
        h1[0, 0] = big
        h2[0, 0, 1] = big
        c.add({"n": big, "h1": h1, "h2": h2})
        c.fold_rows(np.tile([0.25, 0.75], (5, 1)))
        got = c.counts()
    assert got["n"] == 2 ** 32 + 3
    assert int(got["h1"][0, 0]) == 2 ** 32 + 3 and int(got["h2"][0, 0, 1]) == 2 ** 32 + 3
    assert int(got["h1"][1, 1]) == 5 and int(got["h1"].sum()) == 2 ** 32 + 8
    assert int(got["outside1"][0]) == 0 and int(got["outside2"][0]) == 0


@pytest.mark.parametrize("nsrc", [2, 3])
def test_device_chain_equals_host_rows_and_numpy(lib_loaded, nsrc):
    """fold(sampler) reads each launch's device chain [W][nrec][PS] behind the launch;
    the counts equal fold_rows of the chains read back, and NumPy's."""
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    W = 67
    img, _ = synth.make_image(32, nsrc, 0)
    p0 = initial_parameters(img, synth.guess_values(32, nsrc), nsrc)
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    other = Sampler(img if nsrc == 3 else synth.make_image(32, 3, 0)[0], 1.0, 1, 1, 2,
                    nsrc=5 - nsrc)
    try:
        p0[-1] = s.chi_squared(p0)
        s.seed(np.arange(1, W + 1))
        s.set_state(np.tile(p0, (W, 1)))
        # ranges before any row exists: around the start, as a streaming caller would
        sig = np.maximum(0.02 * np.abs(p0), 0.05)
        rg = Corner.ranges_from_summary(p0, sig, k=5.0)
        ps = s.ps
        with Corner(rg, bins=20, fine_bins=2048) as dev, Corner(rg, bins=20, fine_bins=2048) as host:
            with pytest.raises(_lib.OlpeError) as e:
                dev.fold(s)                                  # nothing launched yet
            assert e.value.code == _lib.ESTATE
            chains = []
            for n_it in (3, 65):
                nrec = s.run_async(n_it, 0, 1)
                dev.fold(s)                                  # behind the launch, no sync
                assert nrec == n_it
                s.sync()
                chains.append(s.chain())
                assert chains[-1].shape == (W, n_it, ps)
                host.fold_rows(chains[-1])
            with pytest.raises(_lib.OlpeError) as e:
                dev.fold(s)                                  # the same launch twice
            assert e.value.code == _lib.ESTATE and "already folded" in str(e.value)
            with pytest.raises(_lib.OlpeError) as e:
                dev.fold(other)                              # another PS
            assert e.value.code == _lib.EINVAL and "PS" in str(e.value)
            a, b = dev.counts(), host.counts()
            assert a["n"] == W * 68 and same(a, b)
            rows = np.concatenate([c.reshape(-1, ps) for c in chains])
            check_counts(a, rows, dev.fine_edges, dev.edges)
            assert a["h2"].sum() > 0
    finally:
        s.close()
        other.close()


def test_cli_corner(tmp_path, lib_loaded, capsys):
    """apf_step3.py --corner on a small step-2 output: the .npz counts equal NumPy's on the
    files' rows, the quantile brackets contain np.percentile, the table is printed and
    recorded; without the flag the summary is what it was."""
    d = tmp_path / "2014_test"
    path = synth.write_case(str(d), 32, 2)
    out = step2.main([path, "--walkers", "4", "--seed", "3", "--iters", "120", "--burn-in", "20",
                      "-q"])
    plain = step3.main([path, "sys", "-s", "4", "-q"])
    with open(out + "step3_summary.json", "rb") as f:
        before = f.read()
    assert "corner" not in plain and before == json.dumps(plain, indent=1).encode()
    assert not os.path.exists(out + "00001_corner.npz")
    capsys.readouterr()
    got = step3.main([path, "sys", "-s", "4", "--corner", "--corner-bins", "11",
                      "--corner-fine-bins", "500"])
    text = capsys.readouterr().out
    assert "Creating a corner plot..." in text and "chisquared" in text and "50%:" in text
    chains = step3.load_chains(out, 4, 1)
    rows = chains.reshape(-1, 17)
    z = corner.load_npz(out + "00001_corner.npz")
    assert z["labels"].tolist() == corner.LABELS_2
    assert z["edges"].shape == (17, 12) and z["fine_edges"].shape == (17, 501)
    rg = Corner.ranges_of(chains)
    assert np.array_equal(z["edges"][:, 0], rg[:, 0]) and np.array_equal(z["edges"][:, -1], rg[:, 1])
    h1, h2 = numpy_counts(rows, z["fine_edges"], z["edges"])
    assert int(z["n"]) == rows.shape[0]
    assert np.array_equal(z["h1"], h1) and np.array_equal(z["h2"], h2)
    assert not z["outside1"].any() and not z["outside2"].any()
    for c in range(17):
        for iq, q in enumerate((0.16, 0.5, 0.84)):
            want = np.percentile(rows[:, c], 100 * q)
            assert z["q_lo"][c, iq] <= want <= z["q_hi"][c, iq], (c, q)
            assert z["q_lo"][c, iq] <= z["q_estimate"][c, iq] <= z["q_hi"][c, iq]
    with open(out + "step3_summary.json") as f:
        saved = json.load(f)
    assert saved["corner"]["samples"] == rows.shape[0] and saved["corner"]["bins"] == 11
    assert saved["corner"]["quantiles"]["xcs"]["lo"] == [float(v) for v in z["q_lo"][0]]
    assert got["corner"]["labels"] == corner.LABELS_2
    assert {k: v for k, v in saved.items() if k != "corner"} == json.loads(before)


def test_cli_corner_three_sources(tmp_path, lib_loaded):
    d = tmp_path / "2016_test"
    path = synth.write_case(str(d), 64, 3)
    out = step2.main([path, "--walkers", "3", "--seed", "5", "--iters", "100", "--burn-in", "20",
                      "-q"], nsrc=3)
    got = step3.main([path, "sys", "-s", "3", "-q", "--corner"], nsrc=3)
    rows = step3.load_chains(out, 3, 1).reshape(-1, 20)
    z = corner.load_npz(out + "00001_corner.npz")
    assert z["labels"].tolist() == corner.LABELS_3 and z["h2"].shape == (190, 20, 20)
    h1, h2 = numpy_counts(rows, z["fine_edges"], z["edges"])
    assert np.array_equal(z["h1"], h1) and np.array_equal(z["h2"], h2)
    assert got["corner"]["samples"] == rows.shape[0] == int(z["n"])
