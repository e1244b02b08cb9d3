"""Corner histograms (olpe_corner_*, olpefit_amd/corner.py): what needs no GPU.

Argument validation of the C entry (OLPE_EINVAL with a message before any GPU call), the
host arithmetic of the quantile brackets on hand-made counts (yardstick: np.percentile of
the samples the counts were made from with np.histogram), the .npz round trip, and step 3
without --corner leaving exactly what it left before the option existed.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from olpefit_amd import _lib, corner, pipeline, step3


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _create(lib, ncols, nb1, nb2, e1=None, e2=None, out=True):
    e1 = np.stack([np.linspace(0.0, 1.0, nb1 + 1)] * ncols) if e1 is None else e1
    e2 = np.stack([np.linspace(0.0, 1.0, nb2 + 1)] * ncols) if e2 is None else e2
    e1 = np.ascontiguousarray(e1, dtype=np.float64)
    e2 = np.ascontiguousarray(e2, dtype=np.float64)
    h = C.c_void_p()
    rc = lib.olpe_corner_create(0, ncols, e1.ctypes.data_as(_lib._pd), nb1,
                                e2.ctypes.data_as(_lib._pd), nb2, C.byref(h) if out else None)
    assert not h.value or rc == 0
    if rc == 0:                      # (only where a GPU is present: not what is tested here)
        lib.olpe_corner_destroy(h)
    return rc, lib.olpe_last_error().decode()


@pytest.mark.parametrize("ncols, nb1, nb2, word", [
    (1, 8, 4, "ncols 1"), (25, 8, 4, "ncols 25"), (3, 8, 1, "nb2 1"), (3, 8, 65, "nb2 65"),
    (3, 1, 4, "nb1 1"), (3, 4097, 4, "nb1 4097")])
def test_create_rejects_shapes_before_any_gpu_call(lib, ncols, nb1, nb2, word):
    rc, msg = _create(lib, ncols, nb1, nb2)
    assert rc == _lib.EINVAL and word in msg, msg


def test_create_rejects_bad_edges_naming_the_column(lib):
    good1 = np.stack([np.linspace(0.0, 1.0, 9)] * 3)
    good2 = np.stack([np.linspace(0.0, 1.0, 5)] * 3)
    e = good1.copy()
    e[1, 3] = np.nan
    rc, msg = _create(lib, 3, 8, 4, e1=e)
    assert rc == _lib.EINVAL and "column 1" in msg and "not finite" in msg
    e = good2.copy()
    e[2, 4] = np.inf
    rc, msg = _create(lib, 3, 8, 4, e2=e)
    assert rc == _lib.EINVAL and "column 2" in msg and "not finite" in msg
    e = good1.copy()
    e[0, 5] = e[0, 4]                                   # equal
    rc, msg = _create(lib, 3, 8, 4, e1=e)
    assert rc == _lib.EINVAL and "column 0" in msg and "strictly increasing" in msg
    e = good2.copy()
    e[2] = e[2][::-1]                                   # decreasing
    rc, msg = _create(lib, 3, 8, 4, e2=e)
    assert rc == _lib.EINVAL and "column 2" in msg and "strictly increasing" in msg
    rc, msg = _create(lib, 3, 8, 4, out=False)
    assert rc == _lib.EINVAL and "NULL out" in msg
    assert lib.olpe_corner_create(0, 3, None, 8, good2.ctypes.data_as(_lib._pd), 4,
                                  C.byref(C.c_void_p())) == _lib.EINVAL
    assert lib.olpe_corner_create(-1, 3, good1.ctypes.data_as(_lib._pd), 8,
                                  good2.ctypes.data_as(_lib._pd), 4,
                                  C.byref(C.c_void_p())) == _lib.EINVAL     # no CPU path


def test_null_handles_are_errors(lib):
    assert lib.olpe_corner_fold_ctx(None, None) == _lib.EINVAL
    assert lib.olpe_corner_fold_rows(None, None, 0) == _lib.EINVAL
    assert lib.olpe_corner_get(None, None, None, None) == _lib.EINVAL
    assert lib.olpe_corner_add(None, 0, None, None) == _lib.EINVAL
    assert lib.olpe_corner_reset(None) == _lib.EINVAL
    lib.olpe_corner_destroy(None)


def _table(cols, edges, q):
    """quantile_table of np.histogram's counts of the columns."""
    h1 = np.stack([np.histogram(x, bins=e)[0] for x, e in zip(cols, edges)]).astype(np.uint64)
    return corner.Corner.quantile_table(edges, h1, len(cols[0]), q)


def _check_brackets(cols, edges, q, t):
    for c, x in enumerate(cols):
        for iq, qq in enumerate(q):
            want = np.percentile(x, 100 * qq)
            lo, hi, est = t["lo"][c, iq], t["hi"][c, iq], t["estimate"][c, iq]
            assert lo <= want <= hi, (c, qq, lo, want, hi)
            assert lo <= est <= hi
            assert lo in edges[c] and hi in edges[c]


def test_quantile_brackets_contain_numpy_percentile():
    rng = np.random.RandomState(7)
    q = (0.16, 0.5, 0.84, 0.0, 1.0, 0.25, 0.999)
    for n in (1, 2, 5, 100, 101, 1000, 4097):
        cols = [rng.normal(3.0, 2.0, n), rng.exponential(1.0, n), np.round(rng.normal(0, 3, n))]
        edges = np.stack([np.linspace(x.min(), x.max() if x.max() > x.min() else x.min() + 1,
                                      257) for x in cols])
        t = _table(cols, edges, q)
        assert t["notes"] == ["", "", ""]
        _check_brackets(cols, edges, q, t)


def test_quantile_exactly_on_an_order_statistic_and_between_two_bins():
    # 5 samples, q = 0.5 -> v = 2 exactly: the bracket is the one bin of the third sample
    x = np.array([0.5, 1.5, 4.5, 8.5, 9.5])
    edges = np.linspace(0.0, 10.0, 11)[None, :]
    t = _table([x], edges, (0.5, 0.25))
    assert (t["lo"][0, 0], t["hi"][0, 0]) == (4.0, 5.0)
    assert np.percentile(x, 50) == 4.5
    # q = 0.25 -> v = 1 exactly: the second sample's bin alone
    assert (t["lo"][0, 1], t["hi"][0, 1]) == (1.0, 2.0)
    # 4 samples, q = 0.5 -> v = 1.5: between the second and third samples, which sit in
    # bins 1 and 8: the bracket is their union and holds the interpolated 5.0
    x = np.array([0.5, 1.5, 8.5, 9.5])
    t = _table([x], edges, (0.5,))
    assert (t["lo"][0, 0], t["hi"][0, 0]) == (1.0, 9.0)
    assert np.percentile(x, 50) == 5.0 and 1.0 <= t["estimate"][0, 0] <= 9.0
    # q (N - 1) within rounding of an integer: 0.16 * 100 is 16 give or take an ulp, and
    # NumPy may interpolate from either side of the 17th sample
    x = np.sort(np.random.RandomState(3).uniform(0, 10, 101))
    e = np.linspace(0.0, 10.0, 2049)[None, :]
    t = _table([x], e, (0.16,))
    assert t["lo"][0, 0] <= x[15] and x[17] <= t["hi"][0, 0]
    _check_brackets([x], e, (0.16,), t)


def test_quantiles_of_a_column_with_outside_samples_are_nan():
    x = np.array([0.5, 1.5, 2.5, 11.0])                 # one beyond the last edge
    y = np.array([0.5, 1.5, 2.5, 3.5])
    edges = np.stack([np.linspace(0.0, 10.0, 11)] * 2)
    t = _table([x, y], edges, (0.16, 0.5, 0.84))
    assert np.all(np.isnan(t["lo"][0])) and np.all(np.isnan(t["hi"][0]))
    assert np.all(np.isnan(t["estimate"][0]))
    assert "1 of 4 samples outside" in t["notes"][0]
    assert t["notes"][1] == "" and np.all(np.isfinite(t["lo"][1]))
    empty = corner.Corner.quantile_table(edges, np.zeros((2, 10), np.uint64), 0)
    assert np.all(np.isnan(empty["lo"])) and empty["notes"][0] == "no samples folded"


def test_ranges():
    rows = np.array([[[1.0, np.nan, 5.0], [3.0, 2.0, 5.0]], [[-1.0, np.inf, 5.0], [0.0, 4.0, 5.0]]])
    r = corner.Corner.ranges_of(rows)
    assert r.tolist() == [[-1.0, 3.0], [2.0, 4.0], [4.5, 5.5]]
    with pytest.raises(ValueError, match="column 1"):
        corner.Corner.ranges_of(np.array([[1.0, np.nan], [2.0, np.nan]]))
    r = corner.Corner.ranges_from_summary([1.0, 2.0], [0.5, 0.0], k=4.0)
    assert r.tolist() == [[-1.0, 3.0], [1.5, 2.5]]
    assert corner.pairs_of(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert len(corner.LABELS_2) == 17 and len(corner.LABELS_3) == 20
    assert corner.LABELS_2[:-1] == step3.NAMES_2[:-1] and corner.LABELS_3[:-1] == step3.NAMES_3[:-1]


def test_npz_round_trip(tmp_path):
    rng = np.random.RandomState(11)
    cols = [rng.normal(0, 1, 500), rng.normal(5, 2, 500), rng.uniform(-1, 1, 500)]
    cols[2][7] = 3.0                                    # outside: a NaN row of the table
    fine = np.stack([np.linspace(-10.0, 15.0, 129), np.linspace(-10.0, 15.0, 129),
                     np.linspace(-1.0, 1.0, 129)])
    coarse = fine[:, ::16].copy()
    h1 = np.stack([np.histogram(x, bins=e)[0] for x, e in zip(cols, fine)]).astype(np.uint64)
    pairs = corner.pairs_of(3)
    h2 = np.stack([np.histogram2d(cols[i], cols[j], bins=[coarse[i], coarse[j]])[0]
                   for i, j in pairs]).astype(np.uint64)
    counts = {"n": 500, "h1": h1, "h2": h2, "outside1": np.uint64(500) - h1.sum(axis=1),
              "outside2": np.uint64(500) - h2.sum(axis=(1, 2))}
    table = corner.quantile_table(fine, h1, 500)
    path = str(tmp_path / "c.npz")
    corner.save_npz(path, ["a", "b", "c"], coarse, fine, counts, table)
    z = corner.load_npz(path)
    assert z["labels"].tolist() == ["a", "b", "c"] and int(z["n"]) == 500
    assert np.array_equal(z["h1"], h1) and np.array_equal(z["h2"], h2)
    assert z["h1"].dtype == np.uint64 and z["h2"].dtype == np.uint64
    assert np.array_equal(z["edges"], coarse) and np.array_equal(z["fine_edges"], fine)
    assert z["outside1"].tolist() == [0, 0, 1] and z["outside2"].tolist() == [0, 1, 1]
    assert z["pairs"].tolist() == [list(p) for p in pairs]
    assert z["q"].tolist() == [0.16, 0.5, 0.84]
    for k in ("lo", "hi", "estimate"):
        assert np.array_equal(z["q_" + k], table[k], equal_nan=True)
    assert np.all(np.isnan(z["q_lo"][2])) and "outside" in z["q_notes"][2]
    assert z["q_notes"][0] == ""


def test_step3_without_corner_is_unchanged(tmp_path, golden):
    """Without --corner step 3 leaves the files and the summary it left before the option
    existed (the statistics test_pipeline pins with the same fixture), and --corner with
    --from-moments is an argument error before anything is read."""
    g = golden("gr")
    chains = g["chains2"]
    N, M, ps = chains.shape
    image = str(tmp_path / "N2.20250127.00042.LDIF.fits")
    outdir = pipeline.image_paths(image)[2]
    os.makedirs(outdir)
    paths = [outdir + f"{w}_finalarray_mpi.csv" for w in range(M)]
    pipeline.write_chain_csvs(paths, chains.transpose(1, 0, 2), nan_row=True)
    before = set(os.listdir(outdir))
    out = step3.main([image, "x", "-s", str(M), "-q"])
    assert set(os.listdir(outdir)) == before | {"step3_summary.json"}
    assert list(out) == ["walkers", "rows_per_walker", "additional_burnin", "source",
                         "gr_rc_mean", "gr_rc_std", "parameters"]
    with open(outdir + "step3_summary.json", "rb") as f:
        assert f.read() == json.dumps(out, indent=1).encode()
    assert out["parameters"] == step3.summary(chains, nsrc=2)
    with pytest.raises(SystemExit) as e:
        step3.main([image, "x", "-s", str(M), "-q", "--corner", "--from-moments"])
    assert e.value.code == 2
    assert set(os.listdir(outdir)) == before | {"step3_summary.json"}
