"""The host side of the pointwise-deviance fold (olpefit_amd/predictive.py) without a GPU:
planes_from_state and merge_lse against the long-double restatement, compare on hand-made
planes, the saved file's round trip, step 3's argument errors, and the piece plan of
olpe_lik.hip restated from the sources' constants."""
import os
import re

import numpy as np
import pytest

import lik_restatement as lr
from olpefit_amd import predictive as pr, step3, synth

LD = np.longdouble
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "olpefit_amd",
                    "csrc")


def lse_ref(xs):
    """(m, L) of a list of x in long double."""
    xs = np.asarray(xs, dtype=LD)
    m = xs.min()
    return m, np.exp(-(xs - m) / 2).sum()


def test_merge_lse_against_the_restatement():
    rng = np.random.RandomState(3)
    a, b = rng.uniform(0, 30, 40), rng.uniform(5, 60, 17)
    (ma, La), (mb, Lb), (mr, Lr) = lse_ref(a), lse_ref(b), lse_ref(np.concatenate([a, b]))
    m, L = pr.merge_lse(float(ma), float(La), float(mb), float(Lb))
    assert m == float(mr) and abs(L - float(Lr)) <= 8 * lr.U * float(Lr)
    m2, L2 = pr.merge_lse(float(mb), float(Lb), float(ma), float(La))      # the other order
    assert m2 == m and abs(L2 - float(Lr)) <= 8 * lr.U * float(Lr)


def test_merge_lse_edges():
    """An empty side leaves the other as it is (either way round); equal minima add the sums
    exactly; minima 2,000 apart: the larger side's factor underflows to exactly 0."""
    inf = float("inf")
    assert pr.merge_lse(3.0, 2.5, inf, 0.0) == (3.0, 2.5)
    assert pr.merge_lse(inf, 0.0, 3.0, 2.5) == (3.0, 2.5)
    assert pr.merge_lse(inf, 0.0, inf, 0.0) == (inf, 0.0)
    assert pr.merge_lse(7.0, 1.25, 7.0, 2.5) == (7.0, 3.75)
    assert pr.merge_lse(2001.0, 5.0, 1.0, 3.0) == (1.0, 3.0)
    assert pr.merge_lse(1.0, 3.0, 2001.0, 5.0) == (1.0, 3.0)
    m, L = pr.merge_lse(np.array([1.0, inf, 4.0]), np.array([2.0, 0.0, 1.0]),
                        np.array([inf, 2.0, 4.0]), np.array([0.0, 3.0, 1.0]))
    assert np.array_equal(m, [1.0, 2.0, 4.0]) and np.array_equal(L, [2.0, 3.0, 2.0])


def make_state(x, c, split=None):
    """The state the device would hold after folding x [S][n][n] about c, in float64 (the
    fold's own recurrences), optionally as two states cut at `split`."""
    def one(xs):
        d = xs - c
        m = xs.min(axis=0)
        return {"n": xs.shape[0], "n_bad": 0, "a1": d.sum(axis=0), "a2": (d * d).sum(axis=0),
                "m": m, "l": np.exp(-(xs - m) / 2).sum(axis=0)}
    return one(x) if split is None else (one(x[:split]), one(x[split:]))


def test_planes_from_state_against_the_restatement():
    """A 12x12 synthetic frame, 50 rows about the truth: the planes and totals of a state
    built in float64 equal the long-double restatement's to a few S u; two states merged
    with merge_lse give the same."""
    n, S = 12, 50
    img, truth = synth.make_image(n, 2, 0)
    rng = np.random.RandomState(1)
    rows = truth * (1.0 + 1e-3 * rng.normal(size=(S, truth.size)))
    D, err, mask = lr.frame(img)
    mask = mask.copy()
    mask[2, 3] = True
    t, x = lr.deviance(lr.models(rows, n, 2), D, err, mask)
    ref = lr.planes(x, mask)
    x64 = x.astype(np.float64)
    c = x64[0]
    st = make_state(x64, c)
    a, b = make_state(x64, c, 19)
    m, L = pr.merge_lse(a["m"], a["l"], b["m"], b["l"])
    merged = {"n": S, "n_bad": 0, "a1": a["a1"] + b["a1"], "a2": a["a2"] + b["a2"], "m": m,
              "l": L}
    ok = ~mask
    for state in (st, merged):
        planes, sc = pr.planes_from_state(state, np.where(mask, np.nan, c), dev_best=x64[3],
                                          dev_at=x64[4])
        assert sc["pixels"] == int(ok.sum()) and sc["poisoned"] == 0 and sc["samples"] == S
        for k in ("mean_dev", "std_dev", "lppd", "p_waic", "elpd"):
            assert np.isnan(planes[k][mask]).all(), k
            scale = np.abs(x64).max() ** (2 if k == "p_waic" else 1)
            d = np.abs(planes[k][ok] - ref[k][ok].astype(np.float64)).max()
            assert d <= 64 * S * lr.U * scale, (k, d)
        want = lr.scalars(ref, ok, 16, dev_best=x[3], dev_at=x[4])
        for k in ("lppd", "p_waic", "elpd_waic", "waic", "se_elpd", "mean_deviance",
                  "deviance_best", "deviance_at", "p_d", "dic"):
            assert abs(sc[k] - float(want[k])) <= 1e-10 * max(1.0, abs(float(want[k]))), k
        assert sc["p_waic_high"] == want["p_waic_high"]
    # one sample: no variance, lppd = -x / 2
    one = make_state(x64[:1], c)
    planes, sc = pr.planes_from_state(one, np.where(mask, np.nan, c))
    assert np.array_equal(planes["p_waic"][ok], np.zeros(ok.sum()))
    assert np.array_equal(planes["std_dev"][ok], np.zeros(ok.sum()))
    assert np.array_equal(planes["lppd"][ok], -0.5 * x64[0][ok])
    assert np.isnan(sc["dic"])


def test_planes_from_state_poisoned_pixel():
    """A non-finite sum at an unmasked pixel: NaN planes there, counted, out of the totals."""
    x = np.random.RandomState(5).uniform(0.5, 3.0, size=(9, 4, 4))
    c = x[0].copy()
    st = make_state(x, c)
    clean, sc0 = pr.planes_from_state(st, c)
    st["a2"][1, 2] = np.inf
    planes, sc = pr.planes_from_state(st, c)
    assert sc["poisoned"] == 1 and sc["pixels"] == 16 and sc0["poisoned"] == 0
    assert all(np.isnan(planes[k][1, 2]) for k in ("mean_dev", "lppd", "elpd"))
    keep = np.ones((4, 4), bool)
    keep[1, 2] = False
    assert sc["elpd_waic"] == float(clean["elpd"][keep].sum())


def saved(elpd, mask, data, waic=None, dic=0.0):
    e = np.where(mask, np.nan, elpd)
    return {"data": data, "mask": mask, "elpd": e,
            "scalar_waic": -2.0 * np.nansum(e) if waic is None else waic, "scalar_dic": dic}


def test_compare_on_hand_made_planes():
    data = np.arange(16.0).reshape(4, 4)
    mask = np.zeros((4, 4), bool)
    mask[0, 0] = True
    ea = -np.ones((4, 4))
    eb = ea - np.arange(16.0).reshape(4, 4) / 10.0
    c = pr.compare(saved(ea, mask, data, dic=10.0), saved(eb, mask, data, dic=14.5))
    d = np.arange(1, 16) / 10.0
    assert c["pixels"] == 15
    assert c["d_elpd"] == pytest.approx(d.sum(), rel=1e-14)
    assert c["se"] == pytest.approx(np.sqrt(15 * d.var(ddof=1)), rel=1e-14)
    assert c["ratio"] == pytest.approx(c["d_elpd"] / c["se"], rel=1e-14)
    assert c["d_waic"] == pytest.approx(-2.0 * d.sum(), rel=1e-13) and c["d_dic"] == -4.5
    # a pixel poisoned in one run counts in neither
    eb2 = eb.copy()
    eb2[3, 3] = np.nan
    c2 = pr.compare(saved(ea, mask, data), saved(eb2, mask, data))
    assert c2["pixels"] == 14 and c2["d_elpd"] == pytest.approx(d[:-1].sum(), rel=1e-14)
    same = pr.compare(saved(ea, mask, data), saved(ea, mask, data))
    assert same["d_elpd"] == 0.0 and same["se"] == 0.0 and same["d_waic"] == 0.0


def test_compare_refuses_other_masks_and_data():
    data = np.ones((4, 4))
    mask = np.zeros((4, 4), bool)
    other = mask.copy()
    other[1, 1] = True
    e = -np.ones((4, 4))
    with pytest.raises(ValueError, match="mask"):
        pr.compare(saved(e, mask, data), saved(e, other, data))
    with pytest.raises(ValueError, match="data"):
        pr.compare(saved(e, mask, data), saved(e, mask, data + 1.0))
    with pytest.raises(ValueError, match="data"):
        pr.compare(saved(e, mask, data), saved(e[:3], mask[:3], data[:3]))


def test_state_round_trips_through_the_saved_file(tmp_path):
    x = np.random.RandomState(2).uniform(0.5, 3.0, size=(7, 5, 5))
    c = x[0].copy()
    st = make_state(x, c)
    st["pivot"] = np.arange(17.0)
    st["best"] = np.arange(17.0) + 0.5
    mask = np.zeros((5, 5), bool)
    mask[4, 4] = True
    planes, sc = pr.planes_from_state(st, np.where(mask, np.nan, c), dev_best=x[2])
    path = tmp_path / "run_waic.npz"
    pr.write_npz(path, planes, sc, st, c, np.ones((5, 5)), mask, 2, 1, 3)
    z = pr.load_npz(path)
    back = pr.state_of(z)
    assert back["n"] == 7 and back["n_bad"] == 0
    for k in ("pivot", "a1", "a2", "m", "l", "best"):
        assert np.array_equal(back[k], st[k]), k
    assert int(z["nsrc"]) == 2 and int(z["bkgd_mode"]) == 1 and int(z["thin"]) == 3
    assert np.array_equal(z["mask"], mask) and float(z["scalar_waic"]) == sc["waic"]
    again, sc2 = pr.planes_from_state(back, np.where(z["mask"], np.nan, z["c"]),
                                      dev_best=z["dev_best"])
    for k in planes:
        assert np.array_equal(again[k], z[k], equal_nan=True), k
    assert sc2["elpd_waic"] == sc["elpd_waic"]
    assert pr.compare(str(path), z)["d_elpd"] == 0.0        # a path or its dict
    lines = pr.table_lines({**sc, "reduced": 1.0, "log_norm": -3.0})
    assert any("WAIC" in ln for ln in lines) and any("DIC" in ln for ln in lines)


@pytest.mark.parametrize("argv, word", [
    (["--waic", "--from-moments"], "moments are not samples"),
    (["--waic", "--waic-thin", "0"], "--waic-thin 0"),
    (["--waic-against", "x.npz"], "give --waic"),
])
def test_cli_argument_errors(tmp_path, capsys, argv, word):
    with pytest.raises(SystemExit) as e:
        step3.main([str(tmp_path / "2014_x" / "N2.20250127.00001.LDIF.fits"), "sys", "-s", "4"]
                   + argv)
    assert e.value.code == 2 and word in capsys.readouterr().err


def const(text, name):
    m = re.search(r"constexpr\s+[\w ]+?\b%s\s*=\s*([^;]+);" % re.escape(name), text)
    assert m, name
    expr = re.sub(r"(\d)(?:ull|ll|u)\b", r"\1", m.group(1))
    assert re.fullmatch(r"[\d\s*<>()+-]+", expr), (name, expr)
    return int(eval(expr, {"__builtins__": {}}))


def lik_piece_blocks(n):
    """olpe_lik_create's piece size in blocks of kB samples, from the sources' constants."""
    shared = open(os.path.join(CSRC, "olpe_samples.h")).read()
    per_block = n * n * 32
    return min(const(shared, "kMaxPieceBlocks"),
               max(1, const(shared, "kPartBudget") // per_block)), const(shared, "kB")


def test_the_piece_plan_is_the_sources():
    """Four planes of partials per block (32 bytes a pixel) from the shared 64 MB budget:
    half of olpe_resid's blocks, capped by the book kernel's workgroup; both units take
    the constants from olpe_samples.h and keep no copy."""
    lik = open(os.path.join(CSRC, "olpe_lik.hip")).read()
    resid = open(os.path.join(CSRC, "olpe_resid.hip")).read()
    shared = open(os.path.join(CSRC, "olpe_samples.h")).read()
    assert "const size_t per_block = npix * 32;" in lik
    assert "const size_t per_block = npix * 16;" in resid
    plan = "std::min<size_t>(kMaxPieceBlocks, std::max<size_t>(1, kPartBudget / per_block))"
    assert plan in lik and plan in resid
    for unit in (lik, resid):
        assert '#include "olpe_samples.h"' in unit
        for name in ("kMaxPieceBlocks", "kPartBudget", "kPartLimit"):
            assert not re.search(r"constexpr[^;]*\b%s\s*=" % name, unit), name
        assert "resid_scan_kernel(RowMap" not in unit and "struct BlkInfo" not in unit
    assert (const(shared, "kB"), const(shared, "kMaxPieceBlocks")) == (256, 1024)
    assert const(shared, "kPartBudget") == 64 << 20 and const(shared, "kPartLimit") == 1 << 30
    assert lik_piece_blocks(64) == (512, 256)       # olpe_resid's is 1,024 there
    assert lik_piece_blocks(32) == (1024, 256)      # the cap
    assert lik_piece_blocks(33)[0] == 1024 and lik_piece_blocks(128)[0] == 128
    assert lik_piece_blocks(2048)[0] == 1           # one block of 128 MiB: above the budget
    assert 4096 * 4096 * 32 <= const(shared, "kPartLimit") < 5793 * 5793 * 32
