"""Posterior model and residual images on the device (olpe_resid.hip,
olpefit_amd/residuals.py) against NumPy over the oracle's build_analytical_model.

Bounds.  A model plane is compared with the project's EXACT model tolerance, 1e-13 x
max|ref|; the mean of values each within a bound is within it, and the
shifted sums add ~S u max|M - R| (S <= 773 rows of relative scatter 1e-3: < 1e-16 x
max|ref| x S).  |std(x + e) - std(x)| <= max|e| bounds the std plane by the per-pixel
model error, doubled for the one-pass formula: 2e-13 x max|ref|.  Where the same
operations run on the same values (the best sample's model against olpe_model, D - model,
unusable rows taken out, a repeated sequence of folds) the comparison is np.array_equal.

Shapes: 32x32 (half a wave's lanes masked), 33x33 (odd side: a partial tile in both
directions), 64x64 with 2 and 3 sources, 128x128 (two column passes, 3 sources).  Sample
counts: B - 1, B, B + 1 and three blocks plus a remainder of the fold's block of B = 256.
"""
import functools
import json
import os

import numpy as np
import pytest

from olpefit_amd import _lib, core, fitsio, residuals, step2, step3, synth
from olpefit_amd.core import Sampler
from olpefit_amd.pipeline import initial_parameters
from olpefit_amd.residuals import Residuals
from oracle import olpe_oracle

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}



B = 256
CASES = ["c32", "s33", "c64", "c64_3", "c128_3"]
COUNTS = [1, B - 1, B, B + 1, 3 * B + 5]


@functools.lru_cache(maxsize=None)
def case(name):
    """(image, nsrc, base vector) of a fixture, or of the synthetic 33x33 frame."""
    if name == "s33":
        img, _ = synth.make_image(33, 2, 0)
        return img, 2, initial_parameters(img, synth.guess_values(33, 2), 2)
    g = load_golden(name)
    return g["image"], int(g["nsrc"]), g["p_init"].copy()


def sampler(name):
    img, nsrc, _ = case(name)
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    s.set_eval_mode("exact")
    return s


@functools.lru_cache(maxsize=None)
def posterior(name, S, seed=0):
    """S rows around the case's base vector (relative scatter 1e-3; 1e-3 absolute where
    the base is 0), their oracle models [S][n][n], computed once per (case, S)."""
    img, nsrc, base = case(name)
    rng = np.random.RandomState(1000 * len(name) + S + seed)
    P = base.size - 1
    rows = np.tile(base, (S, 1))
    rows[:, :P] = base[:P] * (1.0 + 1e-3 * rng.normal(size=(S, P))) \
        + np.where(base[:P] == 0.0, 1e-3, 0.0) * rng.normal(size=(S, P))
    rows[:, P] = rng.uniform(1e3, 2e3, size=S)          # a chi^2 column without ties
    n = img.shape[0]
    models = np.stack([olpe_oracle.build_analytical_model(r, n, nsrc) for r in rows])
    rows.setflags(write=False)
    models.setflags(write=False)
    return rows, models


def check_mean_std(planes, models, label=""):
    ref = float(np.abs(models).max())
    d0 = float(np.abs(planes["mean_model"] - models.mean(axis=0)).max())
    d1 = float(np.abs(planes["std_model"] - models.std(axis=0)).max())
    print(f"{label} mean dev {d0 / ref:.3e} x max|ref|, std dev {d1 / ref:.3e} x max|ref|")
    assert d0 <= 1e-13 * ref, (label, d0, ref)
    assert d1 <= 2e-13 * ref, (label, d1, ref)


def same_state(a, b):
    return (a["n"] == b["n"] and a["n_bad"] == b["n_bad"]
            and all(np.array_equal(a[k], b[k], equal_nan=True)
                    for k in ("pivot", "s1", "s2", "best")))


@pytest.mark.parametrize("name", CASES)
def test_best_model_bitwise_equals_olpe_model(lib_loaded, name):
    """Plane 2 is olpe_model's EXACT image of the best row, bit for bit; the best row is
    np.nanargmin's of the chi^2 column, the first of two tied rows, never a NaN one."""
    rows, _ = posterior(name, B + 1)
    rows = rows.copy()
    P = rows.shape[1] - 1
    rows[0, P] = np.nan                                   # a NaN chi^2 placed first
    k = int(np.nanargmin(rows[:, P]))
    tie = (k + 100) % (B + 1) if (k + 100) % (B + 1) != 0 else 5
    rows[tie, P] = rows[k, P]
    want = int(np.nanargmin(rows[:, P]))                  # the first of the two
    assert want == min(k, tie)
    with sampler(name) as s, Residuals(s) as r:
        r.fold_rows(rows)
        best = r.best()
        assert np.array_equal(best, rows[want])
        img = r.images()
        assert np.array_equal(img["best_model"], s.build_analytical_model(best))
        s.set_eval_mode("fast")                           # the context's mode plays no part
        with Residuals(s) as r2:
            r2.fold_rows(rows)
            assert np.array_equal(r2.images()["best_model"], img["best_model"])
        sc = r.scalars()
        assert sc["samples"] == B + 1 and sc["n_bad"] == 0 and sc["best_chi2"] == rows[want, P]


@pytest.mark.parametrize("name", ["c64", "c64_3", "c128_3"])
def test_mean_of_fixture_vectors_against_reference_models(lib_loaded, golden, name):
    """The fixture's own vectors as rows: plane 0 against np.mean of the reference's own
    model images."""
    g = golden(name)
    ref = float(np.abs(g["models"]).max())
    with sampler(name) as s, Residuals(s) as r:
        r.fold_rows(g["params"])
        got = r.images()["mean_model"]
    d = float(np.abs(got - g["models"].mean(axis=0)).max())
    print(f"{name} mean dev {d / ref:.3e} x max|ref|")
    assert d <= 1e-13 * ref


@pytest.mark.parametrize("name, S", [("c64", S) for S in COUNTS] + [("c64_3", S) for S in COUNTS]
                         + [(n, 3 * B + 5) for n in ("c32", "s33", "c128_3")])
def test_mean_and_std_against_numpy(lib_loaded, name, S):
    rows, models = posterior(name, S)
    with sampler(name) as s, Residuals(s) as r:
        r.fold_rows(rows)
        planes = r.images()
        st = r.state()
    assert st["n"] == S and np.array_equal(st["pivot"], rows[0])
    check_mean_std(planes, models, f"{name} S={S}")
    # the host arithmetic of residuals.mean_std on the state gives the same planes
    mean, std = residuals.mean_std(models[0], st["s1"], st["s2"], S)
    ref = float(np.abs(models).max())
    assert np.abs(mean - planes["mean_model"]).max() <= 1e-13 * ref
    assert np.abs(std - planes["std_model"]).max() <= 2e-13 * ref


def test_explicit_pivot_and_tile_heights(lib_loaded, monkeypatch):
    """A caller's pivot (the mean vector) meets the same bounds, and the two tile heights
    of the fold kernel give the same bits."""
    rows, models = posterior("s33", 3 * B + 5)
    states = []
    for h in ("8", "16"):
        monkeypatch.setenv("OLPE_RESID_ROWS", h)
        with sampler("s33") as s, Residuals(s, pivot=rows.mean(axis=0)) as r:
            r.fold_rows(rows)
            check_mean_std(r.images(), models, f"s33 rows={h}")
            states.append(r.state())
    assert same_state(*states)
    monkeypatch.setenv("OLPE_RESID_ROWS", "32")
    with sampler("s33") as s:
        with pytest.raises(_lib.OlpeError) as e:
            Residuals(s)
        assert e.value.code == _lib.EINVAL and "OLPE_RESID_ROWS" in str(e.value)


def test_residual_planes_and_masks(lib_loaded, golden):
    """c64_nan (NaN and inf pixels) with a few saturated pixels: planes 3-6 are NaN exactly
    at the staged-masked pixels, elsewhere D - model and that times 1/err bit for bit."""
    g = golden("c64_nan")
    img = g["image"].copy()
    img[10, 11] = img[40, 3] = 0.9 * 22000.0              # above 0.8 x satlevel
    rows, _ = posterior("c64", B + 1)
    mask, pois2, rn2, _, _ = core.noise_model(img, 1.0, 1, 1, 2)
    assert mask[10, 11] and mask[40, 3] and mask[np.isnan(img)].all()
    with np.errstate(invalid="ignore"):
        inv_err = 1.0 / np.sqrt(rn2 + pois2.astype(np.float64))
    D = img.astype(np.float64)
    with Sampler(img, 1.0, 1, 1, 2, nsrc=2) as s, Residuals(s) as r:
        s.set_eval_mode("exact")
        r.fold_rows(rows)
        p = r.images()
        sc = r.scalars()
        chi = s.chi_squared(r.best())
    for k in ("resid", "nresid", "mean_resid", "mean_nresid"):
        assert np.array_equal(np.isnan(p[k]), mask), k
    for k in ("mean_model", "std_model", "best_model"):
        assert np.isfinite(p[k]).all(), k
    ok = ~mask
    assert np.array_equal(p["resid"][ok], D[ok] - p["best_model"][ok])
    assert np.array_equal(p["nresid"][ok], (D[ok] - p["best_model"][ok]) * inv_err[ok])
    assert np.array_equal(p["mean_resid"][ok], D[ok] - p["mean_model"][ok])
    assert np.array_equal(p["mean_nresid"][ok], (D[ok] - p["mean_model"][ok]) * inv_err[ok])
    assert sc["pixels"] == int(ok.sum())
    assert abs(sc["chi2_best_model"] - chi) <= 1e-12 * chi
    assert abs(sc["chi2_mean_model"] - float((p["mean_nresid"][ok] ** 2).sum())) <= 1e-12 * chi
    at = int(np.nanargmax(np.abs(p["nresid"])))
    assert sc["max_abs_nresid_at"] == at and sc["max_abs_nresid"] == abs(p["nresid"].ravel()[at])
    assert sc["reduced_chi2"] == sc["best_chi2"] / (sc["pixels"] - 16)


def test_unusable_rows(lib_loaded):
    """A leading all-NaN row and a row with one inf parameter, a block apart: counted,
    and the planes are those of the rows without them, bit for bit."""
    good, _ = posterior("c64", 2 * B + 7)
    P = good.shape[1] - 1
    bad1 = np.full(P + 1, np.nan)
    bad2 = good[3].copy()
    bad2[5] = np.inf
    rows = np.concatenate([bad1[None], good[:B + 3], bad2[None], good[B + 3:]])
    with sampler("c64") as s, Residuals(s) as a, Residuals(s) as b, Residuals(s) as c:
        a.fold_rows(rows)
        b.fold_rows(good)
        sa, sb = a.state(), b.state()
        assert sa["n"] == sb["n"] == 2 * B + 7 and sa["n_bad"] == 2 and sb["n_bad"] == 0
        pa, pb = a.images(), b.images()
        for k in pa:
            assert np.array_equal(pa[k], pb[k], equal_nan=True), k
        assert np.array_equal(sa["best"], sb["best"]) and a.scalars()["n_bad"] == 2
        c.fold_rows(np.stack([bad1, bad2]))
        assert c.state()["n"] == 0 and c.state()["n_bad"] == 2
        with pytest.raises(_lib.OlpeError) as e:
            c.finalize()
        assert e.value.code == _lib.ESTATE and "no usable sample" in str(e.value)


def test_splits_agree_and_repeat(lib_loaded):
    """One call, or uneven pieces that are no multiples of the block: the planes agree
    within the bounds, the best row is the same, and each sequence repeats its bits."""
    rows, models = posterior("c64", 3 * B + 5)
    cuts = [0, 37, 37 + B + 1, 37 + B + 1 + 300, 3 * B + 5]
    with sampler("c64") as s:
        states = []
        for pieces in (1, 0, 1, 0):
            with Residuals(s) as r:
                if pieces:
                    r.fold_rows(rows)
                else:
                    for lo, hi in zip(cuts, cuts[1:]):
                        r.fold_rows(rows[lo:hi])
                check_mean_std(r.images(), models, f"split={1 - pieces}")
                states.append(r.state())
    assert same_state(states[0], states[2]) and same_state(states[1], states[3])
    assert np.array_equal(states[0]["best"], states[1]["best"])
    assert states[0]["n"] == states[1]["n"] == 3 * B + 5


def test_more_than_one_piece(lib_loaded):
    """More samples than one piece holds (1,024 blocks at 32x32): the second piece starts
    at a block boundary, so one call and two calls split there give the same bits, and the
    mean is NumPy's over the repeated rows."""
    rows, models = posterior("c32", 3 * B + 5)
    piece = 1024 * B
    reps = -(-(piece + 300) // rows.shape[0])
    many = np.tile(rows, (reps, 1))[:piece + 300].copy()
    many[piece + 7, -1] = 1.0                             # the best row lies in the second piece
    with sampler("c32") as s, Residuals(s) as a, Residuals(s) as b:
        a.fold_rows(many)
        b.fold_rows(many[:piece])
        b.fold_rows(many[piece:])
        sa = a.state()
        assert sa["n"] == piece + 300 and same_state(sa, b.state())
        assert np.array_equal(sa["best"], many[piece + 7])
        got = a.images()["mean_model"]
    idx = np.arange(piece + 300) % rows.shape[0]
    w = np.bincount(idx, minlength=rows.shape[0]).astype(np.float64)
    want = np.tensordot(w / w.sum(), models, axes=1)
    ref = float(np.abs(models).max())
    d = float(np.abs(got - want).max())
    print(f"two pieces: mean dev {d / ref:.3e} x max|ref|")
    assert d <= 1e-13 * ref


@pytest.mark.parametrize("name, W", [("c64", 7), ("c128_3", 13)])
def test_device_chain_thinned_equals_host_rows(lib_loaded, name, W):
    """fold(sampler, 3, 2) reads rows 0, 3, ... of walkers 0, 2, ... of the launch's
    device chain in place: the same bits as fold_rows of that subset read back."""
    _, _, base = case(name)
    with sampler(name) as s, Residuals(s) as dev, Residuals(s) as host:
        with pytest.raises(_lib.OlpeError) as e:
            dev.fold(s)                                   # nothing launched yet
        assert e.value.code == _lib.ESTATE
        s.seed(np.arange(1, W + 1))
        p0 = base.copy()
        p0[-1] = s.chi_squared(p0)
        s.set_state(np.tile(p0, (W, 1)))
        assert s.run_async(37, 0, 1) == 37
        dev.fold(s, row_step=3, walker_step=2)            # behind the launch, no sync
        s.sync()
        chain = s.chain()
        sub = chain[::2, ::3]
        assert sub.shape == ((W + 1) // 2, 13, s.ps)
        host.fold_rows(sub)
        a, b = dev.state(), host.state()
        assert a["n"] == sub.shape[0] * 13 and same_state(a, b)
        pa, pb = dev.images(), host.images()
        for k in pa:
            assert np.array_equal(pa[k], pb[k], equal_nan=True), k
        with pytest.raises(_lib.OlpeError) as e:
            dev.fold(s)                                   # the same launch twice
        assert e.value.code == _lib.ESTATE and "already folded" in str(e.value)
        for bad in ((0, 1), (1, 0), (-2, 1)):
            with pytest.raises(_lib.OlpeError) as e:
                host.fold(s, *bad)
            assert e.value.code == _lib.EINVAL
    with sampler("c32") as other, sampler(name) as s, Residuals(s) as r:
        other.seed([1])
        other.set_state(case("c32")[2])
        other.run(2, 0, 1)
        with pytest.raises(_lib.OlpeError) as e:
            r.fold(other)                                 # another side
        assert e.value.code == _lib.EINVAL and "side" in str(e.value)


def test_merge(lib_loaded):
    """Rows split over two objects with one explicit pivot, merged with add; differing
    pivots are refused; an empty object adopts the incoming pivot."""
    rows, models = posterior("c64_3", 3 * B + 5)
    pivot = rows[:50].mean(axis=0)
    cut = B + 77
    with sampler("c64_3") as s, Residuals(s, pivot) as one, Residuals(s, pivot) as a, \
            Residuals(s, pivot) as b, Residuals(s) as empty, Residuals(s, rows[1]) as other:
        one.fold_rows(rows)
        a.fold_rows(rows[:cut])
        b.fold_rows(rows[cut:])
        a.add(b.state())
        st = a.state()
        assert st["n"] == 3 * B + 5 and np.array_equal(st["pivot"][:-1], pivot[:-1])
        check_mean_std(a.images(), models, "merged")
        assert np.array_equal(a.best(), one.best())
        ref = float(np.abs(models).max())
        assert np.abs(a.images()["mean_model"] - one.images()["mean_model"]).max() <= 2e-13 * ref
        other.fold_rows(rows[:3])
        with pytest.raises(_lib.OlpeError) as e:
            other.add(b.state())
        assert e.value.code == _lib.EINVAL and "pivot" in str(e.value)
        empty.add(one.state())
        assert same_state(empty.state(), one.state())
        for k, v in empty.images().items():
            assert np.array_equal(v, one.images()[k], equal_nan=True), k
        empty.reset()
        assert empty.state()["n"] == 0
        with pytest.raises(_lib.OlpeError) as e:
            empty.finalize()
        assert e.value.code == _lib.ESTATE


def test_cli_residuals(tmp_path, lib_loaded, capsys):
    """apf_step3.py --residuals on a small step-2 output: the npz and the four FITS files,
    read back equal; the scalars printed and recorded; the rest of the summary as before."""
    d = tmp_path / "2014_test"
    path = synth.write_case(str(d), 32, 2)
    out = step2.main([path, "--walkers", "4", "--seed", "3", "--iters", "120", "--burn-in", "20",
                      "-q"])
    plain = step3.main([path, "sys", "-s", "4", "-q"])
    with open(out + "step3_summary.json", "rb") as f:
        before = f.read()
    assert "residuals" not in plain and before == json.dumps(plain, indent=1).encode()
    capsys.readouterr()
    got = step3.main([path, "sys", "-s", "4", "--residuals", "--residuals-thin", "3"])
    text = capsys.readouterr().out
    assert "Building model and residual images..." in text and "reduced_chi2" in text
    chains = step3.load_chains(out, 4, 1)
    rows = chains[::3].reshape(-1, 17)
    z = residuals.load_npz(out + "00001_residuals.npz")
    assert int(z["scalar_samples"]) == rows.shape[0] and int(z["scalar_n_bad"]) == 0
    assert np.array_equal(z["best"], rows[int(np.nanargmin(rows[:, 16]))])
    img, _ = fitsio.getdata_header(path)
    assert np.array_equal(z["data"], np.asarray(img, dtype=np.float64))
    models = np.stack([olpe_oracle.build_analytical_model(r, 32, 2) for r in rows])
    ref = float(np.abs(models).max())
    assert np.abs(z["mean_model"] - models.mean(axis=0)).max() <= 1e-13 * ref
    assert np.abs(z["std_model"] - models.std(axis=0)).max() <= 2e-13 * ref
    for suffix, key in (("model", "best_model"), ("meanmodel", "mean_model"),
                        ("resid", "resid"), ("nresid", "nresid")):
        back, _ = fitsio.getdata_header(out + f"00001_{suffix}.fits")
        assert np.array_equal(np.asarray(back, dtype=np.float64), z[key], equal_nan=True), suffix
    with open(out + "step3_summary.json") as f:
        saved = json.load(f)
    assert saved["residuals"]["samples"] == rows.shape[0] and saved["residuals"]["thin"] == 3
    assert saved["residuals"]["best_chi2"] == float(z["scalar_best_chi2"])
    assert got["residuals"]["file"] == out + "00001_residuals.npz"
    assert {k: v for k, v in saved.items() if k != "residuals"} == json.loads(before)
