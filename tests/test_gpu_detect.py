"""The companion detection map on the device (olpe_detect.hip, olpefit_amd/detect.py) against
the long-double restatement of tests/detect_restatement.py over the oracle's
build_analytical_model, at a chosen subset of the candidate lattice: the four corners, the
edge midpoints, the fitted sources' nearest lattice points and their neighbours, points at
masked pixels and 40 seeded random ones.

Bounds (derived, not tuned).  delta = 1e-13 x max|M_ref| is the project's EXACT model
tolerance, u = 2^-53.
  K        The argument of each Gaussian is a sum of three terms; a coefficient carries 4
           roundings (cos or sin to 1 ulp, its square, the divisions by sx^2 and sy^2, the sum,
           the half), the offset's subtraction, its square or product and the product with
           the coefficient 4 more, the two additions 2: |d arg| <= 10 u T with T the sum of
           the terms' absolute values.  exp_neg is within 2 ulp, the weights (1 - q), q, the
           two products and the sum add 3:  dK <= sum_k (5 + 10 T_k) u |component k|.
  z, w     z = w (D - M): the model within delta, the subtraction, w = (1 / err)^2 with
           1 / err within 1 ulp, and the product:  dz <= w delta + 4 u |z|,  dw <= 3 u w.
  N, Q     |dN| <= sum (w delta K + 4 u |z| K + |z| dK) + n^2 u sum |z K| (n^2 fused
           additions);  |dQ| <= sum 2 w K dK + (n^2 + 4) u Q.
  A        <= (dN / Q + |N| dQ / Q^2) / (1 - dQ / Q) + 2 u |A|;  sigma_A <= sigma (dQ / 2Q /
           (1 - dQ / Q) + 3 u);  snr <= dN / sqrt(Q) / (1 - dQ / Q) + |snr| (the same).
  means    <= max_s (the sample's bound) + 2 S u max_s |x - x_p| (the shifted sum of S terms)
           + 2 u |mean|;  stds <= twice the samples' bound + the same spread (|std(x + e) -
           std(x)| <= max |e|, doubled for the one-pass form, as in test_gpu_resid).
  sigma_stat   mean sigma^2 within max_s 2 sigma dsigma + (S + 2) u of itself, through the
           square root;  sigma_total the same with var A's 2 std b + b^2 added;  snr_marg
           from amp_mean's and sigma_total's bounds as A from N's and Q's.
Where the same operations run on the same values the comparison is np.array_equal: repeats,
one sample against point, the best row's planes against point(best), the device chain
against the same rows from the host, unusable rows taken out, two objects folded on halves
of B rows each and merged, the even lattice points of oversample 2 and 4 against 1, and
planes_from_state against finalize.

Shapes: 32 (half the lanes idle), 33 (partial tiles both ways; oversample 2 and 4), 64 with 2
and 3 sources, 128 with 3 sources and 5 rows (two column tiles, the table beyond the LDS).
Counts 1, B - 1, B, B + 1, 3 B + 5 of B = 256 at 64x64 -- prefixes of one set of rows, so the
restatement runs once per frame -- and B + 1 elsewhere.
"""
import functools
import json

import numpy as np
import pytest

import detect_restatement as dr
from olpefit_amd import _lib, detect as dt, fitsio, step2, step3, synth
from olpefit_amd.core import Sampler
from olpefit_amd.detect import Detect
from test_gpu_predictive import case, scatter

pytestmark = pytest.mark.gpu
LD = np.longdouble
B = 256
COUNTS = [1, B - 1, B, B + 1, 3 * B + 5]
KEYS = ("amp_mean", "amp_std", "sigma_stat", "sigma_total", "snr_mean", "snr_std", "snr_marg")
PLANE_CASES = ([("c64", 1, S) for S in COUNTS] + [("c64_3", 1, S) for S in COUNTS]
               + [("c32", 1, B + 1), ("s33", 1, B + 1), ("s33", 2, B + 1), ("s33", 4, B + 1),
                  ("c128_3", 1, 5), ("y33", 1, B + 1), ("y64", 1, B + 1), ("y64_3", 1, B + 1)])
SMAX = {"c64": 3 * B + 5, "c64_3": 3 * B + 5, "c128_3": 5}


class Ref:
    """The restatement of one set of rows on one frame at the chosen candidates, once."""

    def __init__(self, img, nsrc, rows, oversample=1, cand=None):
        self.rows, self.nsrc, self.os = rows, nsrc, oversample
        self.fr = dr.Frame(img)
        self.n = self.fr.n
        self.g = dt.lattice_side(self.n, oversample)
        self.cand = dr.chosen(self.n, nsrc, rows[0], self.fr.mask, oversample) if cand is None \
            else np.asarray(cand)
        self.flat = self.cand[:, 0] * self.g + self.cand[:, 1]
        with np.errstate(all="ignore"):
            self.e = dr.ensemble(self.fr, rows, nsrc, self.cand, oversample)
        rows.setflags(write=False)

    def planes(self, S=None):
        with np.errstate(all="ignore"):
            return dr.planes(self.e, S)

    def at(self, plane):
        return np.asarray(plane).reshape(-1)[self.flat]


@functools.lru_cache(maxsize=None)
def reference(name):
    img, nsrc, base = case(name)
    S = SMAX.get(name, B + 1)
    return Ref(img, nsrc, scatter(base, S, 1000 * len(name) + S))


@functools.lru_cache(maxsize=None)
def reference_os(name, oversample):
    if oversample == 1:
        return reference(name)
    img, nsrc, _ = case(name)
    return Ref(img, nsrc, reference(name).rows, oversample)


def sampler(name):
    img, nsrc, _ = case(name)
    return Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)


def same_state(a, b):
    return (a["n"] == b["n"] and a["n_bad"] == b["n_bad"]
            and all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("pivot", "sums", "best")))


def check(maps, ref, S, label):
    """The seven sample planes at the chosen candidates within their bounds; prints and
    returns the largest ratio to each bound."""
    want, bound = ref.planes(S)
    worst = {}
    for k in KEYS:
        got = ref.at(maps[k])
        assert np.isfinite(got).all(), (label, k)
        d = np.abs(got.astype(LD) - want[k]).astype(np.float64)
        b = bound[k]
        worst[k] = float((d / b).max()) if np.all(b > 0) else float(d.max() == 0) - 1.0
        assert np.all(d <= b), (label, k, float((d / np.maximum(b, 1e-300)).max()))
    print(label, " ".join(f"{k} {v:.2e}" for k, v in worst.items()), "(x bound)")
    return worst


def check_point(planes, ref, s, label):
    for i, (k, bk) in enumerate((("A", "bA"), ("sigma", "bsigma"), ("snr", "bsnr"))):
        d = np.abs(ref.at(planes[i]).astype(LD) - ref.e[k][s]).astype(np.float64)
        print(label, k, float((d / ref.e[bk][s]).max()), "x bound")
        assert np.all(d <= ref.e[bk][s]), (label, k)


@pytest.mark.parametrize("name, oversample, S", PLANE_CASES)
def test_planes_against_the_restatement(lib_loaded, name, oversample, S):
    ref = reference_os(name, oversample)
    rows = ref.rows[:S]
    with sampler(name) as s, Detect(s, oversample=oversample) as d:
        d.fold_rows(rows)
        maps, sc = d.maps(), d.scalars()
        st = d.state()
        check(maps, ref, S, f"{name} os {oversample} S {S}")
        assert sc["samples"] == S and sc["n_bad"] == 0 and sc["blind"] == 0
        assert sc["pixels"] == int((~ref.fr.mask).sum())
        assert np.array_equal(st["pivot"], rows[0])
        assert np.array_equal(st["best"], rows[int(np.argmin(rows[:, -1]))])
        # finalize's arithmetic restated on the host: the same bits
        piv, best = d.point(st["pivot"]), d.point(st["best"])
        again, sc2 = dt.planes_from_state(st, piv, best)
        for k in dt.PLANES:
            assert np.array_equal(again[k], maps[k], equal_nan=True), k
        for k in ("samples", "n_bad", "blind", "max_snr", "max_snr_at", "min_snr",
                  "median_sigma"):
            assert sc2[k] == sc[k], k
        check_point(best, ref, int(np.argmin(rows[:, -1])), f"{name} best")


@pytest.mark.parametrize("name, oversample", [("c64", 1), ("c64_3", 1), ("s33", 2)])
def test_one_sample_repeats_and_the_best_row(lib_loaded, name, oversample):
    """S = 1 is point(row) in every bit (the sums about the row itself are zero); a repeat
    gives the same state; amp_best, sigma_best, snr_best are point(best())."""
    ref = reference_os(name, oversample)
    rows = ref.rows[:B + 1]
    with sampler(name) as s, Detect(s, oversample=oversample) as one, \
            Detect(s, oversample=oversample) as a, Detect(s, oversample=oversample) as b:
        one.fold_rows(rows[:1])
        m, p = one.maps(), one.point(rows[0])
        assert np.array_equal(m["amp_mean"], p[0]) and np.array_equal(m["snr_mean"], p[2])
        assert np.array_equal(m["amp_best"], p[0]) and np.array_equal(m["sigma_best"], p[1])
        assert np.all(m["amp_std"] == 0.0) and np.all(m["snr_std"] == 0.0)
        assert np.array_equal(one.point(rows[0][:-1]), p)
        a.fold_rows(rows)
        b.fold_rows(rows)
        assert same_state(a.state(), b.state())
        ma, pb = a.maps(), a.point(a.best())
        for i, k in enumerate(("amp_best", "sigma_best", "snr_best")):
            assert np.array_equal(ma[k], pb[i], equal_nan=True), k
        for k, v in b.maps().items():
            assert np.array_equal(v, ma[k], equal_nan=True), k


def test_device_chain_equals_host_rows(lib_loaded):
    """fold(sampler, row_step, walker_step) of rows placed as a launch's device chain: the
    same bits as fold_rows of that subset, walker-major; once per launch."""
    W, nrec = 7, 41
    img, nsrc, base = case("c64")
    chain = scatter(base, W * nrec, 17).reshape(W, nrec, -1)
    with sampler("c64") as s, Detect(s) as dev, Detect(s) as host, Detect(s) as thin, \
            Detect(s) as thin_host:
        with pytest.raises(_lib.OlpeError) as e:
            dev.fold(s)                                   # nothing launched yet
        assert e.value.code == _lib.ESTATE
        s.seed(np.arange(1, W + 1))
        s.test_chain_set(chain)
        dev.fold(s)
        host.fold_rows(chain)
        assert dev.state()["n"] == W * nrec and same_state(dev.state(), host.state())
        thin.fold(s, row_step=3, walker_step=2)
        thin_host.fold_rows(chain[::2, ::3])
        assert same_state(thin.state(), thin_host.state())
        with pytest.raises(_lib.OlpeError) as e:
            dev.fold(s)                                   # the same launch twice
        assert e.value.code == _lib.ESTATE and "already folded" in str(e.value)
        for bad in ((0, 1), (1, 0)):
            with pytest.raises(_lib.OlpeError) as e:
                host.fold(s, *bad)
            assert e.value.code == _lib.EINVAL
    with sampler("c32") as small, sampler("c64") as s, Detect(s) as p:
        small.seed([1])
        small.test_chain_set(scatter(case("c32")[2], 3, 1).reshape(1, 3, -1))
        with pytest.raises(_lib.OlpeError) as e:
            p.fold(small)                                 # another side
        assert e.value.code == _lib.EINVAL and "side" in str(e.value)
        for bad in (0, 3, 8):
            with pytest.raises(_lib.OlpeError) as e:
                Detect(s, oversample=bad)
            assert e.value.code == _lib.EINVAL and "oversample" in str(e.value)


def test_unusable_rows(lib_loaded):
    """Rows with a NaN or inf parameter at block starts, ends and in runs change no bit of
    the state, and n_bad counts them; with no usable row finalize is ESTATE."""
    good = reference("c64").rows[:2 * B + 3]
    P = good.shape[1] - 1
    nan_row = np.full(P + 1, np.nan)
    inf_row = good[3].copy()
    inf_row[5] = np.inf
    rows, at = list(good), [0, B - 1, B, B + 1, 2 * B - 1, 2 * B, 300, 301]
    for i, k in enumerate(at):
        rows.insert(k, (nan_row, inf_row)[i % 2])
    rows = np.stack(rows + [nan_row, inf_row])
    with sampler("c64") as s, Detect(s) as a, Detect(s) as b, Detect(s) as c:
        a.fold_rows(rows)
        b.fold_rows(good)
        sa, sb = a.state(), b.state()
        assert sa["n"] == sb["n"] == 2 * B + 3 and sa["n_bad"] == len(at) + 2
        sb["n_bad"] = sa["n_bad"]
        assert same_state(sa, sb)
        assert a.scalars()["n_bad"] == len(at) + 2
        c.fold_rows(np.stack([nan_row, inf_row]))
        assert c.state()["n"] == 0 and c.state()["n_bad"] == 2
        with pytest.raises(_lib.OlpeError) as e:
            c.finalize()
        assert e.value.code == _lib.ESTATE and "no usable sample" in str(e.value)


def test_halves_merge_by_add(lib_loaded):
    """Two objects folded on B rows each and merged by add hold the bits of one object folded
    on all 2 B (a block's sums are added to the running ones as a whole, so pieces aligned to
    B merge exactly); add refuses another pivot; an empty object adopts the incoming one;
    reset empties."""
    ref = reference("c64_3")
    rows = ref.rows[:2 * B]
    pivot = rows[0]
    with sampler("c64_3") as s, Detect(s, pivot) as one, Detect(s, pivot) as a, \
            Detect(s, pivot) as b, Detect(s) as empty, Detect(s, rows[1]) as other:
        one.fold_rows(rows)
        a.fold_rows(rows[:B])
        b.fold_rows(rows[B:])
        a.add(b.state())
        assert same_state(a.state(), one.state())
        assert same_state(dt.merge_states(empty.state(), one.state()), one.state())
        other.fold_rows(rows[:3])
        with pytest.raises(_lib.OlpeError) as e:
            other.add(b.state())
        assert e.value.code == _lib.EINVAL and "pivot" in str(e.value)
        empty.add(one.state())
        assert same_state(empty.state(), one.state())
        whole = one.maps()
        for k, v in empty.maps().items():
            assert np.array_equal(v, whole[k], equal_nan=True), k
        check(whole, ref, 2 * B, "c64_3 merged")
        empty.reset()
        assert empty.state()["n"] == 0 and not empty.state()["sums"].any()
        with pytest.raises(_lib.OlpeError) as e:
            empty.finalize()
        assert e.value.code == _lib.ESTATE


def test_oversampled_lattice_holds_the_coarse_one(lib_loaded):
    """The even points of oversample 2 and every fourth of oversample 4 are the oversample-1
    lattice: the same operations on the same values."""
    rows = reference("s33").rows
    with sampler("s33") as s, Detect(s) as d1, Detect(s, oversample=2) as d2, \
            Detect(s, oversample=4) as d4:
        for d in (d1, d2, d4):
            d.fold_rows(rows)
        s1 = d1.state()["sums"]
        assert np.array_equal(d2.state()["sums"][:, ::2, ::2], s1)
        assert np.array_equal(d4.state()["sums"][:, ::4, ::4], s1)
        assert np.array_equal(d4.state()["sums"][:, ::2, ::2], d2.state()["sums"])
        p1 = d1.point(rows[5])
        assert np.array_equal(d2.point(rows[5])[:, ::2, ::2], p1)
        assert np.array_equal(d4.point(rows[5])[:, ::4, ::4], p1)
        assert d4.g == 129 and d2.maps()["snr_marg"].shape == (65, 65)


def test_a_masked_block(lib_loaded):
    """A saturated 5x5 patch is masked by the context; the planes at its centre are finite
    (the neighbours carry weight) and within the bounds there and around it."""
    img, truth = synth.make_image(33, 2, 0)
    img = img.copy()
    img[20:25, 6:11] = 3.0e4
    rows = scatter(np.append(truth, 0.0), B + 1, 77)
    fr = dr.Frame(img)
    assert fr.mask[20:25, 6:11].all()
    cand = [(22, 8), (20, 6), (24, 10), (22, 5), (19, 8), (22, 9), (0, 0), (16, 16)]
    ref = Ref(img, 2, rows, cand=cand)
    with Sampler(img, 1.0, 1, 1, 2, nsrc=2) as s, Detect(s) as d:
        d.fold_rows(rows)
        maps, sc = d.maps(), d.scalars()
        assert sc["pixels"] == int((~fr.mask).sum()) and sc["blind"] == 0
        assert all(np.isfinite(v).all() for v in maps.values())
        check(maps, ref, B + 1, "masked block")


def test_the_injection_frame_end_to_end(lib_loaded):
    """80 psi_truth injected at (15.7, 45.3) into the 64x64 2-source frame (seed 0), 257 rows
    about the truth: exactly one candidate outside the fitted sources, within one lattice step
    of the injection, its amplitude within 3 sigma_total of 80; the same frame without the
    injection gives none; the device's map of the truth agrees with the restatement's at
    the peak within the bounds (test_detect_cpu checks the restatement itself)."""
    pos, amp = (15.7, 45.3), 80.0
    for a in (amp, 0.0):
        img, p = dr.inject(64, a, pos, 0)
        rows = scatter(np.append(p, 0.0), B + 1, 4242)
        known, ex = dt.known_of(p, 2), dt.default_exclude_px(p, 2)
        with Sampler(img, 1.0, 1, 1, 2, nsrc=2) as s, Detect(s, pivot=p) as d:
            d.fold_rows(rows)
            m = d.maps()
            pt = d.point(p)
        c = dt.candidates(m["snr_marg"], m["amp_mean"], m["sigma_total"], known, 5.0, ex,
                          flux0=dt.flux0_of(p, 2), pixscale=9.952)
        free = [x for x in c if not x["flagged"]]
        for line in dt.table_lines({"samples": B + 1, "n_bad": 0, "blind": 0,
                                    "max_snr": float(np.nanmax(m["snr_marg"])),
                                    "max_snr_at": int(np.nanargmax(m["snr_marg"])),
                                    "min_snr": float(np.nanmin(m["snr_marg"])),
                                    "median_sigma": float(np.nanmedian(m["sigma_total"]))}, c):
            print(line)
        if a == 0.0:
            assert free == []
            continue
        assert len(free) == 1
        f = free[0]
        assert abs(f["x"] - pos[0]) <= 1 and abs(f["y"] - pos[1]) <= 1
        assert abs(f["amp"] - amp) <= 3 * f["sigma"]
        jy, jx = int(f["y"]), int(f["x"])
        ref = Ref(img, 2, np.append(p, 0.0)[None, :].copy(), cand=[(jy, jx), (46, 16), (45, 15)])
        check_point(pt, ref, 0, "injection, truth")


def test_cli_detect(tmp_path, lib_loaded, capsys):
    """apf_step3.py --detect on a small step-2 output: the npz, the three FITS files and the
    summary's entry; without the flag nothing changes."""
    d = tmp_path / "2014_test"
    path = synth.write_case(str(d), 33, 2)
    out = step2.main([path, "--walkers", "4", "--seed", "3", "--iters", "120", "--burn-in", "20",
                      "-q"])
    plain = step3.main([path, "sys", "-s", "4", "-q"])
    with open(out + "step3_summary.json", "rb") as f:
        before = f.read()
    assert "detect" not in plain and before == json.dumps(plain, indent=1).encode()
    capsys.readouterr()
    got = step3.main([path, "sys", "-s", "4", "--detect", "--detect-thin", "3",
                      "--detect-oversample", "2"])
    text = capsys.readouterr().out
    assert "Folding the companion detection map" in text and "contrast curve" in text
    chains = step3.load_chains(out, 4, 1)
    rows = chains[::3].reshape(-1, 17)
    z = dt.load_npz(out + "00001_detect.npz")
    assert int(z["scalar_samples"]) == rows.shape[0] and int(z["thin"]) == 3
    assert int(z["oversample"]) == 2 and z["snr_marg"].shape == (65, 65)
    assert np.array_equal(z["lattice"], np.arange(65) / 2.0)
    assert np.array_equal(z["best"], rows[int(np.nanargmin(rows[:, 16]))])
    theta = np.array([plain["parameters"][k]["mean"] for k in step3.NAMES_2[:-1]])
    assert np.array_equal(z["pivot"][:-1], theta) and np.array_equal(z["theta_hat"], theta)
    img, _ = fitsio.getdata_header(path)
    assert np.array_equal(z["mask"], dr.Frame(np.asarray(img)).mask)
    st = dt.state_of(z)
    again, _ = dt.planes_from_state(st, z["pivot_planes"])
    for k in KEYS:
        assert np.array_equal(again[k], z[k], equal_nan=True), k
    flux0 = dt.flux0_of(theta, 2)
    for suffix, want in (("snr", z["snr_marg"]), ("sigma", z["sigma_total"]),
                         ("contrast", 5.0 * z["sigma_total"] / flux0)):
        back, _ = fitsio.getdata_header(out + f"00001_{suffix}.fits")
        assert np.array_equal(np.asarray(back, dtype=np.float64), want, equal_nan=True), suffix
    curve = dt.contrast_curve(z["sigma_total"], dt.known_of(theta, 2)[0], flux0,
                              float(z["pixscale"]), oversample=2)
    assert np.array_equal(z["curve_contrast_median"], curve["contrast_median"])
    with open(out + "step3_summary.json") as f:
        saved = json.load(f)
    assert saved["detect"]["samples"] == rows.shape[0] and saved["detect"]["thin"] == 3
    assert saved["detect"]["oversample"] == 2
    assert saved["detect"]["curve"]["count"] == curve["count"].tolist()
    assert len(saved["detect"]["candidates"]) == z["candidates"].shape[0]
    assert got["detect"]["file"] == out + "00001_detect.npz"
    assert {k: v for k, v in saved.items() if k != "detect"} == json.loads(before)
