"""The false-alarm calibration on the device (olpe_detnull.hip, olpefit_amd/detect_null.py)
against the long-double restatement of tests/detnull_restatement.py at
detect_restatement.chosen's candidates, within the bound derived there (n^2 u covers any
order of a candidate's n^2 additions; the deviates within the project's gauss tolerance
3.2e-15).  Where the same operations run on the same values the comparison is
np.array_equal: batch sizes, split runs, a repeat after reset, maps() inside a larger run,
explicit frames that are the device's own noise, and the stats against map_stats on the
device's own maps.

Shapes: 32 (half a column tile idle), 33 (partial tiles both ways; oversample 1, 2, 4: the
phases), y33 with a masked block, 64 with 2 and 3 sources, 128 with 3 sources and R = 16 (two
column tiles).  R = 37 elsewhere: no multiple of a wave's 8 or a workgroup's 32 realisations.

The consistency test with ``Detect``: a frame D = M(theta) + err eps_r is built on the host
in float64 and handed to a sampler as float64 with the original frame's mask, Poisson term
and read noise, so the frame is exact (no float32 staging) and err is the original's in
every bit.  ``Detect.point(theta)[2]`` over it and ``maps(r)`` then estimate the same
number: both are within their own bounds of their long-double restatements, which differ by
what the host's D carries, w (2 u |D| + delta + 2 u err |eps|) per pixel through the filter
(the sum's and the product's roundings, the model tolerance, and (1 / err) err = 1 within a
rounding).
"""
import copy
import functools
import json

import numpy as np
import pytest

import detect_restatement as dr
import detnull_restatement as drn
from olpefit_amd import _lib, detect as dt, detect_null as dn, step2, step3, synth
from olpefit_amd.core import Sampler, noise_model
from olpefit_amd.detect import Detect
from olpefit_amd.detect_null import DetectNull
from oracle import olpe_oracle
from test_gpu_predictive import case

pytestmark = pytest.mark.gpu
LD = np.longdouble
SEED = 20240
MAP_CASES = [("c32", 1, 37, False), ("s33", 1, 37, False), ("s33", 2, 37, True),
             ("s33", 4, 37, False), ("y33", 1, 37, False), ("c64", 1, 37, False),
             ("c64_3", 1, 37, False), ("c128_3", 1, 16, False)]


@functools.lru_cache(maxsize=None)
def image(name):
    """case(name)'s image; y33 with a block of saturated pixels."""
    img, nsrc, base = case(name)
    if name == "y33":
        img = img.copy()
        img[20:25, 6:11] = 3.0e4
    return img, nsrc, np.array(base[:-1])


def scale_of(g):
    return 0.5 + np.random.RandomState(9).uniform(size=(g, g))


def objects(name, oversample=1, **kw):
    img, nsrc, vec = image(name)
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    d = Detect(s, oversample=oversample)
    return s, d, DetectNull(d, vec, **kw)


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in dn.FIELDS)


@pytest.mark.parametrize("name, oversample, R, scaled", MAP_CASES)
def test_maps_against_the_restatement(lib_loaded, name, oversample, R, scaled):
    img, nsrc, vec = image(name)
    fr = dr.Frame(img)
    g = dt.lattice_side(fr.n, oversample)
    scale = scale_of(g) if scaled else None
    s, d, h = objects(name, oversample, scale=scale, seed=SEED)
    with s, d, h:
        maps = h.maps(0, R)
    if name == "y33":
        assert fr.mask[20:25, 6:11].all()
    cand = dr.chosen(fr.n, nsrc, vec, fr.mask, oversample)
    with np.errstate(all="ignore"):
        ref = drn.maps_at(fr, vec, nsrc, cand, dn.noise_frames(SEED, 0, R, fr.n), oversample, scale)
    got = maps[:, cand[:, 0], cand[:, 1]]
    blind = np.isnan(ref["snr"].astype(np.float64))
    assert np.array_equal(np.isnan(got), blind)
    ok = ~blind
    diff = np.abs(got.astype(LD) - ref["snr"]).astype(np.float64)
    ratio = float((diff[ok] / ref["bsnr"][ok]).max())
    print(f"{name} os {oversample} R {R}: worst {ratio:.3e} x bound, max |snr| "
          f"{np.nanmax(np.abs(maps)):.2f}, relative bound up to "
          f"{float((ref['bsnr'][ok] / np.maximum(np.abs(got[ok]), 1e-3)).max()):.2e}")
    assert np.all(diff[ok] <= ref["bsnr"][ok])
    # a null map is a map of unit-variance deviates
    assert 0.5 < np.nanstd(maps / (1.0 if scale is None else scale)) < 1.5


@pytest.mark.parametrize("seed", [0, 2 ** 32 - 1, 12345])
def test_noise_is_randomstate(lib_loaded, seed):
    """5 realisations at n = 33: 1089 deviates, so a frame ends mid-pair with a deviate
    cached and discarded; seed 2^32 - 1 wraps to 0 at realisation 1.  The tolerance is
    test_gpu_parity's for the sampler's gauss; a wrong accept would shift every later
    value."""
    s, d, h = objects("s33", seed=seed)
    with s, d, h:
        got = h.noise(0, 5)
        tail = h.noise(3, 2)
    want = dn.noise_frames(seed, 0, 5, 33)
    assert got.shape == want.shape == (5, 33, 33)
    assert np.array_equal(got == 0.0, want == 0.0) and np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=3.2e-15, atol=0.0)
    assert np.array_equal(tail, got[3:])
    print("seed", seed, "worst relative difference", float(np.max(np.abs(got / want - 1.0))))


def test_batches_splits_resets_and_frames_give_the_same_bits(lib_loaded):
    R = 37
    s, d, ref = objects("s33", 2, seed=SEED, threshold=2.0)
    with s, d, ref:
        ref.run(R)
        want = ref.results()
        assert want["done"] == R and want["ranges"].tolist() == [[SEED, 0, R]]
        maps = ref.maps(0, R)
        vec = image("s33")[2]
        for batch in (5, 16, 37):
            with DetectNull(d, vec, seed=SEED, threshold=2.0, batch=batch) as h:
                h.run(R)
                assert same(h.results(), want), batch
                assert np.array_equal(h.maps(0, R), maps, equal_nan=True), batch
        with DetectNull(d, vec, seed=SEED, threshold=2.0, batch=16) as h:
            h.run(20)
            assert h.results()["done"] == 20
            h.run(17)
            got = h.results()
            assert same(got, want) and got["ranges"].tolist() == [[SEED, 0, R]]
            # maps of realisations inside the run, across a batch boundary; nothing is disturbed
            assert np.array_equal(h.maps(11, 9), maps[11:20], equal_nan=True)
            assert same(h.results(), want)
            h.reset()
            assert h.results()["done"] == 0
            h.run(R)
            assert same(h.results(), want)
            # explicit frames: the device's own deviates, so the weight kernel sees the same bits
            eps = h.noise(0, R)
            h.reset()
            h.run_frames(eps)
            got = h.results()
            assert got["frames"] and same(got, want)
        # another seed is another set of frames
        with DetectNull(d, vec, seed=SEED + 1, threshold=2.0) as h:
            h.run(2)
            r1 = h.results()
            assert np.array_equal(r1["max_all"][:1], want["max_all"][1:2])
            assert not np.array_equal(r1["max_all"], want["max_all"][:2])


@pytest.mark.parametrize("name, oversample", [("y33", 1), ("s33", 4), ("c64_3", 1)])
def test_stats_are_map_stats_of_the_device_maps(lib_loaded, name, oversample):
    """results() against map_stats on the device's own maps, field by field, exactly;
    threshold 2.0 so that peaks exist, a centre off the lattice and bin_px 0.75."""
    R = 37
    img, nsrc, vec = image(name)
    known = dt.known_of(vec, nsrc)
    kw = dict(known=known, exclude_px=3.3, centre=(known[0][0] + 0.3, known[0][1] - 0.2),
              bin_px=0.75, threshold=2.0)
    s, d, h = objects(name, oversample, seed=SEED, **kw)
    with s, d, h:
        h.run(R)
        res, maps = h.results(), h.maps(0, R)
    assert res["peaks_all"].sum() > R and res["peaks_out"].sum() > 0
    assert np.any(res["peaks_out"] < res["peaks_all"])
    for r in range(R):
        want = dn.map_stats(maps[r], oversample=oversample, **kw)
        for k in dn.FIELDS:
            assert np.array_equal(res[k][r], want[k], equal_nan=True), (r, k)
    assert res["ring_max"].shape[1] == dn.rings(d.g, kw["centre"], 0.75, oversample).max() + 1


def test_consistency_with_detect(lib_loaded):
    """See the module docstring: Detect.point over the frame M(theta) + err eps_r against
    maps(r), within the sum of both bounds and what the host's frame carries."""
    name, r = "c64", 3
    img, nsrc, vec = image(name)
    fr = dr.Frame(img)
    n = fr.n
    mask, pois2, rn2, _, _ = noise_model(img, 1.0, 1, 1, 2)
    M = olpe_oracle.build_analytical_model(np.append(vec, 0.0), n, nsrc, 0)
    eps = dn.noise_frames(SEED, r, 1, n)[0]
    D = M + fr.err * eps
    D[fr.mask] = img[fr.mask]
    s, d, h = objects(name, seed=SEED)
    with s, d, h:
        null_map = h.maps(r, 1)[0]
    with Sampler(D, 1.0, 1, 1, 2, nsrc=nsrc, mask=mask, pois2=pois2.astype(np.float64),
                 readnoise2=rn2) as s2, Detect(s2) as d2:
        snr = d2.point(vec)[2]
    cand = dr.chosen(n, nsrc, vec, fr.mask)
    fr2 = copy.copy(fr)
    fr2.D = D
    with np.errstate(all="ignore"):
        a = drn.maps_at(fr, vec, nsrc, cand, eps[None], 1)
        b = dr.sample(fr2, np.append(vec, 0.0), nsrc, cand)
        delta = 1e-13 * float(np.abs(M).max())
        T = np.abs(dr.table(vec, nsrc, n)[0]).astype(np.float64)
        # D = fl(M + fl(err eps)): the sum's and the product's roundings, and (1 / err) err = 1
        # within a rounding, per pixel through the filter
        per = fr.wf * (2 * dr.U * np.abs(D) + delta + 2 * dr.U * fr.err * np.abs(eps))
        per[fr.mask] = 0.0
        carried = np.array([float((per * T[n - 1 - cy:2 * n - 1 - cy,
                                           n - 1 - cx:2 * n - 1 - cx]).sum())
                            for cy, cx in cand]) / np.sqrt(b["Q"].astype(np.float64))
    got_a, got_b = null_map[cand[:, 0], cand[:, 1]], snr[cand[:, 0], cand[:, 1]]
    bound = a["bsnr"][0] + b["bsnr"] + carried
    diff = np.abs(got_a - got_b)
    print("consistency: worst", float((diff / bound).max()), "x bound; relative",
          float((diff / np.abs(got_a)).max()))
    assert np.all(diff <= bound)
    # and the two long-double statements themselves agree to what the frame carries
    assert np.all(np.abs(a["snr"][0] - b["snr"]).astype(np.float64) <= carried)


def test_cli_detect_null(tmp_path, lib_loaded, capsys):
    """apf_step3.py --detect --detect-null 64 on the c32 frame: the npz's arrays, the
    summary's keys and the printed lines; without the flag the output is the existing run's."""
    d = tmp_path / "2014_test"
    path = synth.write_case(str(d), 32, 2)          # the c32 fixture's frame (seed 0)
    assert np.array_equal(synth.make_image(32, 2, 0)[0], case("c32")[0])
    out = step2.main([path, "--walkers", "4", "--seed", "3", "--iters", "120", "--burn-in", "20",
                      "-q"])
    base = ["sys", "-s", "4", "--detect", "--detect-thin", "3", "--detect-threshold", "3"]
    plain = step3.main([path] + base)
    text0 = capsys.readouterr().out
    with open(out + "step3_summary.json", "rb") as f:
        before = f.read()
    npz0 = dt.load_npz(out + "00001_detect.npz")
    assert "detect_null" not in plain["detect"] and "null maps" not in text0
    got = step3.main([path] + base + ["--detect-null", "64", "--detect-null-seed", "5"])
    text = capsys.readouterr().out
    assert text.startswith(text0) and "null maps" in text and "64 realisations" in text
    for words in ("map maximum", "false per map", "per-map FAP", "calibrated curve"):
        assert words in text[len(text0):], words
    npz1 = dt.load_npz(out + "00001_detect.npz")
    assert sorted(npz1) == sorted(npz0)
    assert all(np.array_equal(npz1[k], npz0[k], equal_nan=True) for k in npz0)
    z = dt.load_npz(out + "00001_detect_null.npz")
    g = 32
    assert int(z["done"]) == 64 and z["ranges"].tolist() == [[5, 0, 64]]
    assert z["max_all"].shape == z["max_out"].shape == z["peaks_all"].shape == (64,)
    assert z["ring_max"].shape[0] == 64 and z["scale"].shape == (g, g)
    assert np.all(z["max_out"] <= z["max_all"]) and np.all(z["max_all"] > 0.0)
    assert z["ring_k"].shape == (z["ring_max"].shape[1],) and np.isnan(z["ring_k"]).all()
    nul = got["detect"]["detect_null"]
    assert nul["realisations"] == 64 and nul["seed"] == 5 and nul["p"] == 0.01
    for k in ("max_all_median", "max_all_q90", "max_all_q99", "max_out_median",
              "false_per_map_all", "false_per_map_out", "candidate_fap", "curve_k", "file"):
        assert k in nul, k
    assert len(nul["candidate_fap"]) == len(got["detect"]["candidates"])
    with open(out + "step3_summary.json") as f:
        saved = json.load(f)
    assert saved["detect"]["detect_null"]["realisations"] == 64
    rest = {k: v for k, v in saved["detect"].items() if k != "detect_null"}
    assert rest == json.loads(before)["detect"]
    assert {k: v for k, v in saved.items() if k != "detect"} == \
        {k: v for k, v in json.loads(before).items() if k != "detect"}
    with pytest.raises(SystemExit):
        step3.main([path, "sys", "-s", "4", "--detect-null", "8"])
    capsys.readouterr()


def test_argument_errors(lib_loaded):
    """Refused before any GPU call: NULL, a non-finite vector, a scale that is not finite and
    positive, negative counts, and generated against explicit use within one object."""
    import ctypes as C
    lib = lib_loaded
    s, d, h = objects("c32", seed=1)
    img, nsrc, vec = image("c32")
    with s, d, h:
        out = C.c_void_p()
        ctr = np.zeros(2)
        pd = lambda a: a.ctypes.data_as(_lib._pd)   # noqa: E731
        args = (None, 0, 1.0, pd(ctr), 1.0, 5.0, 0, 0, C.byref(out))
        assert lib.olpe_detect_null_create(None, pd(vec), None, *args) == _lib.EINVAL
        assert lib.olpe_detect_null_create(d._h, None, None, *args) == _lib.EINVAL
        assert lib.olpe_detect_null_create(d._h, pd(vec), None, None, 0, 1.0, None, 1.0, 5.0, 0,
                                           0, C.byref(out)) == _lib.EINVAL
        assert lib.olpe_detect_null_create(d._h, pd(vec), None, None, 0, 1.0, pd(ctr), 1.0, 5.0,
                                           0, 0, None) == _lib.EINVAL
        for k, bad in ((0, np.nan), (3, np.inf)):
            v = vec.copy()
            v[k] = bad
            with pytest.raises(_lib.OlpeError) as e:
                DetectNull(d, v)
            assert e.value.code == _lib.EINVAL and "non-finite" in str(e.value)
        for bad in (0.0, -1.0, np.nan, np.inf):
            sc = np.ones((d.g, d.g))
            sc[3, 4] = bad
            with pytest.raises(_lib.OlpeError) as e:
                DetectNull(d, vec, scale=sc)
            assert e.value.code == _lib.EINVAL and "scale" in str(e.value)
        for kw in (dict(bin_px=0.0), dict(bin_px=1e-3), dict(exclude_px=-1.0),
                   dict(threshold=np.nan), dict(batch=-1), dict(centre=(np.nan, 0.0))):
            with pytest.raises(_lib.OlpeError) as e:
                DetectNull(d, vec, **kw)
            assert e.value.code == _lib.EINVAL, kw
        assert not out.value
        assert lib.olpe_detect_null_maps(h._h, 0, -1, None) == _lib.EINVAL
        assert lib.olpe_detect_null_noise(h._h, 0, 1, None) == _lib.EINVAL
        for call in (lambda: h.run(-1), lambda: h.maps(-1, 1), lambda: h.noise(-1, 1)):
            with pytest.raises(_lib.OlpeError) as e:
                call()
            assert e.value.code == _lib.EINVAL
        assert lib.olpe_detect_null_run(None, 1) == _lib.EINVAL
        assert lib.olpe_detect_null_run_frames(h._h, None, 1) == _lib.EINVAL
        assert lib.olpe_detect_null_get(None, None, None, None, None, None, None, None, None,
                                        None) == _lib.EINVAL
        with pytest.raises(ValueError):
            h.run_frames(np.zeros((2, 31, 32)))
        h.run(3)
        with pytest.raises(_lib.OlpeError) as e:
            h.run_frames(np.zeros((1, 32, 32)))
        assert e.value.code == _lib.ESTATE and "generated" in str(e.value)
        assert h.results()["done"] == 3
        h.reset()
        h.run_frames(np.ones((2, 32, 32)))
        for call in (lambda: h.run(1), lambda: h.maps(0, 1), lambda: h.noise(0, 1)):
            with pytest.raises(_lib.OlpeError) as e:
                call()
            assert e.value.code == _lib.ESTATE and "explicit" in str(e.value)
        assert h.results()["done"] == 2
