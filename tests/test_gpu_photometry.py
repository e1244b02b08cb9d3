"""Photometry posteriors on the GPU (olpe_phot_*, olpefit_amd/photometry.py) against a NumPy
restatement in the operation order olpe_phot.hip states.

* Per-sample planes: everything but ``dmag`` is exact IEEE arithmetic and equals NumPy bit
  for bit.  ``dmag = -2.5 * log10(ratio)`` goes through the device library's log10; the
  largest difference from NumPy's measured on this file's inputs is 1 ulp (DMAG_ULP_MEASURED;
  DESIGN.md 7f) and the bound is four times that.
* Order statistics: bit-equal to the sorted valid samples (the radix select is exact).  The
  select's and the reductions' workgroups hold 256 threads (kSelThreads of olpe_select.h,
  kThreads of olpe_phot.hip), so the sizes around a block are 255 / 256 / 257; a reduction
  block covers 4096 samples (kChunk), so 4095 / 4096 / 4097 are here too.  The select's grid
  is 1024 such blocks and stage 2 of the reductions has 256 threads: 262,144, 262,145, 600,001
  and 1,048,577 values (tests/fold_scale_cases.py) go past both.
* Percentiles: ``np.nanpercentile`` to rtol 4e-16.  Mean and np.std: a np.longdouble
  restatement under the worst-case bound n * 2^-53 * max|x| of any summation order; the
  largest errors observed on this file's inputs were 4e-5 of that bound (mean) and 9e-4 (std).
* fold(sampler) against fold_rows of the same launch: bit-identical.
"""
import functools
import json
import os

import numpy as np
import pytest

import fold_scale_cases as fc
from olpefit_amd import _lib, fitsio, step2, step3, synth
from olpefit_amd.astrometry import header_scalars, py2_str
from olpefit_amd.photometry import (PLANES, Photometry, aperture_snr, reference_fwhm,
                                    reference_numbers)

pytestmark = pytest.mark.gpu

PIXSCALE = 9.952
DMAG_ULP_MEASURED = 1.0           # the largest |device - NumPy| of dmag on PLANE_CHAINS, in ulp
DMAG_ULP = 4 * DMAG_ULP_MEASURED
PROBS = np.array([0, 16, 50, 84, 100]) / 100     # what np.percentile makes of its q


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def columns(variant):
    """(first amplitude column, sources): the A_k, then q, b, sx, sy, sx2, sy2 follow."""
    return (6, 2) if variant == 2 else (8, 3)


def restate(chain, variant, pixscale):
    """The planes of chain [rows, walkers, PS] in olpe_phot.hip's operation order, and the
    number of unusable rows."""
    c0, ns = columns(variant)
    A = [chain[:, :, c0 + k] for k in range(ns)]
    q, b = chain[:, :, c0 + ns], chain[:, :, c0 + ns + 1]
    sx, sy, sx2, sy2 = (chain[:, :, c0 + ns + 2 + i] for i in range(4))
    nan = np.float64("nan")
    with np.errstate(all="ignore"):
        ok = np.isfinite(np.stack(A + [q, b, sx, sy, sx2, sy2])).all(axis=0)
        d0 = A[0] - b
        ok &= (d0 > 0) & (sx > 0) & (sy > 0) & (sx2 > 0) & (sy2 > 0)
        planes = []
        for k in range(1, ns):
            dk = A[k] - b
            ratio = dk / d0
            planes += [ratio, np.where(dk > 0, -2.5 * np.log10(ratio), nan)]
        c1 = ((1.0 - q) * sx) * sy
        c2 = (q * sx2) * sy2
        tot = c1 + c2
        planes += [((2.0 * np.pi) * d0) * tot,
                   (2.355 * np.maximum(sx, sy)) * pixscale,
                   (2.355 * np.minimum(sx, sy)) * pixscale,
                   (2.355 * np.maximum(sx2, sy2)) * pixscale,
                   c1 / tot]
    return [np.where(ok, p, nan) for p in planes], int((~ok).sum())


def plane_chain(variant):
    """3 walkers x 37 rows with every kind of row the kernel tells apart."""
    ps = 17 if variant == 2 else 20
    c0, ns = columns(variant)
    rng = np.random.RandomState(40 + variant)
    c = rng.normal(size=(37, 3, ps)) * 3.0 + 50.0
    c[:, :, c0] = 3.0e4 + 500.0 * rng.normal(size=(37, 3))
    for k in range(1, ns):
        c[:, :, c0 + k] = 2.0e3 / k + 60.0 * rng.normal(size=(37, 3))
    c[:, :, c0 + ns] = 0.2 + 0.02 * rng.normal(size=(37, 3))
    c[:, :, c0 + ns + 1] = 30.0 + rng.normal(size=(37, 3))
    for i, s0 in enumerate((1.5, 1.5, 4.5, 4.5)):          # sx > sy and sx < sy both occur
        c[:, :, c0 + ns + 2 + i] = s0 + 0.2 * rng.normal(size=(37, 3))
    b = c0 + ns + 1
    c[0] = np.nan                                           # the chain files' seed row
    c[5, 1, c0] = c[5, 1, b] - 1.0                          # A_0 - b < 0
    c[6, 0, c0 + 1] = c[6, 0, b] - 2.0                      # A_1 - b < 0: ratio kept, dmag NaN
    c[7, 2, c0 + ns - 1] = c[7, 2, b]                       # A_k - b = 0: ratio 0, dmag NaN
    c[8, 2, c0 + ns + 2] = 0.0                              # a zero width
    c[9, 0, c0 + ns + 5] = np.inf                           # a non-finite width
    c[10, 1, 0] = np.nan                                    # a column no plane reads
    for r in (12, 13, 20, 36):                              # rejected proposals repeat the row
        c[r] = c[r - 1]
    return c


PLANE_CHAINS = {v: plane_chain(v) for v in (2, 3)}


@pytest.mark.parametrize("variant", [2, 3])
def test_planes_match_numpy(lib_loaded, variant):
    chain = PLANE_CHAINS[variant]
    ref, bad = restate(chain, variant, PIXSCALE)
    assert bad == 6
    sx, sy = chain[1:, :, columns(variant)[0] + variant + 2], \
        chain[1:, :, columns(variant)[0] + variant + 3]
    assert (sx > sy).any() and (sx < sy).any()
    with Photometry(3, 37, variant=variant, pixscale=PIXSCALE) as p, \
            Photometry(3, 40, variant=variant, pixscale=PIXSCALE) as s:
        p.fold_rows(chain)
        for lo, hi in ((0, 1), (1, 9), (9, 37)):            # the same rows in three folds
            s.fold_rows(chain[lo:hi])
        assert p.unusable == bad and s.unusable == bad and p.rows == s.rows == 37
        assert p.planes == PLANES[variant] and len(ref) == len(p.planes)
        worst = 0.0
        for name, want in zip(p.planes, ref):
            got = p.samples(name)
            assert got.shape == (37, 3)
            assert np.array_equal(bits(got), bits(s.samples(name))), name
            assert np.array_equal(np.isnan(got), np.isnan(want)), name
            m = ~np.isnan(want)
            if name.startswith("dmag"):
                ulp = np.max(np.abs(got[m] - want[m]) / np.spacing(np.abs(want[m])))
                print(f"variant {variant} {name}: max |device - NumPy| = {ulp:.2f} ulp")
                worst = max(worst, ulp)
            else:
                assert np.array_equal(bits(got[m]), bits(want[m])), name
        assert worst <= DMAG_ULP, worst
        # the ratio of a companion at or below the offset is kept
        k = p.planes.index(PLANES[variant][0])
        assert p.samples(k)[6, 0] < 0 and np.isnan(p.samples(k + 1)[6, 0])
        assert json.dumps(p.finalize(), sort_keys=True) == json.dumps(s.finalize(), sort_keys=True)


def ratio_chain(values, W, variant=2):
    """Rows whose flux_ratio (of the first companion) plane holds ``values`` exactly (A_0 = 1,
    b = 0: ratio = A_1 / 1), padded with NaN rows to a multiple of W walkers."""
    ps = 17 if variant == 2 else 20
    c0, ns = columns(variant)
    v = np.asarray(values, dtype=np.float64)
    rows = max(1, -(-v.size // W))
    flat = np.full(rows * W, np.nan)
    flat[:v.size] = v
    c = np.ones((rows, W, ps))
    c[:, :, c0 + ns] = 0.5
    c[:, :, c0 + ns + 1] = 0.0
    c[:, :, c0 + 1] = flat.reshape(rows, W)
    return c


def total_order(x):
    """The valid samples in IEEE total order: as np.sort, with -0.0 before +0.0 (np.sort
    leaves the order of equal elements open)."""
    x = x[~np.isnan(x)]
    return x[np.lexsort((~np.signbit(x), x))]


def select_cases():
    rng = np.random.RandomState(9)
    ties = np.concatenate([rng.randint(-20, 30, size=60000) / 7.0, rng.normal(size=10070),
                           [0.0, -0.0] * 4])
    rng.shuffle(ties)
    signs = np.concatenate([rng.normal(size=300) * 1e3, [-0.0, 0.0, -0.0, 5e-324, -5e-324,
                                                          1e150, -1e150]])
    rng.shuffle(signs)
    cases = {"n1": (np.array([3.25]), 1), "n2": (np.array([2.0, -1.0]), 1),
             "n2_w2": (np.array([2.0, -1.0]), 2), "ties70k": (ties, 70),
             "repeated": (np.full(1000, 0.1), 8), "signs": (signs, 5)}
    for n in (255, 256, 257, 4095, 4096, 4097):
        cases[f"n{n}"] = (rng.normal(size=n) * rng.choice([1.0, 1e-3, 1e3], size=n), 7)
    return cases


SELECT_CASES = select_cases()


@pytest.mark.parametrize("case", list(SELECT_CASES))
def test_order_statistics_and_moments(lib_loaded, case):
    values, W = SELECT_CASES[case]
    check_order_statistics(values, W, case)


def check_order_statistics(values, W, case):
    """The checks of test_order_statistics_and_moments; returns every plane's summary."""
    chain = ratio_chain(values, W)
    with Photometry(W, chain.shape[0], pixscale=PIXSCALE) as p:
        p.fold_rows(chain)
        every = p.finalize(PROBS)
        res = every["flux_ratio"]
        x = p.samples("flux_ratio").ravel()
    n = values.size
    assert np.array_equal(bits(x[:n]), bits(values)) and np.isnan(x[n:]).all()
    srt = total_order(x)
    assert res["n"] == n == srt.size
    assert bits(res["min"]) == bits(srt[0]) and bits(res["max"]) == bits(srt[-1])
    for (lo, hi), q in zip(res["brackets"], PROBS):
        vi = (n - 1) * q
        assert bits(lo) == bits(srt[int(np.floor(vi))]), (case, q)
        assert bits(hi) == bits(srt[int(np.ceil(vi))]), (case, q)
    np.testing.assert_allclose(res["percentiles"], np.nanpercentile(x, 100 * PROBS),
                               rtol=4e-16, atol=0)
    xl = srt.astype(np.longdouble)
    mean = xl.sum() / n
    std = np.sqrt(((xl - mean) ** 2).sum() / n)
    bound = n * 2.0 ** -53 * np.max(np.abs(srt))
    em, es = abs(res["mean"] - mean), abs(res["std"] - std)
    print(f"{case}: n {n} passes {res['passes']} mean err {float(em):.3e} std err "
          f"{float(es):.3e} bound {bound:.3e}")
    assert em <= bound and es <= bound
    if case == "repeated":
        assert res["std"] == 0.0 and res["mean"] == 0.1 and res["percentiles"] == [0.1] * 5
    # ranks share the select's passes: far fewer reads than one descent per rank (6 digits
    # of 11 bits at the most, for 5 ranks and their upper neighbours)
    if bits(srt[0]) != bits(srt[-1]):
        assert 0 < res["passes"] <= 1 + 5 * 5 + 5
    else:
        assert res["passes"] == 0                  # one value: nothing to select
    return every


@functools.lru_cache(maxsize=None)
def scale_values(n):
    """n values after the ties70k and signs recipes: half of them multiples of 1 / 7 (50
    distinct values: ranks share bins down to the last digit), the rest a normal sample scaled
    by 1, 1e-3 or 1e3, and +-0.0, +-5e-324, +-1e150: the keys differ from the first bit, so the
    descent has all six digits to go."""
    rng = np.random.RandomState(n % 100003)
    special = [0.0, -0.0] * 4 + [5e-324, -5e-324, 1e150, -1e150]
    m = n - n // 2 - len(special)
    v = np.concatenate([rng.randint(-20, 30, size=n // 2) / 7.0,
                        rng.normal(size=m) * rng.choice([1.0, 1e-3, 1e3], size=m), special])
    rng.shuffle(v)
    assert v.size == n
    v.setflags(write=False)
    return v


@pytest.mark.parametrize("case", list(fc.PHOT))
def test_order_statistics_past_the_grid_caps(lib_loaded, case):
    """Sample counts past the caps (tests/fold_scale_cases.py): the select's 1024 x 256 threads
    make no second trip of their grid-stride loops at 262,144 samples, one (one block) at
    262,145 + padding, a third for part of the grid at 600,001; 1,048,577 values in rows of
    1024 walkers are 257 stage-1 partials for the 256 threads of phot_reduce_stage2.  The
    checks are test_order_statistics_and_moments'.  With +-1e150 among the values the bound on
    the mean says little; the core_fraction plane of the same rows is 0.5 in every usable
    sample, whose sums are exact in any order: n, mean 0.5 and std 0 exactly, which a dropped
    or doubled partial would miss."""
    n, W = fc.PHOT[case]
    every = check_order_statistics(scale_values(n), W, case)
    core = every["core_fraction"]
    assert (core["n"], core["mean"], core["std"]) == (n, 0.5, 0.0)
    assert core["min"] == core["max"] == 0.5 and core["passes"] == 0


def test_a_plane_without_numbers(lib_loaded):
    # every companion at or below the offset: ratios kept, no dmag; then no usable row at all
    chain = ratio_chain(-np.arange(1.0, 21.0), 4)
    with Photometry(4, 10, pixscale=PIXSCALE) as p:
        p.fold_rows(chain)
        res = p.finalize()
        assert res["flux_ratio"]["n"] == 20 and p.unusable == 0
        d = res["dmag"]
        assert d["n"] == 0 and d["passes"] == 0
        assert all(np.isnan(d[k]) for k in ("mean", "std", "min", "max"))
        assert all(np.isnan(v) for v in d["percentiles"]) and len(d["percentiles"]) == 3
        assert np.isnan(p.samples("dmag")).all()
        p.reset()
        assert p.rows == 0 and p.unusable == 0
        with pytest.raises(_lib.OlpeError) as e:
            p.finalize()                                   # nothing folded
        assert e.value.code == _lib.ESTATE
        p.fold_rows(np.full((3, 4, 17), np.nan))
        res = p.finalize((0.5,))
        assert p.unusable == 12
        assert all(r["n"] == 0 and np.isnan(r["percentiles"][0]) for r in res.values())


def test_device_fold_equals_host_fold(golden, lib_loaded):
    """fold(sampler) reads the launch's device chain [W][nrec][PS] in place; fold_rows the
    same rows from the host, collated [rows][W][PS]: bit-identical samples and summary."""
    from olpefit_amd.core import Sampler
    g = golden("c32")
    smp = Sampler(g["image"], 1.0, 1, 1, 2, nsrc=2)
    smp.seed([1, 2, 3, 4])
    smp.set_state(g["p_init"])
    chain = smp.run(200, burn_in=0, record_stride=1)
    assert chain.shape == (4, 200, 17)
    rows = np.ascontiguousarray(np.transpose(chain, (1, 0, 2)))
    with Photometry(4, 200, pixscale=PIXSCALE) as a, Photometry(4, 200, pixscale=PIXSCALE) as b:
        for step in (1, 3):
            a.fold(smp, row_step=step)
            with pytest.raises(_lib.OlpeError) as e:     # the same launch twice
                a.fold(smp, row_step=step)
            assert e.value.code == _lib.ESTATE and "already folded" in str(e.value)
            b.fold_rows(rows[::step])
            assert a.rows == b.rows == len(range(0, 200, step))
            for name in a.planes:
                assert np.array_equal(bits(a.samples(name)), bits(b.samples(name))), (step, name)
            ra, rb = a.finalize(), b.finalize()
            assert json.dumps(ra, sort_keys=True) == json.dumps(rb, sort_keys=True)
            assert ra["flux_ratio"]["n"] > 0
            a.reset()                                    # allows the launch again
            b.reset()
    # a full store: refused, and what the object holds still finalizes
    with Photometry(4, 150, pixscale=PIXSCALE) as a:
        a.fold_rows(rows[:100])
        before = a.finalize()
        with pytest.raises(_lib.OlpeError) as e:
            a.fold(smp)                                  # 100 + 200 rows into 150
        assert e.value.code == _lib.ESTATE and "store full" in str(e.value)
        with pytest.raises(_lib.OlpeError) as e:
            a.fold_rows(rows[:51])
        assert e.value.code == _lib.ESTATE and "store full" in str(e.value)
        assert a.rows == 100
        assert json.dumps(a.finalize(), sort_keys=True) == json.dumps(before, sort_keys=True)
        a.fold(smp, row_step=4)                          # 50 more rows fit
        assert a.rows == 150
    with pytest.raises(_lib.OlpeError) as e:
        with Photometry(5, 10, pixscale=PIXSCALE) as a:
            a.fold(smp)                                  # another walker count
    assert e.value.code == _lib.EINVAL
    smp.close()


HEADER = {"KOAID": "N2.20250127.00001.fits", "PARANG": 12.5, "ROTPPOSN": 100.25,
          "INSTANGL": 0.7, "EL": 55.0, "AZ": 200.0, "ROTMODE": "position angle",
          "PARANTEL": -20.0, "ITIME": 1.0, "COADDS": 1, "MULTISAM": 1, "SAMPMODE": 2}


def test_cli_photometry_fills_the_pasep_line(tmp_path, lib_loaded):
    """apf_step3 --astrometry --photometry on a small step-2 output: the npz, the summary
    entry, and a pasep line whose S/N and FWHM fields are the host functions' values;
    without --photometry the fields stay nan."""
    d = tmp_path / "2014_test"
    path = synth.write_case(str(d), 64, 2)
    img, _ = synth.make_image(64, 2, 0)
    fitsio.write(path, img, {**synth.HEADER, **HEADER})
    out = step2.main([path, "--walkers", "4", "--seed", "3", "--iters", "120", "--burn-in", "20",
                      "-q"])
    step3.main([path, "sys", "-s", "4", "-q", "--astrometry"])
    got = step3.main([path, "sys", "-s", "4", "-q", "--astrometry", "--photometry",
                      "--photometry-thin", "2"])
    with open(str(d) + "/epoch_grand_pasep") as f:
        lines = [ln.split(" , ") for ln in f.read().splitlines()]
    assert len(lines) == 2 and len(lines[0]) == len(lines[1]) == 11
    assert lines[0][5:9] == ["nan"] * 4
    assert lines[0][:5] + lines[0][9:] == lines[1][:5] + lines[1][9:]
    chains = step3.load_chains(out, 4, 1)
    image, hdr = fitsio.getdata_header(path)
    pixscale = header_scalars(hdr, "pre")["pixscale"]
    ref = reference_numbers(image, chains, pixscale, 2)
    want = ref["snr"] + [ref["fwhm_mean"], ref["fwhm_std"]]
    assert all(np.isfinite(v) for v in want)
    assert lines[1][5:9] == [py2_str(v) for v in want]
    (sx, sy), (cx, cy) = ref["positions"]
    assert want[0] == aperture_snr(image, sx, sy) and want[1] == aperture_snr(image, cx, cy)
    assert want[2:] == list(reference_fwhm(chains[:, :, 10], pixscale))
    # (the companion's annulus reaches the star's wings on this frame, so its S/N by the
    # reference's recipe is finite but not positive: only the star's is a detection)
    assert want[0] > 10.0
    ph = got["photometry"]
    assert ph["thin"] == 2 and ph["rows"] == len(chains[::2]) and ph["pixscale"] == pixscale
    assert ph["unusable"] == 0 and ph["reference"]["snr"] == ref["snr"]
    planes, _ = restate(chains[::2], 2, pixscale)
    for name, x in zip(PLANES[2], planes):
        e = ph["planes"][name]
        assert e["n"] == np.count_nonzero(~np.isnan(x)) > 0
        # (dmag: the samples themselves differ by up to DMAG_ULP ulp)
        rtol = 4e-16 + (DMAG_ULP * 2.0 ** -52 if name.startswith("dmag") else 0.0)
        np.testing.assert_allclose([e["p16"], e["median"], e["p84"]],
                                   np.nanpercentile(x, [16, 50, 84]), rtol=rtol, atol=0)
    assert 0.0 < ph["planes"]["flux_ratio"]["median"] < 0.2      # truth 1970 / 29970
    with open(out + "step3_summary.json") as f:
        saved = json.load(f)
    assert saved["photometry"] == json.loads(json.dumps(ph))
    assert saved["astrometry"]["pasep_line"] == " , ".join(lines[1])
    assert os.path.basename(ph["file"]).endswith("_photometry.npz")
    with np.load(ph["file"]) as z:
        assert list(z["planes"]) == PLANES[2] and z["table"].shape == (7, 7)
        assert list(z["probs"]) == [0.16, 0.5, 0.84] and list(z["counts"]) == [ph["planes"][k]["n"] for k in PLANES[2]]
        assert list(z["snr"]) == ref["snr"] and float(z["fwhm_mean"]) == ref["fwhm_mean"]
        assert float(z["table"][0, 0]) == ph["planes"]["flux_ratio"]["median"]


def test_cli_photometry_three_sources(tmp_path, lib_loaded):
    """3body/apf_step3_3body.py --astrometry --photometry: snra, snrb, snrc, FWHMmean, FWHMstd
    in the 3-source script's field order (3body :575-590), 80 rows (the FWHM's indices wrap),
    and both companions' planes in the summary."""
    d = tmp_path / "2016_test"
    path = synth.write_case(str(d), 64, 3)
    img, _ = synth.make_image(64, 3, 0)
    fitsio.write(path, img, {**synth.HEADER, **HEADER})
    out = step2.main([path, "--walkers", "3", "--seed", "5", "--iters", "100", "--burn-in", "20",
                      "-q"], nsrc=3)
    got = step3.main([path, "sys", "-s", "3", "-q", "--astrometry", "--photometry"], nsrc=3)
    chains = step3.load_chains(out, 3, 1)
    assert chains.shape[2] == 20 and 50 <= chains.shape[0] < 100
    image, hdr = fitsio.getdata_header(path)
    pixscale = header_scalars(hdr, "post")["pixscale"]           # directory 2016_*
    ref = reference_numbers(image, chains, pixscale, 3)
    with open(str(d) + "/epoch_grand_pasep") as f:
        pf = f.read().splitlines()[0].split(" , ")
    assert len(pf) == 16 and len(ref["snr"]) == 3
    assert pf[9:14] == [py2_str(v) for v in ref["snr"] + [ref["fwhm_mean"], ref["fwhm_std"]]]
    assert all(np.isfinite(v) for v in ref["snr"]) and ref["snr"][0] > 10.0
    ph = got["photometry"]
    assert list(ph["planes"]) == PLANES[3] and ph["pixscale"] == 9.971
    planes, bad = restate(chains, 3, pixscale)
    assert ph["unusable"] == bad
    for name, x in zip(PLANES[3], planes):
        if not name.startswith("dmag"):
            np.testing.assert_allclose(ph["planes"][name]["median"], np.nanpercentile(x, 50),
                                       rtol=4e-16, atol=0)
