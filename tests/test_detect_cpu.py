"""The host side of the companion detection map (olpefit_amd/detect.py) and the long-double
restatement the GPU tests compare the device with (tests/detect_restatement.py).  No GPU."""
import functools

import numpy as np
import pytest

import detect_restatement as dr
from olpefit_amd import detect as dt, step3, synth

LD = np.longdouble


def hand_state(S=7, g=5, seed=3):
    """Per-sample planes [S][g][g] and the state a fold about row 0 would hold; candidate
    (1, 2) is blind."""
    rng = np.random.RandomState(seed)
    A = 50.0 + 10.0 * rng.normal(size=(S, g, g))
    sg = 8.0 + rng.uniform(size=(S, g, g))
    A[:, 1, 2] = sg[:, 1, 2] = np.nan
    snr = A / sg
    piv = np.stack([A[0], sg[0], snr[0]])
    da, ds = A - A[0], snr - snr[0]
    sums = np.stack([da.sum(0), (da * da).sum(0), (sg * sg).sum(0), ds.sum(0), (ds * ds).sum(0)])
    row = np.append(synth.truth_params(64, 2), 5.0)
    return A, sg, snr, piv, {"n": S, "n_bad": 2, "pivot": row, "sums": sums, "best": row}


def test_planes_from_state_against_the_restatement():
    A, sg, snr, piv, st = hand_state()
    got, sc = dt.planes_from_state(st, piv, best_planes=piv)
    e = {"A": A.reshape(7, -1).astype(LD), "sigma": sg.reshape(7, -1).astype(LD),
         "snr": snr.reshape(7, -1).astype(LD)}
    e.update(bA=np.zeros((7, 25)), bsigma=np.zeros((7, 25)), bsnr=np.zeros((7, 25)))
    with np.errstate(all="ignore"):
        want, _ = dr.planes(e)
    ok = np.ones(25, bool)
    ok[1 * 5 + 2] = False
    for k, w in want.items():
        g = got[k].ravel()
        assert np.isnan(g[~ok]).all(), k
        assert np.allclose(g[ok], w[ok].astype(np.float64), rtol=1e-11, atol=0), k
    assert np.array_equal(got["amp_best"], piv[0], equal_nan=True)
    assert sc["samples"] == 7 and sc["n_bad"] == 2 and sc["blind"] == 1
    marg = got["snr_marg"].ravel()
    assert sc["max_snr_at"] == int(np.nanargmax(marg)) and sc["max_snr"] == np.nanmax(marg)
    assert sc["min_snr"] == np.nanmin(marg)
    assert sc["median_sigma"] == np.nanmedian(got["sigma_total"])
    with pytest.raises(ValueError, match="no usable sample"):
        dt.planes_from_state({**st, "n": 0}, piv)


def test_one_sample_state_gives_the_pivot_planes_back():
    A, sg, snr, piv, st = hand_state(S=1)
    got, _ = dt.planes_from_state(st, piv)
    assert np.array_equal(got["amp_mean"], A[0], equal_nan=True)
    assert np.array_equal(got["sigma_stat"], np.sqrt(sg[0] * sg[0]), equal_nan=True)
    assert np.array_equal(got["snr_mean"], snr[0], equal_nan=True)
    assert np.all(got["amp_std"][~np.isnan(A[0])] == 0.0)


def test_contrast_curve_rings_nans_and_closed_form():
    g, flux0, pix = 21, 2.0e4, 9.952
    sigma = np.full((g, g), 8.0)
    sigma[3, 4] = np.nan
    centre = (10.0, 10.0)
    c = dt.contrast_curve(sigma, centre, flux0, pix, k=5, bin_px=1.0)
    y, x = np.mgrid[:g, :g]
    r = np.hypot(x - 10.0, y - 10.0)
    ring = np.floor(r).astype(int)
    ok = ~np.isnan(sigma)
    rings = np.unique(ring[ok])
    assert np.array_equal(c["count"], [int((ok & (ring == i)).sum()) for i in rings])
    assert c["count"].sum() == g * g - 1 and c["count"][0] == 1
    assert np.array_equal(c["sep_px"], rings + 0.5) and np.allclose(c["sep_mas"], c["sep_px"] * pix)
    want = 5 * 8.0 / flux0
    assert np.all(c["contrast_median"] == want) and np.all(c["contrast_min"] == want)
    assert np.allclose(c["dmag_median"], -2.5 * np.log10(want), rtol=0, atol=1e-12)
    # a wider bin, an oversampled lattice: positions are index / oversample
    c2 = dt.contrast_curve(sigma, (5.0, 5.0), flux0, pix, k=3, bin_px=2.0, oversample=2)
    r2 = np.hypot(x / 2.0 - 5.0, y / 2.0 - 5.0)
    assert c2["count"][0] == int((ok & (r2 < 2.0)).sum())
    assert np.all(c2["contrast_min"] == 3 * 8.0 / flux0)
    # a brighter ring member sets the minimum only
    s3 = sigma.copy()
    s3[10, 15] = 4.0
    c3 = dt.contrast_curve(s3, centre, flux0, pix)
    i = int(np.flatnonzero(c3["sep_px"] == 5.5)[0])
    assert c3["contrast_min"][i] == 5 * 4.0 / flux0 and c3["contrast_median"][i] == want


def test_candidates_bump_plateau_flag_and_threshold():
    g = 16
    snr = np.zeros((g, g))
    amp, sig = 10.0 * np.ones((g, g)), 2.0 * np.ones((g, g))
    snr[4:7, 8:11] = 5.5
    snr[5, 9] = 7.0                                   # a 3x3 bump, strict centre
    snr[11, 3] = snr[11, 4] = 9.0                     # a plateau of two: no strict maximum
    snr[13, 13] = 5.0                                 # exactly the threshold
    snr[14, 14] = np.nan                              # a NaN neighbour is no neighbour
    snr[0, 0] = 6.0                                   # a corner: three neighbours
    known = [(9.0, 6.5), (2.0, 2.0)]
    c = dt.candidates(snr, amp, sig, known, threshold=5.0, exclude_px=2.0, flux0=100.0,
                      pixscale=10.0)
    assert [(d["x"], d["y"]) for d in c] == [(9.0, 5.0), (0.0, 0.0), (13.0, 13.0)]
    assert [d["flagged"] for d in c] == [True, False, False]       # flagged, not dropped
    assert c[0]["snr"] == 7.0 and c[0]["index"] == 5 * g + 9
    assert c[0]["contrast"] == 0.1 and c[0]["dmag"] == 2.5
    assert c[0]["sep_px"] == 1.5 and c[0]["sep_mas"] == 15.0 and c[0]["pa_deg"] == 270.0
    assert c[2]["pa_deg"] == pytest.approx(np.degrees(np.arctan2(6.5, 4.0)))
    assert [d["x"] for d in dt.candidates(snr, amp, sig, known, threshold=5.0 + 1e-12)] == [9.0, 0.0]
    assert dt.candidates(snr, amp, sig, known, threshold=7.5) == []
    half = dt.candidates(snr, amp, sig, known, threshold=6.5, oversample=2)
    assert (half[0]["x"], half[0]["y"]) == (4.5, 2.5)
    lines = dt.table_lines({"samples": 3, "n_bad": 0, "pixels": 9, "blind": 0, "max_snr": 7.0,
                            "max_snr_at": 89, "min_snr": 0.0, "median_sigma": 2.0}, c,
                           dt.contrast_curve(sig, known[0], 100.0, 10.0))
    assert any("near a fitted source" in ln for ln in lines) and any("rings" in ln for ln in lines)


def test_state_merge_algebra_and_pivot_mismatch():
    _, _, _, _, a = hand_state(S=4, seed=1)
    _, _, _, _, b = hand_state(S=6, seed=2)
    b = {**b, "best": np.append(b["best"][:-1], 3.0)}
    m = dt.merge_states(a, b)
    assert m["n"] == 10 and m["n_bad"] == 4
    assert np.array_equal(m["sums"], a["sums"] + b["sums"], equal_nan=True)
    assert m["best"][-1] == 3.0                       # strictly smaller wins
    assert dt.merge_states(b, a)["best"][-1] == 3.0   # ... and stays
    tie = dt.merge_states(a, {**b, "best": a["best"] + 0.0})
    assert tie["best"] is not b["best"] and np.array_equal(tie["best"], a["best"])
    empty = {"n": 0, "n_bad": 1, "pivot": np.full(17, np.nan), "sums": np.zeros_like(a["sums"]),
             "best": np.full(17, np.nan)}
    e = dt.merge_states(empty, a)
    assert e["n"] == 4 and e["n_bad"] == 3 and np.array_equal(e["pivot"], a["pivot"])
    assert np.array_equal(dt.merge_states(a, empty)["sums"], a["sums"], equal_nan=True)
    other = {**b, "pivot": b["pivot"] * (1 + 2.0 ** -52)}
    with pytest.raises(ValueError, match="pivots differ"):
        dt.merge_states(a, other)
    # the chi^2 slot of the pivot plays no part
    assert dt.merge_states(a, {**b, "pivot": np.append(b["pivot"][:-1], 99.0)})["n"] == 10


def test_lattice_and_vector_helpers():
    assert [dt.lattice_side(33, o) for o in dt.OVERSAMPLE] == [33, 65, 129]
    assert np.array_equal(dt.lattice(3, 2), [0.0, 0.5, 1.0, 1.5, 2.0])
    for nsrc in (2, 3):
        p = synth.truth_params(64, nsrc)
        assert dt.flux0_of(p, nsrc) == 3.0e4 - 30.0
        assert dt.known_of(p, nsrc)[1] == (p[2], p[3]) and len(dt.known_of(p, nsrc)) == nsrc
        assert dt.default_exclude_px(p, nsrc) == 2.355 * (synth.SIGMA0 * 1.05)
        q, dx, dy, nar, wid = dr.shape_of(p, nsrc)
        assert (q, dx, dy) == (0.2, 0.1, -0.1) and nar[0] == synth.SIGMA0 and wid[2] == 0.10


def test_cli_detect_needs_the_chain_rows(capsys):
    for main_nsrc in (2, 3):
        with pytest.raises(SystemExit) as e:
            step3.main(["x/N2.20250127.00001.LDIF.fits", "sys", "-s", "4", "--detect",
                        "--from-moments"], nsrc=main_nsrc)
        assert e.value.code == 2
        assert "--detect needs the chain rows" in capsys.readouterr().err
    for bad in (["--detect-oversample", "3"], ["--detect-thin", "0"]):
        with pytest.raises(SystemExit):
            step3.main(["x/N2.20250127.00001.LDIF.fits", "sys", "-s", "4", "--detect"] + bad)
        capsys.readouterr()


def test_restatement_reads_psi_at_the_same_arguments():
    """The table read per candidate equals psi evaluated directly at x_i - x_c, y_i - y_c, at
    every oversample: the restatement's only shortcut changes nothing."""
    n, p = 9, synth.truth_params(9, 2)
    y, x = np.mgrid[:n, :n]
    for os_, (jy, jx) in ((1, (3, 7)), (2, (5, 16)), (4, (31, 2))):
        cy, py = divmod(jy, os_)
        cx, px = divmod(jx, os_)
        T, _ = dr.table(p, 2, n, os_, (py, px))
        K = T[n - 1 - cy:2 * n - 1 - cy, n - 1 - cx:2 * n - 1 - cx]
        want, _ = dr.psi(p, 2, x - LD(jx) / os_, y - LD(jy) / os_)
        assert np.array_equal(K, want)
    # the peak of psi: (1 - q) + q g2(-dx, -dy) at the origin
    assert float(dr.psi(p, 2, LD(0), LD(0))[0]) == pytest.approx(0.8 + 0.2, abs=1e-3)


@functools.lru_cache(maxsize=None)
def injection(n, amp, pos, seed):
    img, p = dr.inject(n, amp, pos, seed)
    A, s, r = dr.full_map(dr.Frame(img), p, 2)
    return p, A, s, r


@pytest.mark.parametrize("n, amp, pos", [(64, 80.0, (15.7, 45.3)), (33, 100.0, (7.4, 24.6))])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_injection_is_found_by_the_restatement(n, amp, pos, seed):
    """synth.truth_params(n, 2) rendered, amp x psi_truth added at pos, noise as
    synth.make_image draws it; the restatement's map at theta = truth with core.noise_model's
    err.  Amplitudes as the issue chose them: 80 at 64x64 (snr 8.9 .. 10.9, sigma_A 8.1 .. 8.2
    over seeds 0 - 3), 100 at 33x33 (snr 8.8 .. 9.1); the project's err did not move them.
    The peak is within one lattice step of the injection with snr >= 6, it is the only
    candidate above 5 outside the fitted sources, and the same frame without the injection
    has none."""
    p, A, s, r = injection(n, amp, pos, seed)
    jy, jx = divmod(int(np.nanargmax(r)), n)
    print(f"n {n} seed {seed}: peak ({jx}, {jy}) snr {r[jy, jx]:.2f} A {A[jy, jx]:.1f} "
          f"sigma {s[jy, jx]:.2f}")
    assert abs(jx - pos[0]) <= 1 and abs(jy - pos[1]) <= 1
    assert r[jy, jx] >= 6.0
    assert abs(A[jy, jx] - amp) <= 3 * s[jy, jx]
    known, ex = dt.known_of(p, 2), dt.default_exclude_px(p, 2)
    free = [c for c in dt.candidates(r, A, s, known, 5.0, ex) if not c["flagged"]]
    assert len(free) == 1 and (free[0]["x"], free[0]["y"]) == (jx, jy)
    _, A0, s0, r0 = injection(n, 0.0, pos, seed)
    assert [c for c in dt.candidates(r0, A0, s0, known, 5.0, ex) if not c["flagged"]] == []


def test_chosen_candidates_cover_the_edge_cases():
    img, p = synth.make_image(33, 2, 0)
    fr = dr.Frame(img)
    for os_ in (1, 2, 4):
        g = dt.lattice_side(33, os_)
        c = dr.chosen(33, 2, p, fr.mask, os_)
        have = {tuple(x) for x in c}
        assert {(0, 0), (0, g - 1), (g - 1, 0), (g - 1, g - 1), (0, g // 2)} <= have
        for x, y in dr.sources_of(p, 2):
            assert (int(round(y * os_)), int(round(x * os_))) in have
        assert fr.mask.any() and len(c) >= 50 and c.min() >= 0 and c.max() < g
