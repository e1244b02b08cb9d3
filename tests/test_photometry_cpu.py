"""The host side of the photometry (olpefit_amd/photometry.py): the exact circle-pixel
overlap, the reference's aperture S/N and FWHM lines (apf_step3.py:454-511), the pasep
line's photometry fields and the command line's argument check.  No GPU."""
import numpy as np
import pytest

from olpefit_amd import step3
from olpefit_amd.astrometry import pasep_line, py2_str
from olpefit_amd.photometry import (aperture_snr, circle_overlap, interpolate, reference_fwhm,
                                    source_positions)

L = np.longdouble
GRID = 48
RADII = (5, 11, 14)
CENTRES = ((20, 20), (20.5, 20.5), (20.3, 19.6))


def restated_overlap(ny, nx, x0, y0, r):
    """Per pixel, the integral over x of the length of the pixel's column inside the circle,
    in closed form and in np.longdouble.  With h(x) = sqrt(r^2 - x^2), a pixel [x1, x2] x
    [y1, y2] (relative to the centre) holds, at x, the length max(0, min(y2, h) - max(y1,
    -h)).  A pixel below the centre is mirrored above it; one that straddles y = 0 has
    min(y2, h) + min(-y1, h) >= 0; one above it is cut to |x| <= sqrt(r^2 - y1^2), where
    h >= y1, and holds min(y2, h) - y1 there.  Both need only M(c) = the integral of
    min(c, h) for a constant c >= 0, which is c times the length where h >= c (|x| <=
    sqrt(r^2 - c^2)) plus the integral of h elsewhere, G(t) = (t sqrt(r^2 - t^2) + r^2
    asin(t / r)) / 2."""
    r = L(r)
    x1 = (np.arange(nx).astype(L) - L(0.5) - L(x0))[None, :] + np.zeros((ny, 1), dtype=L)
    y1 = (np.arange(ny).astype(L) - L(0.5) - L(y0))[:, None] + np.zeros((1, nx), dtype=L)
    x2, y2 = x1 + 1, y1 + 1
    low = y2 <= 0
    y1, y2 = np.where(low, -y2, y1), np.where(low, -y1, y2)

    def G(t):
        return (t * np.sqrt(np.maximum(r * r - t * t, 0)) + r * r * np.arcsin(t / r)) / 2

    def M(c, a, b):
        xc = np.sqrt(np.maximum(r * r - c * c, 0))
        lo, hi = np.maximum(a, -xc), np.minimum(b, xc)
        inside = np.maximum(hi - lo, 0)
        return c * inside + (G(b) - G(a)) - np.where(inside > 0, G(hi) - G(lo), 0)

    a, b = np.clip(x1, -r, r), np.clip(x2, -r, r)
    straddle = M(y2, a, b) + M(-y1, a, b)
    X = np.sqrt(np.maximum(r * r - y1 * y1, 0))
    a2, b2 = np.maximum(a, -X), np.minimum(b, X)
    a2 = np.minimum(a2, b2)
    above = M(y2, a2, b2) - y1 * (b2 - a2)
    return np.where(y1 < 0, straddle, np.where(y1 < r, above, 0))


def overlap_bound(r, grid=GRID):
    """The largest difference a correct double-precision overlap may show against the
    restatement, from rounding alone.  (a) The code forms a pixel's four edges i -+ 1/2 - x0
    in double: each is off by at most ulp(grid) / 2 <= grid * 2^-53 and moves the area by at
    most that times the pixel's side.  (b) Its closed form adds 2 x 4 quadrant terms, each a sum
    of three quantities of at most pi r^2 / 4 reached through at most 8 roundings.  (c) The
    restatement's own rounding is the same count at 2^-64.  Nothing here is measured on the
    code under test."""
    u, ul = 2.0 ** -53, 2.0 ** -64
    return 4 * grid * u + 4 * 3 * 8 * (np.pi * r * r / 4) * (u + ul)


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("centre", CENTRES)
def test_overlap_sums_to_the_circle_and_matches_the_restatement(centre, r):
    x0, y0 = centre
    w = circle_overlap(GRID, GRID, x0, y0, r)
    assert w.shape == (GRID, GRID) and w.dtype == np.float64
    assert abs(np.sum(w.astype(L)) - L(np.pi) * r * r) <= 1e-12 * np.pi * r * r
    assert w.min() >= 0.0 and w.max() <= 1.0
    j, i = np.mgrid[:GRID, :GRID]
    far = np.hypot(np.abs(i - x0) + 0.5, np.abs(j - y0) + 0.5)
    near = np.hypot(np.maximum(np.abs(i - x0) - 0.5, 0), np.maximum(np.abs(j - y0) - 0.5, 0))
    assert (far < r - 1e-9).any() and (near > r + 1e-9).any()
    assert np.all(w[far < r - 1e-9] == 1.0) and np.all(w[near > r + 1e-9] == 0.0)
    ref = restated_overlap(GRID, GRID, x0, y0, r)
    dev = float(np.max(np.abs(w.astype(L) - ref)))
    print(f"centre {centre} r {r}: max |overlap - restatement| {dev:.3e}, bound "
          f"{overlap_bound(r):.3e}")
    assert dev <= overlap_bound(r)


@pytest.mark.parametrize("r", RADII)
def test_overlap_has_the_eightfold_symmetry_about_a_pixel_centre(r):
    w = circle_overlap(GRID, GRID, 20, 20, r)[20 - 16:20 + 17, 20 - 16:20 + 17]
    for other in (w[::-1], w[:, ::-1], w[::-1, ::-1], w.T, w.T[::-1], w.T[:, ::-1],
                  w.T[::-1, ::-1]):
        assert np.array_equal(w, other)


@pytest.mark.parametrize("r", RADII)
def test_overlap_off_the_grid_is_the_larger_grid_cropped(r):
    # centre 3 px from two edges: the circle leaves the 48 x 48 grid on both
    big = circle_overlap(GRID + 40, GRID + 40, 3.3 + 20, 2.6 + 20, r)
    small = circle_overlap(GRID, GRID, 3.3, 2.6, r)
    assert small.sum() < 0.95 * np.pi * r * r
    # the shifted centre rounds its edges and its closed form differently: each grid is
    # within its own bound of the true areas
    assert np.max(np.abs(small - big[20:20 + GRID, 20:20 + GRID])) <= \
        overlap_bound(r) + overlap_bound(r, GRID + 40)
    # and exactly, where the shift is by whole pixels of a centre that stays representable
    big = circle_overlap(GRID + 32, GRID + 32, 3.25 + 16, 2.5 + 16, r)
    small = circle_overlap(GRID, GRID, 3.25, 2.5, r)
    assert np.array_equal(small, big[16:16 + GRID, 16:16 + GRID])


def test_aperture_signal_is_the_bright_pixels_excess():
    # apf_step3.py:476-495: the aperture sits at (x - 1, y - 1); the pixel there is wholly
    # inside it.  On a zero background every sum holds one term: exact.
    img = np.zeros((64, 64))
    img[29, 33] = 1234.5
    snr, signal, noise = aperture_snr(img, 34, 30, parts=True)
    assert signal == 1234.5
    assert noise == 0.0 and snr == np.inf          # the box holds zeros only
    # on a constant c the aperture and the scaled annulus cancel as far as the weights sum
    # to their areas: to 1e-12 relative each (the bound of the overlap test above), which
    # leaves at most c * ap.area * 2e-12; twice that covers the sums' own rounding
    c = 3.0
    img = np.full((64, 64), c)
    img[29, 33] += 1234.5
    img[45, 50] += 1.0                             # in the noise box [42:57, 46:61]
    snr, signal, noise = aperture_snr(img, 34, 30, parts=True)
    assert abs(signal - 1234.5) <= 4e-12 * c * np.pi * 25
    box = img[42:57, 46:61]
    assert box.shape == (15, 15)
    assert noise == np.std(box) * np.sqrt(np.pi * 25) and snr == signal / noise
    # a pixel outside the aperture and the annulus changes nothing; one in the annulus
    # lowers the signal by ap.area / annulus.area of its excess
    img2 = img.copy()
    img2[29 + 12, 33] += 75.0
    _, s2, _ = aperture_snr(img2, 34, 30, parts=True)
    want = signal - 75.0 * 25.0 / (14 ** 2 - 11 ** 2)
    assert abs(s2 - want) <= 1e-12 * abs(want)


def test_noise_box_follows_numpy_slicing():
    rng = np.random.RandomState(3)
    img = rng.normal(10.0, 2.0, size=(48, 48))
    # y + 12 = 40: rows 40..47 only (8 of 15); x + 12 = 30: all 15 columns
    _, _, noise = aperture_snr(img, 18, 28, parts=True)
    assert img[40:55, 30:45].shape == (8, 15)
    assert noise == np.std(img[40:55, 30:45]) * np.sqrt(np.pi * 25)
    # y + 12 = 48: an empty box
    snr, signal, noise = aperture_snr(img, 18, 36, parts=True)
    assert np.isnan(noise) and np.isnan(snr) and np.isfinite(signal)
    assert np.isnan(aperture_snr(img, 18, 36))


def restated_fwhm(sigmax, sigmay, pixscale):
    """apf_step3.py:454-470 line by line."""
    majorsigma = np.array([])
    sigx = np.array([])
    sigy = np.array([])
    for i in np.arange(len(sigmax) - 100, len(sigmax)):
        sigx = np.append(sigx, sigmax[i])
    for i in np.arange(0, len(sigmay)):
        sigy = np.append(sigx, sigmay[i])
    for i, j in zip(sigx, sigy):
        biggestsigma = np.max([i, j])
        majorsigma = np.append(majorsigma, biggestsigma)
    FWHM = 2.355 * majorsigma * pixscale
    return np.mean(FWHM), np.std(FWHM)


@pytest.mark.parametrize("rows", [130, 60])
def test_reference_fwhm_is_the_literal_reading(rows):
    rng = np.random.RandomState(rows)
    sigmax = 1.5 + 0.1 * rng.normal(size=(rows, 3))
    sigmay = 5.0 + 0.1 * rng.normal(size=(rows, 3))      # larger, and never enters
    mean, std = reference_fwhm(sigmax, 9.952)
    rmean, rstd = restated_fwhm(sigmax, sigmay, 9.952)
    assert mean == rmean and std == rstd
    assert mean < 2.355 * 3.0 * 9.952


def test_reference_fwhm_raises_below_fifty_rows():
    sigmax = np.full((40, 3), 1.5)
    with pytest.raises(IndexError):
        restated_fwhm(sigmax, sigmax, 9.952)
    with pytest.raises(IndexError):
        reference_fwhm(sigmax, 9.952)
    reference_fwhm(np.full((50, 3), 1.5), 9.952)


def test_source_positions_are_the_integer_means_after_the_offset():
    c = np.zeros((4, 2, 20))
    c[:, :, 0], c[:, :, 1] = 30.7, 31.2
    c[:, :, 2], c[:, :, 3] = 40.999, 12.0
    c[:, :, 4], c[:, :, 5] = 7.5, 8.49
    assert source_positions(c[:, :, :17], 2) == [(31, 32), (41, 13)]
    assert source_positions(c, 3) == [(31, 32), (41, 13), (8, 9)]


RES = [{"sep_median": 100.5, "sep_std": 0.25, "pa_median": 33.0, "pa_std": 0.125},
       {"sep_median": 200.0, "sep_std": 0.5, "pa_median": 133.0, "pa_std": 1.0 / 3.0}]


def test_pasep_line_without_photometry_is_unchanged():
    assert pasep_line("K", RES[:1], 1.01, 0.002) == \
        "K , 100.5 , 0.25 , 33.0 , 0.125 , nan , nan , nan , nan , 1.01 , 0.002"
    assert pasep_line("K", RES[:1], 1.01, 0.002, 2, photometry=None) == \
        pasep_line("K", RES[:1], 1.01, 0.002, 2)
    assert pasep_line("K", RES, 1.01, 0.002, 3) == \
        ("K , 100.5 , 0.25 , 33.0 , 0.125 , 200.0 , 0.5 , 133.0 , 0.333333333333 , "
         "nan , nan , nan , nan , nan , 1.01 , 0.002")


def test_pasep_line_carries_the_photometry_in_the_references_order():
    ph = {"snr": [812.25, 41.0], "fwhm_mean": 49.5, "fwhm_std": 1.0 / 7.0}
    f = pasep_line("K", RES[:1], 1.01, 0.002, 2, photometry=ph).split(" , ")
    # apf_step3.py:517-527: starsnr, compsnr, FWHMmean, FWHMstd after the four astrometry fields
    assert f[5:9] == ["812.25", "41.0", "49.5", py2_str(1.0 / 7.0)] and len(f) == 11
    assert f[:5] + f[9:] == pasep_line("K", RES[:1], 1.01, 0.002, 2).split(" , ")[:5] + \
        ["1.01", "0.002"]
    ph3 = {"snr": [812.25, 41.0, float("nan")], "fwhm_mean": 49.5, "fwhm_std": 0.5}
    f = pasep_line("K", RES, 1.01, 0.002, 3, photometry=ph3).split(" , ")
    # 3body :575-590: snra, snrb, snrc, FWHMmean, FWHMstd after the eight astrometry fields
    assert f[9:14] == ["812.25", "41.0", "nan", "49.5", "0.5"] and len(f) == 16
    with pytest.raises(ValueError):
        pasep_line("K", RES, 1.01, 0.002, 3, photometry=ph)


def test_interpolate_is_numpys_linear_rule():
    rng = np.random.RandomState(7)
    for n in (1, 2, 3, 10, 257):
        x = np.sort(rng.normal(size=n))
        for p in (0.0, 0.16, 0.5, 0.84, 1.0, 1.0 / 3.0):
            vi = (n - 1) * p
            lo, hi = x[int(np.floor(vi))], x[int(np.ceil(vi))]
            assert interpolate(lo, hi, n, p) == np.quantile(x, p)
    assert np.isnan(interpolate(np.nan, np.nan, 0, 0.5))


@pytest.mark.parametrize("nsrc", [2, 3])
def test_cli_refuses_photometry_from_moments(nsrc, capsys):
    with pytest.raises(SystemExit) as e:
        step3.main(["d/2014_x/N2.20140101.00001.LDIF.fits", "sys", "-s", "4", "--photometry",
                    "--from-moments"], nsrc=nsrc)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--photometry needs the chain rows" in err and "percentile is not a moment" in err
    with pytest.raises(SystemExit):
        step3.main(["d/2014_x/N2.20140101.00001.LDIF.fits", "sys", "-s", "4", "--photometry",
                    "--photometry-thin", "0"], nsrc=nsrc)
