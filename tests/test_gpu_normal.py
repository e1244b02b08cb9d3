"""The Gauss-Newton sums on the device (olpe_normal.hip, Sampler.normal_equations) and the
per-pixel derivatives behind them (olpe_test_jacobian) against the long-double restatement
of tests/normal_restatement.py.

Bounds (derived, not tuned).  u = 2^-53, N = n^2 pixels, w = 1 / err (0 at masked pixels).
  J per pixel   delta_k = 1e-13 x max_p |J_ref[:, k]|: the project's EXACT model tolerance
                 applied per column.  A column that is identically zero in the
                restatement (theta at sigma_x = sigma_y) must be exactly zero on the device.
  Jw = J w      eJw_k = delta_k w + 4 u |Jw|: the rounded w, the product, and J's own error.
  r             er = delta_M w + 4 u |r|, delta_M = 1e-13 max|M| (as test_gpu_predictive).
  chi2          sum (2 |r| er + er^2) + N u sum r^2.
  grad[k]       sum (|Jw_k| er + |r| eJw_k + eJw_k er + u |Jw_k r|) + N u sum |Jw_k r|:
                each product's 4 u-free factors' errors, its rounding, and a fixed-order sum
                of N terms (per-lane FMAs, then a tree: at most N roundings deep).
  jtj[k][l]     sum (|Jw_k| eJw_l + |Jw_l| eJw_k + eJw_k eJw_l + u |Jw_k Jw_l|)
                + N u sum |Jw_k Jw_l|; the matrix core's FP64 FMAs round like the VALU's.
No column needed more than this: the largest measured error is a few percent of its bound
(DESIGN.md §7k has the ratios per quantity).  Where the same operations run on the same
values the comparison is np.array_equal: symmetry, the place in a batch, repeats, the
context's eval mode, the content of masked pixels.

Frames: the fixtures c32 (two rows of the cutout a 64-pixel step), c64, c64_3, c128_3 and
the non-finite-pixel fixtures c64_nan, c64_3_nan with their 14 vectors each (off-image
source, tiny core, ratio > 1, rotated wide component); s33 (33 x 33: the last step of 64
pixels is partial) with c32's vectors; c64 in bkgd_mode 1; synth.make_image's y33, y64, y64_3
at truth (t = O(1), saturated core masked).
"""
import functools
import os

import numpy as np
import pytest

import normal_restatement as nr
from olpefit_amd import core, synth
from olpefit_amd.core import Sampler

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LD = np.longdouble
U = nr.U
SYNTH = {"y33": (33, 2), "y64": (64, 2), "y64_3": (64, 3)}
FRAMES = ["c32", "s33", "c64", "c64_b1", "c64_3", "c128_3", "c64_nan", "c64_3_nan",
          "y33", "y64", "y64_3"]


def golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return z["image"], int(z["nsrc"]), z["params"].copy()


@functools.lru_cache(maxsize=None)
def case(name):
    """(image, nsrc, bkgd_mode, vectors [V, PS])."""
    if name in SYNTH:
        n, nsrc = SYNTH[name]
        img, truth = synth.make_image(n, nsrc, 0)
        return img, nsrc, 0, np.append(truth, 0.0)[None]
    if name == "s33":
        return synth.make_image(33, 2, 0)[0], 2, 0, golden("c32")[2]
    if name == "c64_b1":
        img, nsrc, params = golden("c64")
        return img, nsrc, 1, params[[1, 3, 12, 13]]
    img, nsrc, params = golden(name)
    return img, nsrc, 0, params


class Ref:
    """The restatement of one frame's vectors with the bounds, computed once."""

    def __init__(self, name):
        img, self.nsrc, self.bkgd_mode, self.vecs = case(name)
        self.img, self.n = img, img.shape[0]
        D, err, mask = nr.frame(img)
        self.mask = mask
        w = np.where(mask, 0.0, 1.0 / np.where(mask, 1.0, err))
        N = self.n * self.n
        self.J, self.dJ, self.chi2, self.grad, self.jtj, self.b = [], [], [], [], [], []
        for p in self.vecs:
            M, J = nr.jacobian(p, self.n, self.nsrc, self.bkgd_mode)
            r, Jw = nr.weighted(p, D, err, mask, self.nsrc, self.bkgd_mode)
            P = J.shape[0]
            dk = 1e-13 * np.abs(J).reshape(P, -1).max(axis=1).astype(np.float64)
            dM = 1e-13 * float(np.abs(M).max())
            A = np.abs(Jw).reshape(P, -1).astype(np.float64)
            ar = np.abs(r).ravel().astype(np.float64)
            E = dk[:, None] * w.ravel()[None] + 4 * U * A
            er = dM * w.ravel() + 4 * U * ar
            self.b.append({
                "chi2": float((2 * ar * er + er * er).sum() + N * U * (ar * ar).sum()),
                "grad": A @ er + E @ ar + E @ er + (N + 1) * U * (A @ ar),
                "jtj": A @ E.T + E @ A.T + E @ E.T + (N + 1) * U * (A @ A.T)})
            Jf = Jw.reshape(P, -1)
            self.J.append(J)
            self.dJ.append(dk)
            self.chi2.append((r * r).sum())
            self.grad.append(Jf @ r.ravel())
            self.jtj.append(Jf @ Jf.T)


@functools.lru_cache(maxsize=None)
def reference(name):
    return Ref(name)


def sampler(name, mode="exact"):
    img, nsrc, bkgd_mode, _ = case(name)
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc, bkgd_mode=bkgd_mode)
    s.set_eval_mode(mode)
    return s


def ratio(d, b):
    """max d / b, a zero bound allowing only a zero difference."""
    d, b = np.asarray(d, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.all(d[b == 0] == 0), "a quantity whose bound is 0 is not exactly 0"
    return float((d[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0


@pytest.mark.parametrize("name", FRAMES)
def test_jacobian_and_sums_against_the_restatement(lib_loaded, name):
    ref = reference(name)
    with sampler(name) as s:
        chi2, grad, jtj = s.normal_equations(ref.vecs)
        chi_eval = s.chi_squared(ref.vecs)
        planes = [s.test_jacobian(p) for p in ref.vecs]
    worst = {"J": 0.0, "chi2": 0.0, "grad": 0.0, "jtj": 0.0}
    for v in range(len(ref.vecs)):
        P = ref.J[v].shape[0]
        assert np.isfinite(planes[v]).all() and np.isfinite(jtj[v]).all(), (name, v)
        dJ = np.abs(planes[v].astype(LD) - ref.J[v]).reshape(P, -1).max(axis=1).astype(np.float64)
        rj = ratio(dJ, ref.dJ[v])
        assert rj <= 1.0, (name, v, "J", (dJ / np.maximum(ref.dJ[v], 1e-300)).round(3))
        b = ref.b[v]
        rc = ratio(abs(float(LD(chi2[v]) - ref.chi2[v])), b["chi2"])
        rg = ratio(np.abs(grad[v].astype(LD) - ref.grad[v]), b["grad"])
        rf = ratio(np.abs(jtj[v].astype(LD) - ref.jtj[v]), b["jtj"])
        assert rc <= 1.0 and rg <= 1.0 and rf <= 1.0, (name, v, rc, rg, rf)
        for k, r in (("J", rj), ("chi2", rc), ("grad", rg), ("jtj", rf)):
            worst[k] = max(worst[k], r)
        assert np.array_equal(jtj[v], jtj[v].T), (name, v)
        assert abs(chi2[v] - chi_eval[v]) <= 1e-12 * abs(chi_eval[v]), (name, v)
    print(name, " ".join(f"{k} {r:.2e}" for k, r in worst.items()), "(x bound)")


@pytest.mark.parametrize("name", ["s33", "c64", "c64_3", "c128_3"])
def test_a_vectors_bits_do_not_depend_on_the_batch(lib_loaded, name):
    """A vector alone, first, last and inside batches of W = 1, 3, 4, 5, 9, 17 (four waves a
    workgroup: every boundary), a repeat, and a FAST context: the same bits."""
    _, _, _, vecs = case(name)
    with sampler(name) as s, sampler(name, "fast") as sf:
        base = s.normal_equations(vecs)
        for a, b in zip(base, s.normal_equations(vecs)):
            assert np.array_equal(a, b)
        for a, b in zip(base, sf.normal_equations(vecs)):
            assert np.array_equal(a, b)
        for W in (1, 3, 4, 5, 9, 17):
            for pos in sorted({0, W // 2, W - 1}):
                idx = (np.arange(W) * 5 + 1) % len(vecs)
                idx[pos] = 2
                got = s.normal_equations(vecs[idx])
                for a, b in zip(base, got):
                    assert np.array_equal(a[idx], b), (name, W, pos)
        one = s.normal_equations(vecs[2, :-1])
        assert all(np.array_equal(a[2], b[0]) for a, b in zip(base, one))
        assert one[0].shape == (1,) and one[2].shape == (1, s.np_, s.np_)


@pytest.mark.parametrize("name", ["c64_nan", "c64_3_nan", "y33", "y64_3"])
def test_masked_pixels_contribute_nothing(lib_loaded, name):
    """Zeroing the masked pixels in the restatement equals the device (the first test, on
    frames that have them); and what a masked pixel holds plays no part: the same frame with
    other values there, under the same mask, gives the same bits."""
    img, nsrc, bkgd_mode, vecs = case(name)
    mask, pois2, rn2, _, _ = core.noise_model(img, 1.0, 1, 1, 2)
    assert 0 < mask.sum() < mask.size
    other = np.array(img)
    other[mask] = 12345.0
    with Sampler(img, nsrc=nsrc, mask=mask, pois2=pois2, readnoise2=rn2) as a, \
            Sampler(other, nsrc=nsrc, mask=mask, pois2=pois2, readnoise2=rn2) as b, \
            sampler(name) as c:
        ra, rb, rc = (s.normal_equations(vecs) for s in (a, b, c))
    assert np.isfinite(ra[0]).all()
    for x, y, z in zip(ra, rb, rc):
        assert np.array_equal(x, y) and np.array_equal(x, z)


@pytest.mark.parametrize("name", ["c64", "c64_3"])
def test_a_bad_vector_poisons_only_itself(lib_loaded, name):
    """A NaN parameter, an infinite one, and finite parameters whose model overflows (wide =
    (A - off) ratio = inf) in mid-batch: NaN in all their outputs, the rest bit-unchanged."""
    _, nsrc, _, vecs = case(name)
    c = nr.columns(nsrc)
    batch = vecs[:9].copy()
    batch[2, 0] = np.nan
    batch[4, c["amp"][1]] = np.inf
    batch[7, c["amp"][0]], batch[7, c["ratio"]] = 1e308, 20.0
    bad = [2, 4, 7]
    good = [k for k in range(9) if k not in bad]
    with sampler(name) as s:
        clean = s.normal_equations(vecs[:9])
        got = s.normal_equations(batch)
    for a, b in zip(clean, got):
        assert np.isnan(b[bad]).all()
        assert np.array_equal(a[good], b[good])


def test_corner_by_a_third_mfma_agrees(lib_loaded, monkeypatch):
    """OLPE_NORMAL_CORNER=mfma (the A/B of DESIGN.md 7k) changes the 3 x 3 corner of the
    3-source J^T J alone, within the same bounds; another value is refused."""
    ref = reference("c64_3")
    with sampler("c64_3") as s:
        base = s.normal_equations(ref.vecs)
        monkeypatch.setenv("OLPE_NORMAL_CORNER", "mfma")
        got = s.normal_equations(ref.vecs)
        monkeypatch.setenv("OLPE_NORMAL_CORNER", "both")
        with pytest.raises(core.OlpeError):
            s.normal_equations(ref.vecs)
    assert np.array_equal(base[0], got[0]) and np.array_equal(base[1], got[1])
    lo = np.ones((19, 19), bool)
    lo[16:, 16:] = False
    assert np.array_equal(base[2][:, lo], got[2][:, lo])
    for v in range(len(ref.vecs)):
        assert np.array_equal(got[2][v], got[2][v].T)
        d = np.abs(got[2][v].astype(LD) - ref.jtj[v])
        assert ratio(d[16:, 16:], ref.b[v]["jtj"][16:, 16:]) <= 1.0


def test_off_is_flat_in_two_source_mode_0(lib_loaded):
    """|jtj (e_amps + e_ampc + e_off)| <= the entries' bounds + 3 u sum |entries| in the
    2-source layout with bkgd_mode 0 (the exact value is 0); in bkgd_mode 1 it is not small."""
    v = np.zeros(16)
    v[[6, 7, 9]] = 1.0
    for name in ("c64", "y64"):
        ref = reference(name)
        with sampler(name) as s:
            _, grad, jtj = s.normal_equations(ref.vecs)
        for q in range(len(ref.vecs)):
            got = np.abs((jtj[q].astype(LD) @ v.astype(LD)).astype(np.float64))
            bound = ref.b[q]["jtj"] @ v + 3 * U * (np.abs(jtj[q]) @ v)
            assert np.all(got <= bound), (name, q, (got / bound).max())
            assert abs(float(grad[q].astype(LD) @ v.astype(LD))) <= ref.b[q]["grad"] @ v \
                + 3 * U * (np.abs(grad[q]) @ v)
    ref = reference("c64_b1")
    with sampler("c64_b1") as s:
        jtj = s.normal_equations(ref.vecs)[2]
    assert np.abs(jtj[0] @ v).max() > 1e3 * (ref.b[0]["jtj"] @ v).max()
