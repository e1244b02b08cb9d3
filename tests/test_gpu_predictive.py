"""Pointwise deviance, WAIC and DIC on the device (olpe_lik.hip, olpefit_amd/predictive.py)
against the long-double restatement of tests/lik_restatement.py over the oracle's
build_analytical_model.

Bounds (derived, not tuned).  delta = 1e-13 x max|M_ref| is the project's EXACT model
tolerance, u = 2^-53.  The device forms t = (D - M) * w with w = 1 / err
rounded: a model within delta moves t by delta w, and the subtraction, the rounded w and the
product by 4 u |t| at most, so  dt_is = delta w_i + 4 u |t_is|  and x = t^2 lies within
eps_i = max_s (2 |t| dt + dt^2)  of the restatement's.
  point(vec)   <= eps of that vector.
  mean_dev     <= eps_i + 2 S u max_s |x - c_i|: a mean of values each within eps_i is
                  within it; the shifted sum of S terms adds ~S u of its largest term.
  std_dev      <= 2 eps_i + the same: |std(x + e) - std(x)| <= max|e|, doubled for the
                  one-pass form, as in test_gpu_resid.
  p_waic       <= (2 sigma b + b^2) S / (S - 1) / 4 with b std_dev's bound, from
                  |d sigma^2| <= 2 sigma d sigma + d sigma^2.
  lppd         <= eps_i / 2 + (S + 32) u nats: a sum of positive terms, each exponent off by
                  eps_i / 2 at most, exp_neg within 2 ulp, S additions, one log.
  totals       <= the sum of their pixels' bounds + N u sum|.|.
  se_elpd      <= sqrt(N) sqrt(N / (N - 1)) max_i (elpd's bound) + N u se, the std rule again.
Where the same operations run on the same values the comparison is np.array_equal: one
sample, dev_best against point(best), tile heights, repeats, unusable rows taken out, the
context's eval mode, the device chain against the same rows from the host.

Two kinds of rows.  The fixtures' p_init with relative scatter 1e-3 (c32, s33, c64, c64_3,
c128_3): x spans hundreds, so the log-sum-exp is dominated by single terms, rescales often
and underflows to 0.  synth.make_image's frame with rows about the vector it was drawn from
(y33, y64, y64_3): t = O(1), many comparable terms; asserted on the reference alone, every
unmasked pixel has (sum e)^2 / sum e^2 >= 16 for S = 257.

Shapes as test_gpu_resid: 32 (half the lanes idle), 33 (partial tile both ways), 64 with 2
and 3 sources, 128 (two column passes).  Counts B - 1, B, B + 1, 3 B + 5 of B = 256, and 1.
"""
import functools
import json
import os

import numpy as np
import pytest

import lik_restatement as lr
from olpefit_amd import _lib, fitsio, predictive, step2, step3, synth
from olpefit_amd.core import Sampler
from olpefit_amd.pipeline import initial_parameters
from olpefit_amd.predictive import Predictive
from test_predictive_cpu import lik_piece_blocks

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LD = np.longdouble
U = lr.U
B = 256
COUNTS = [1, B - 1, B, B + 1, 3 * B + 5]
SYNTH = {"y33": (33, 2), "y64": (64, 2), "y64_3": (64, 3)}
PLANE_CASES = ([("c64", S) for S in COUNTS] + [("c64_3", S) for S in COUNTS]
               + [(n, 3 * B + 5) for n in ("c32", "s33", "c128_3")]
               + [(n, B + 1) for n in SYNTH])


@functools.lru_cache(maxsize=None)
def case(name):
    """(image, nsrc, base row [PS]) of a fixture or of a synthetic frame."""
    if name in SYNTH:
        n, nsrc = SYNTH[name]
        img, truth = synth.make_image(n, nsrc, 0)
        return img, nsrc, np.append(truth, 0.0)
    if name == "s33":
        img, _ = synth.make_image(33, 2, 0)
        return img, 2, initial_parameters(img, synth.guess_values(33, 2), 2)
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return z["image"], int(z["nsrc"]), z["p_init"].copy()


def scatter(base, S, seed):
    """S rows of relative scatter 1e-3 about base (1e-3 absolute where it is 0), a chi^2
    column without ties."""
    rng = np.random.RandomState(seed)
    P = base.size - 1
    rows = np.tile(base, (S, 1))
    rows[:, :P] = base[:P] * (1.0 + 1e-3 * rng.normal(size=(S, P))) \
        + np.where(base[:P] == 0.0, 1e-3, 0.0) * rng.normal(size=(S, P))
    rows[:, P] = rng.uniform(1e3, 2e3, size=S)
    return rows


class Ref:
    """The restatement of one set of rows on one frame, computed once."""

    def __init__(self, img, nsrc, rows, pivot_row=0):
        self.rows, self.nsrc, self.n = rows, nsrc, img.shape[0]
        self.D, self.err, self.mask = lr.frame(img)
        self.ok = ~self.mask
        self.M = lr.models(rows, self.n, nsrc)
        self.t, self.x = lr.deviance(self.M, self.D, self.err, self.mask)
        self.planes = lr.planes(self.x, self.mask)
        self.c = self.x[pivot_row]
        with np.errstate(all="ignore"):
            self.bounds = lr.bounds(self.t, self.x, self.M, self.err, self.mask, self.c)
        self.eps = lr.eps(self.t, self.M, self.err, self.mask)       # [S][n][n]
        for a in (self.rows, self.M, self.x):
            a.setflags(write=False)

    def vec(self, v):
        """(x, eps) of another vector."""
        M = lr.models(v, self.n, self.nsrc)
        t, x = lr.deviance(M, self.D, self.err, self.mask)
        delta_from = np.concatenate([self.M, M])
        return x[0], lr.eps(t, delta_from, self.err, self.mask)[0]


@functools.lru_cache(maxsize=None)
def reference(name, S, seed=0):
    img, nsrc, base = case(name)
    return Ref(img, nsrc, scatter(base, S, 1000 * len(name) + S + seed))


def sampler(name, mode="exact"):
    img, nsrc, _ = case(name)
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    s.set_eval_mode(mode)
    return s


STATE_KEYS = ("pivot", "a1", "a2", "m", "l", "best")


def same_state(a, b):
    return (a["n"] == b["n"] and a["n_bad"] == b["n_bad"]
            and all(np.array_equal(a[k], b[k], equal_nan=True) for k in STATE_KEYS))


def check_planes(img, ref, label, slack=1.0):
    """The five sample planes within their bounds (x slack where two paths are compared);
    prints and returns the largest ratio to each bound."""
    ok, worst = ref.ok, {}
    for k in ("mean_dev", "std_dev", "lppd", "p_waic", "elpd"):
        assert np.isnan(img[k][ref.mask]).all() and np.isfinite(img[k][ok]).all(), (label, k)
        d = np.abs(img[k][ok].astype(LD) - ref.planes[k][ok]).astype(np.float64)
        b = ref.bounds[k][ok] * slack
        worst[k] = float((d / b).max()) if np.all(b > 0) else float(d.max() == 0) - 1.0
        assert np.all(d <= b), (label, k, float((d / np.maximum(b, 1e-300)).max()))
    print(label, " ".join(f"{k} {v:.2e}" for k, v in worst.items()), "(x bound)")
    return worst


def check_totals(sc, img, ref, label, dev_best=None, dev_at=None, eps_best=None, eps_at=None):
    ok, N = ref.ok, int(ref.ok.sum())
    want = lr.scalars(ref.planes, ok, ref.rows.shape[1] - 1, dev_best, dev_at, ref.err)
    assert sc["samples"] == ref.rows.shape[0] and sc["pixels"] == N and sc["poisoned"] == 0
    out = {}
    for key, plane in (("lppd", "lppd"), ("p_waic", "p_waic"), ("elpd_waic", "elpd"),
                       ("mean_deviance", "mean_dev")):
        b = lr.total_bound(ref.bounds[plane], ref.planes[plane].astype(np.float64), ok)
        d = abs(float(LD(sc[key]) - want[key]))
        out[key] = d / b if b > 0 else 0.0
        assert d <= b, (label, key, d, b)
    assert sc["waic"] == -2.0 * sc["elpd_waic"]
    bmax = float(ref.bounds["elpd"][ok].max())
    bse = np.sqrt(N) * np.sqrt(N / (N - 1.0)) * bmax + N * U * float(want["se_elpd"])
    d = abs(float(LD(sc["se_elpd"]) - want["se_elpd"]))
    out["se_elpd"] = d / bse
    assert d <= bse, (label, "se_elpd", d, bse)
    near = int((np.abs(ref.planes["p_waic"][ok].astype(np.float64) - 0.4)
                <= ref.bounds["p_waic"][ok]).sum())
    assert abs(sc["p_waic_high"] - want["p_waic_high"]) <= near, (label, "p_waic_high")
    assert sc["reduced"] == sc["mean_deviance"] / (N - (ref.rows.shape[1] - 1))
    k = np.abs(np.log(ref.err[ok])) + 1.0
    assert abs(float(LD(sc["log_norm"]) - want["log_norm"])) <= 4 * U * k.sum() + N * U * k.sum()
    for key, x, e in (("deviance_best", dev_best, eps_best), ("deviance_at", dev_at, eps_at)):
        if x is not None:
            b = lr.total_bound(e, x.astype(np.float64), ok)
            d = abs(float(LD(sc[key]) - want[key]))
            out[key] = d / b if b > 0 else 0.0
            assert d <= b, (label, key, d, b)
    if dev_at is not None:
        assert sc["p_d"] == sc["mean_deviance"] - sc["deviance_at"]
        assert sc["dic"] == sc["deviance_at"] + 2.0 * sc["p_d"]
    print(label, "totals", " ".join(f"{k} {v:.2e}" for k, v in out.items()), "(x bound)")


@pytest.mark.parametrize("name", list(SYNTH))
def test_synthetic_rows_have_many_comparable_terms(name):
    """On the reference alone: at S = 257 every unmasked pixel's effective number of terms
    (sum e)^2 / sum e^2 is at least 16, the frame has masked pixels, mean chi^2 is about N
    and some pixel has p_waic > 0.4 -- the case cannot go degenerate unnoticed."""
    ref = reference(name, B + 1)
    e = np.exp(-(ref.x - ref.x.min(axis=0)) / 2)
    ess = (e.sum(axis=0) ** 2 / (e * e).sum(axis=0))[ref.ok]
    print(name, "smallest effective number of terms", float(ess.min()))
    assert ess.min() >= 16
    N = int(ref.ok.sum())
    assert ref.mask.sum() > 0
    assert 0.5 * N < float(ref.planes["mean_dev"][ref.ok].sum()) < 2.0 * N
    assert (ref.planes["p_waic"][ref.ok] > 0.4).any()


@pytest.mark.parametrize("name, S", PLANE_CASES)
def test_planes_and_totals_against_the_restatement(lib_loaded, name, S):
    ref = reference(name, S)
    rows = ref.rows
    theta = rows.mean(axis=0)
    with sampler(name) as s, Predictive(s) as p:
        p.fold_rows(rows)
        st = p.state()
        img, sc = p.images(theta), p.scalars(theta)
        best = p.best()
        pt = {k: p.point(v) for k, v in (("first", rows[0]), ("theta", theta), ("best", best))}
        plain = p.images()
    assert st["n"] == S and st["n_bad"] == 0 and np.array_equal(st["pivot"], rows[0])
    assert np.array_equal(best, rows[int(np.nanargmin(rows[:, -1]))])
    label = f"{name} S={S}"
    check_planes(img, ref, label)
    for k, v in (("first", rows[0]), ("theta", theta)):
        x, e = ref.vec(v)
        assert np.isnan(pt[k][ref.mask]).all()
        d = np.abs(pt[k][ref.ok].astype(LD) - x[ref.ok]).astype(np.float64)
        print(label, f"point({k})", float((d / e[ref.ok]).max()), "(x bound)")
        assert np.all(d <= e[ref.ok]), (label, k)
    # masked pixels are NaN in every plane; dev_best is point(best()), dev_at point(theta)
    for k, v in img.items():
        assert np.array_equal(np.isnan(v), ref.mask), k
    assert np.array_equal(img["dev_best"], pt["best"], equal_nan=True)
    assert np.array_equal(img["dev_at"], pt["theta"], equal_nan=True)
    assert np.isnan(plain["dev_at"]).all()
    for k in ("mean_dev", "std_dev", "lppd", "p_waic", "elpd", "dev_best"):
        assert np.array_equal(plain[k], img[k], equal_nan=True), k
    xb, eb = ref.vec(best)
    xa, ea = ref.vec(theta)
    check_totals(sc, img, ref, label, xb, xa, eb, ea)
    # the host arithmetic on the state gives the same planes
    host, hsc = predictive.planes_from_state(st, pt["first"], dev_best=pt["best"],
                                             dev_at=pt["theta"])
    check_planes(host, ref, label + " host")
    assert hsc["pixels"] == sc["pixels"] and hsc["poisoned"] == 0


@pytest.mark.parametrize("name", ["c64", "c64_3", "y64"])
def test_one_sample_is_exact(lib_loaded, name):
    """S = 1: lppd = -x / 2, no variance, and mean_dev, dev_best and point(row) are one
    plane; the sum of point(row) is the EXACT chi^2 of the row."""
    row = reference(name, 1).rows[0]
    mask = reference(name, 1).mask
    with sampler(name) as s, Predictive(s) as p:
        p.fold_rows(row[None])
        img = p.images()
        x = p.point(row)
        chi = s.chi_squared(row)
    ok = ~mask
    assert np.array_equal(np.isnan(x), mask)
    assert np.array_equal(img["lppd"][ok], -0.5 * x[ok])
    assert np.array_equal(img["p_waic"][ok], np.zeros(ok.sum()))
    assert np.array_equal(img["std_dev"][ok], np.zeros(ok.sum()))
    assert np.array_equal(img["mean_dev"], x, equal_nan=True)
    assert np.array_equal(img["dev_best"], x, equal_nan=True)
    assert np.array_equal(img["elpd"][ok], img["lppd"][ok])
    assert abs(float(x[ok].sum()) - chi) <= 1e-12 * chi


@pytest.mark.parametrize("name", ["c32", "s33", "c64", "c64_3", "c128_3"])
def test_best_row_and_its_plane(lib_loaded, name):
    """test_gpu_resid's construction: a NaN chi^2 placed first and two tied rows.  The best
    row is np.nanargmin's, the first of the tie, and dev_best is point(best()) bit for bit;
    the context's eval mode changes nothing."""
    rows = reference(name, B + 1).rows.copy()
    P = rows.shape[1] - 1
    rows[0, P] = np.nan
    k = int(np.nanargmin(rows[:, P]))
    tie = (k + 100) % (B + 1) if (k + 100) % (B + 1) != 0 else 5
    rows[tie, P] = rows[k, P]
    want = int(np.nanargmin(rows[:, P]))
    assert want == min(k, tie)
    with sampler(name) as s, Predictive(s) as p:
        p.fold_rows(rows)
        assert np.array_equal(p.best(), rows[want])
        img = p.images()
        assert np.array_equal(img["dev_best"], p.point(rows[want]), equal_nan=True)
        st = p.state()
        s.set_eval_mode("fast")
        with Predictive(s) as q:
            q.fold_rows(rows)
            assert same_state(st, q.state())
            for key, v in q.images().items():
                assert np.array_equal(v, img[key], equal_nan=True), key


def test_tile_heights_and_repeats(lib_loaded, monkeypatch):
    """Both tile heights give the same state under a caller's pivot, a sequence of folds
    repeats every bit, and another OLPE_LIK_ROWS is refused."""
    ref = reference("s33", 3 * B + 5)
    rows = ref.rows
    pivot = rows.mean(axis=0)
    states = []
    for h in ("4", "8", "8"):
        monkeypatch.setenv("OLPE_LIK_ROWS", h)
        with sampler("s33") as s, Predictive(s, pivot=pivot) as p:
            p.fold_rows(rows[:300])
            p.fold_rows(rows[300:])
            states.append(p.state())
    assert same_state(states[0], states[1]) and same_state(states[1], states[2])
    assert np.array_equal(states[0]["pivot"][:-1], pivot[:-1])
    monkeypatch.setenv("OLPE_LIK_ROWS", "16")
    with sampler("s33") as s:
        with pytest.raises(_lib.OlpeError) as e:
            Predictive(s)
        assert e.value.code == _lib.EINVAL and "OLPE_LIK_ROWS" in str(e.value)


def test_unusable_rows(lib_loaded):
    """Rows with a NaN or inf parameter at block starts, ends and in runs change no bit of
    the state, and n_bad counts them."""
    good = reference("c64", 3 * B + 5).rows
    P = good.shape[1] - 1
    nan_row = np.full(P + 1, np.nan)
    inf_row = good[3].copy()
    inf_row[5] = np.inf
    ninf_row = good[4].copy()
    ninf_row[0] = -np.inf
    rows, at = list(good), [0, B - 1, B, B + 1, 2 * B - 1, 2 * B, 600, 601, 602, 603]
    for i, k in enumerate(at):                      # ascending: positions in the final array
        rows.insert(k, (nan_row, inf_row, ninf_row)[i % 3])
    rows = np.stack(rows + [nan_row, inf_row])      # and the very end
    with sampler("c64") as s, Predictive(s) as a, Predictive(s) as b, Predictive(s) as c:
        a.fold_rows(rows)
        b.fold_rows(good)
        sa, sb = a.state(), b.state()
        assert sa["n"] == sb["n"] == 3 * B + 5 and sa["n_bad"] == len(at) + 2
        sb["n_bad"] = sa["n_bad"]
        assert same_state(sa, sb)
        assert a.scalars()["n_bad"] == len(at) + 2
        c.fold_rows(np.stack([nan_row, inf_row]))
        assert c.state()["n"] == 0 and c.state()["n_bad"] == 2
        assert np.all(c.state()["m"] == np.inf) and np.all(c.state()["l"] == 0.0)
        with pytest.raises(_lib.OlpeError) as e:
            c.finalize()
        assert e.value.code == _lib.ESTATE and "no usable sample" in str(e.value)


def test_splits_and_merge_agree(lib_loaded):
    """Two uneven calls, two objects merged with add, and one whole fold: all within the
    bounds of the restatement and of one another; add refuses unequal pivots and an empty
    object adopts the incoming one; reset empties."""
    ref = reference("c64_3", 3 * B + 5)
    rows = ref.rows
    pivot = rows[0]
    cut = B + 77
    with sampler("c64_3") as s, Predictive(s, pivot) as one, Predictive(s, pivot) as two, \
            Predictive(s, pivot) as a, Predictive(s, pivot) as b, Predictive(s) as empty, \
            Predictive(s, rows[1]) as other:
        one.fold_rows(rows)
        two.fold_rows(rows[:cut])
        two.fold_rows(rows[cut:])
        a.fold_rows(rows[:cut])
        b.fold_rows(rows[cut:])
        a.add(b.state())
        assert a.state()["n"] == 3 * B + 5 and np.array_equal(a.best(), one.best())
        imgs = {"whole": one.images(), "two calls": two.images(), "merged": a.images()}
        for k, img in imgs.items():
            check_planes(img, ref, k)
        for k in ("two calls", "merged"):
            for plane in ("mean_dev", "std_dev", "lppd", "p_waic", "elpd"):
                d = np.abs(imgs[k][plane] - imgs["whole"][plane])[ref.ok]
                r = float((d / (2 * ref.bounds[plane][ref.ok])).max())
                print(f"{k} against whole: {plane} {r:.2e} x twice the bound")
                assert r <= 1.0, (k, plane)
        other.fold_rows(rows[:3])
        with pytest.raises(_lib.OlpeError) as e:
            other.add(b.state())
        assert e.value.code == _lib.EINVAL and "pivot" in str(e.value)
        empty.add(one.state())
        assert same_state(empty.state(), one.state())
        for k, v in empty.images().items():
            assert np.array_equal(v, imgs["whole"][k], equal_nan=True), k
        empty.reset()
        st = empty.state()
        assert st["n"] == 0 and np.all(st["m"] == np.inf) and np.all(st["l"] == 0.0)
        with pytest.raises(_lib.OlpeError) as e:
            empty.finalize()
        assert e.value.code == _lib.ESTATE


@pytest.mark.parametrize("name, W, steps", [("c64", 7, (1, 1)), ("c64", 7, (3, 3)),
                                            ("c128_3", 5, (3, 1))])
def test_device_chain_equals_host_rows(lib_loaded, name, W, steps):
    """fold(sampler, row_step, walker_step) of rows placed as a launch's device chain: the
    same bits as fold_rows of that subset, walker-major.  Once per launch; reset allows the
    same launch again."""
    nrec = 41
    img, nsrc, base = case(name)
    chain = scatter(base, W * nrec, 17).reshape(W, nrec, -1)
    rs, ws = steps
    with sampler(name) as s, Predictive(s) as dev, Predictive(s) as host:
        with pytest.raises(_lib.OlpeError) as e:
            dev.fold(s)                                   # nothing launched yet
        assert e.value.code == _lib.ESTATE
        s.seed(np.arange(1, W + 1))
        s.test_chain_set(chain)
        dev.fold(s, row_step=rs, walker_step=ws)
        sub = chain[::ws, ::rs]
        host.fold_rows(sub)
        a, b = dev.state(), host.state()
        assert a["n"] == sub.shape[0] * sub.shape[1] and same_state(a, b)
        with pytest.raises(_lib.OlpeError) as e:
            dev.fold(s)                                   # the same launch twice
        assert e.value.code == _lib.ESTATE and "already folded" in str(e.value)
        dev.reset()
        dev.fold(s, row_step=rs, walker_step=ws)          # ... and again after a reset
        assert same_state(dev.state(), b)
        for bad in ((0, 1), (1, 0), (-2, 1)):
            with pytest.raises(_lib.OlpeError) as e:
                host.fold(s, *bad)
            assert e.value.code == _lib.EINVAL
    with sampler("c32") as small, sampler(name) as s, Predictive(s) as p:
        small.seed([1])
        small.test_chain_set(scatter(case("c32")[2], 3, 1).reshape(1, 3, -1))
        with pytest.raises(_lib.OlpeError) as e:
            p.fold(small)                                 # another side
        assert e.value.code == _lib.EINVAL and "side" in str(e.value)


def test_more_than_one_piece(lib_loaded):
    """The smallest input that crosses the piece cap at 64x64 (512 blocks of 256, from the
    plan test's restatement): the second piece starts at a block boundary, so one call and
    two calls cut there give the same bits; the mean is the weighted restatement's."""
    ref = reference("c64", 3 * B + 5)
    rows = ref.rows
    blocks, kb = lik_piece_blocks(64)
    piece = blocks * kb
    assert (blocks, kb) == (512, 256)
    total = piece + 1
    many = np.tile(rows, (-(-total // rows.shape[0]), 1))[:total].copy()
    many[piece, -1] = 1.0                                 # the best row is the second piece
    with sampler("c64") as s, Predictive(s) as a, Predictive(s) as b:
        a.fold_rows(many)
        b.fold_rows(many[:piece])
        b.fold_rows(many[piece:])
        sa = a.state()
        assert sa["n"] == total and same_state(sa, b.state())
        assert np.array_equal(sa["best"], many[piece])
        got = a.images()["mean_dev"]
    w = np.bincount(np.arange(total) % rows.shape[0], minlength=rows.shape[0]).astype(LD)
    want = np.tensordot(w / w.sum(), ref.x, axes=1)
    e = ref.eps.max(axis=0) + 2 * total * U * np.abs(ref.x - ref.c).max(axis=0).astype(float)
    d = np.abs(got[ref.ok].astype(LD) - want[ref.ok]).astype(np.float64)
    print("two pieces: mean_dev", float((d / e[ref.ok]).max()), "x bound")
    assert np.all(d <= e[ref.ok])


def test_an_overflowing_row_poisons_its_pixels(lib_loaded):
    """One row with an amplitude of 1e308 (and a narrow profile, so that its model reaches
    only part of the frame) among 300 good ones: where its t overflows the planes are NaN
    and counted, and the totals are the restatement's over the remaining pixels."""
    name = "y64"
    img, nsrc, base = case(name)
    rows = scatter(base, 301, 5)
    rows[150, 6] = 1e308                                  # amps
    rows[150, 10:14] = 0.5                                # both Gaussians half a pixel wide
    ref = Ref(img, nsrc, rows)
    with np.errstate(all="ignore"):
        x64 = ref.x.astype(np.float64)
        must = ref.ok & ~np.isfinite(x64).all(axis=0)
        may = ref.ok & (x64.max(axis=0) > 1e150)
    assert must.sum() > 0
    with sampler(name) as s, Predictive(s) as p:
        p.fold_rows(rows)
        img_, sc = p.images(), p.scalars()
        st, c_plane = p.state(), p.point(rows[0])
    gone = np.isnan(img_["elpd"]) & ref.ok
    assert sc["poisoned"] == int(gone.sum()) > 0 and sc["pixels"] == int(ref.ok.sum())
    assert np.all(gone[must]) and not np.any(gone & ~may)
    left = ref.ok & ~gone
    assert left.sum() > 100
    for k in ("mean_dev", "std_dev", "lppd", "p_waic", "elpd", "dev_best"):
        assert np.array_equal(np.isnan(img_[k]), ~left), k
    # delta follows max|M_ref| = 1e308 here, so every bound below is infinite and those
    # checks hold trivially; what does bind: the NaN set above, and the device's totals
    # against the host arithmetic on the device's state over the same remaining pixels
    # (planes a few ulp apart, N additions in another order: 2 N u sum|.|)
    with np.errstate(over="ignore"):
        host, hsc = predictive.planes_from_state(st, c_plane)
    assert np.array_equal(np.isnan(host["elpd"]), ~left) and hsc["poisoned"] == sc["poisoned"]
    for key, plane in (("lppd", "lppd"), ("p_waic", "p_waic"), ("elpd_waic", "elpd"),
                       ("mean_deviance", "mean_dev")):
        tol = 2 * int(left.sum()) * U * float(np.abs(host[plane][left]).sum())
        print("poisoned: host", key, abs(sc[key] - hsc[key]) / tol, "x bound")
        assert abs(sc[key] - hsc[key]) <= tol, (key, sc[key], hsc[key])
    with np.errstate(all="ignore"):
        for k in ("mean_dev", "std_dev", "lppd", "p_waic", "elpd"):
            d = np.abs(img_[k][left].astype(LD) - ref.planes[k][left]).astype(np.float64)
            assert np.all(d <= ref.bounds[k][left]), k
        print("poisoned:", int(gone.sum()), "pixels gone,", int(left.sum()), "left,",
              int((left & np.isfinite(ref.bounds["elpd"])).sum()), "of them with finite bounds")
        for key, plane in (("lppd", "lppd"), ("p_waic", "p_waic"), ("elpd_waic", "elpd"),
                           ("mean_deviance", "mean_dev")):
            want = ref.planes[plane][left].sum()
            b = lr.total_bound(ref.bounds[plane], ref.planes[plane].astype(np.float64), left)
            d = abs(float(LD(sc[key]) - want))
            print("poisoned:", key, d / b, "x bound")
            assert d <= b, (key, d, b)


def test_compare_two_models_of_one_frame(lib_loaded, tmp_path):
    """Rows about the truth against rows about a vector whose companion amplitude is halved,
    on the same synthetic 64x64 frame.  From the restatement's numbers: the halved model
    predicts the image worse by more than 5 standard errors.  The device's d_elpd and se
    match the restatement's within the summed bounds; other data is refused."""
    img, nsrc, base = case("y64")
    S = B + 1
    ra = reference("y64", S)
    factor = 0.5
    while True:
        worse = base.copy()
        worse[7] *= factor                                # ampc
        rb = Ref(img, nsrc, scatter(worse, S, 77))
        ok = ra.ok
        d = (ra.planes["elpd"] - rb.planes["elpd"])[ok]
        N = int(ok.sum())
        d_elpd, se = d.sum(), np.sqrt(N * d.var(ddof=1))
        if d_elpd / se > 5:
            break
        factor *= 0.5
        assert factor > 1e-3
    print("restatement: d_elpd", float(d_elpd), "se", float(se), "factor", factor)
    assert d_elpd / se > 5
    paths = []
    for tag, ref in (("a", ra), ("b", rb)):
        with sampler("y64") as s, Predictive(s) as p:
            p.fold_rows(ref.rows)
            paths.append(str(tmp_path / f"{tag}_waic.npz"))
            p.save(paths[-1], theta_hat=ref.rows.mean(axis=0))
    c = predictive.compare(*paths)
    assert c["pixels"] == N
    bd = (lr.total_bound(ra.bounds["elpd"], ra.planes["elpd"].astype(np.float64), ok)
          + lr.total_bound(rb.bounds["elpd"], rb.planes["elpd"].astype(np.float64), ok))
    bmax = float((ra.bounds["elpd"] + rb.bounds["elpd"])[ok].max())
    bse = np.sqrt(N) * np.sqrt(N / (N - 1.0)) * bmax + N * U * float(se)
    print("compare: d_elpd", abs(float(LD(c["d_elpd"]) - d_elpd)) / bd, "se",
          abs(float(LD(c["se"]) - se)) / bse, "(x bound)")
    assert abs(float(LD(c["d_elpd"]) - d_elpd)) <= bd
    assert abs(float(LD(c["se"]) - se)) <= bse
    assert c["ratio"] > 5 and c["d_waic"] == pytest.approx(-2.0 * c["d_elpd"], rel=1e-12)
    z = predictive.load_npz(paths[0])
    assert int(z["nsrc"]) == 2 and int(z["bkgd_mode"]) == 0 and np.array_equal(z["mask"], ra.mask)
    assert same_state(predictive.state_of(z), {**predictive.state_of(paths[0])})
    z["data"] = z["data"] + 1.0
    with pytest.raises(ValueError, match="data"):
        predictive.compare(z, paths[1])


def test_cli_waic(tmp_path, lib_loaded, capsys):
    """apf_step3.py --waic on a small step-2 output: the npz, the three FITS files and the
    summary's entry; against itself d_elpd is 0; without the flag nothing changes."""
    d = tmp_path / "2014_test"
    path = synth.write_case(str(d), 32, 2)
    out = step2.main([path, "--walkers", "4", "--seed", "3", "--iters", "120", "--burn-in", "20",
                      "-q"])
    plain = step3.main([path, "sys", "-s", "4", "-q"])
    with open(out + "step3_summary.json", "rb") as f:
        before = f.read()
    assert "waic" not in plain and before == json.dumps(plain, indent=1).encode()
    capsys.readouterr()
    got = step3.main([path, "sys", "-s", "4", "--waic", "--waic-thin", "3"])
    text = capsys.readouterr().out
    assert "Folding pointwise deviance" in text and "WAIC" in text and "DIC" in text
    chains = step3.load_chains(out, 4, 1)
    rows = chains[::3].reshape(-1, 17)
    z = predictive.load_npz(out + "00001_waic.npz")
    assert int(z["scalar_samples"]) == rows.shape[0] and int(z["thin"]) == 3
    assert np.array_equal(z["best"], rows[int(np.nanargmin(rows[:, 16]))])
    img, _ = fitsio.getdata_header(path)
    ref = Ref(np.asarray(img), 2, rows)
    assert np.array_equal(z["mask"], ref.mask)
    check_planes({k: z[k] for k in predictive.PLANES}, ref, "cli")
    for suffix, key in (("meandev", "mean_dev"), ("elpd", "elpd"), ("pwaic", "p_waic")):
        back, _ = fitsio.getdata_header(out + f"00001_{suffix}.fits")
        assert np.array_equal(np.asarray(back, dtype=np.float64), z[key], equal_nan=True), suffix
    with open(out + "step3_summary.json") as f:
        saved = json.load(f)
    assert saved["waic"]["samples"] == rows.shape[0] and saved["waic"]["thin"] == 3
    assert saved["waic"]["waic"] == float(z["scalar_waic"])
    assert saved["waic"]["dic"] == float(z["scalar_dic"]) and np.isfinite(saved["waic"]["dic"])
    assert got["waic"]["file"] == out + "00001_waic.npz"
    assert {k: v for k, v in saved.items() if k != "waic"} == json.loads(before)
    os.replace(out + "00001_waic.npz", str(tmp_path / "other.npz"))
    step3.main([path, "sys", "-s", "4", "--waic", "--waic-thin", "3", "--waic-against",
                str(tmp_path / "other.npz")])
    text = capsys.readouterr().out
    line = [ln for ln in text.splitlines() if ln.strip().startswith("d_elpd")]
    assert line and line[0].split()[1] == "0", text
    with open(out + "step3_summary.json") as f:
        assert json.load(f)["waic"]["against"]["d_elpd"] == 0.0
