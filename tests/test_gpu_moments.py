"""The device moments fold (olpe_moments_accumulate, olpe_moments_summary: step 3's means,
sigmas and Gelman-Rubin numbers) against the long-double restatement of
tests/moments_restatement.py, on rows the tests choose.

Rows reach the device chain through the test hook olpe_test_chain_set
(``Sampler.test_chain_set``), as if a sampler launch had just recorded them; the image of
the context (an 8 x 8 synthetic cutout) plays no part in the fold.  Column k of walker w
holds offset[k] + scale[k] series_k(w, r) (``moments_restatement.chain_rows``): offsets 0,
+-30, 1e6, 1e9, scales 1e-3 .. 1, Gaussian / ramp / step / constant / spike / alternating
series, no two columns or walkers alike, the last column constant.

Every tolerance is derived (moments_restatement: |d mean| <= 4 n u A, |d M2| <= 4 n u (M2 +
A R), constant columns exact); none is taken from the device's output.  The tests print the
largest error / bound they meet.  tests/test_moments_cpu.py shows on the CPU that four
wrong variants of the fold break these bounds on these inputs.

Non-finite rows are out of scope: the sampler records none.
"""
import numpy as np
import pytest

import moments_restatement as mr

pytestmark = pytest.mark.gpu

LD = mr.LD
U = mr.U
LAUNCHES = (97, 5, 64, 150, 63, 1, 0, 2)
SINGLE = (1, 7, 8, 9, 47, 48, 49, 63, 64, 65, 95, 96, 97, 98, 99, 144, 145)
PS = {2: 17, 3: 20}


def make_sampler(nsrc, W=0):
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    img, _ = synth.make_image(8, nsrc, 0)
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    if W:
        s.seed(np.arange(11, 11 + W))
    return s


def fold(s, rows, launches):
    r = 0
    for n in launches:
        s.test_chain_set(rows[:, r:r + n])
        s.moments_accumulate()
        r += n
    assert r == rows.shape[1]
    return s.moments()


def equal_bits(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


@pytest.mark.parametrize("W", [1, 3, 4, 5, 15, 16, 37])
@pytest.mark.parametrize("nsrc", [2, 3])
def test_fold_within_bounds(lib_loaded, nsrc, W):
    """Both kernels in one accumulation (launches of 97, 150 and 64 rows by the wave per
    walker, 5, 63, 1 and 2 by the thread per column, one empty), 17 and 20 columns (lanes
    51 / 60 .. 63 idle), walker counts around the 4 waves of a block and the 256 threads of
    the column fold (W PS = 255, 272): every walker's mean and M2 within the bounds of the
    long-double reference, constant columns exact; the same launches on a fresh context
    give the same bits; the same rows as one launch stay within the bounds."""
    ps = PS[nsrc]
    rows = mr.chain_rows(W, sum(LAUNCHES), ps, seed=100 * nsrc + W)
    s = make_sampler(nsrc, W)
    got = fold(s, rows, LAUNCHES)
    np.testing.assert_array_equal(s.chain(), rows[:, -2:])        # the hook's last upload
    assert s.kernel_times(1)[0] >= 0.0                            # its events were recorded
    fm, fq = mr.check(*got, rows, what=("launches", nsrc, W))
    again = fold(make_sampler(nsrc, W), rows, LAUNCHES)
    equal_bits(got, again)
    fm1, fq1 = mr.check(*fold(make_sampler(nsrc, W), rows, (rows.shape[1],)), rows,
                        what=("one launch", nsrc, W))
    print(f"nsrc {nsrc} W {W}: mean err/bound {max(fm, fm1):.3g}, M2 err/bound {max(fq, fq1):.3g}")


@pytest.mark.parametrize("nsrc", [2, 3])
def test_fold_single_launch_lengths(lib_loaded, nsrc):
    """One launch of every length at which a kernel's blocks or row groups change shape:
    1 .. 9 and 47 .. 63 rows (blocks of 8, the last partial), 64 (the switch to the wave per
    walker), 95 .. 99 and 144, 145 (3 row groups of 16-row blocks: at 97 and 145 rows only
    row group 0 has a row in the new block)."""
    ps, W = PS[nsrc], 5
    s = make_sampler(nsrc, W)
    worst = [0.0, 0.0]
    for n in SINGLE:
        rows = mr.chain_rows(W, n, ps, seed=n)
        s.moments_reset()
        fm, fq = mr.check(*fold(s, rows, (n,)), rows, what=(nsrc, n))
        worst = [max(worst[0], fm), max(worst[1], fq)]
    print(f"nsrc {nsrc}: mean err/bound {worst[0]:.3g}, M2 err/bound {worst[1]:.3g}")


@pytest.mark.parametrize("nsrc", [2, 3])
def test_fold_many_walkers(lib_loaded, nsrc):
    """300 walkers (75 blocks of the wave fold, 20 / 24 of the column fold, the last partial),
    a short launch then a long one."""
    ps, W = PS[nsrc], 300
    rows = mr.chain_rows(W, 203, ps, seed=7)
    fm, fq = mr.check(*fold(make_sampler(nsrc, W), rows, (3, 200)), rows, what=nsrc)
    print(f"nsrc {nsrc}: mean err/bound {fm:.3g}, M2 err/bound {fq:.3g}")


@pytest.mark.parametrize("extra", [9, 70])
def test_checkpoint_form(lib_loaded, extra):
    """set_moments(n, mean, M2) on a second context, then one more hooked launch on both
    (9 rows: column fold, 70: wave fold): the same bits, and within the bounds over all
    rows."""
    W, ps = 5, 17
    rows = mr.chain_rows(W, sum(LAUNCHES) + extra, ps, seed=extra)
    s = make_sampler(2, W)
    n, mean, m2 = fold(s, rows[:, :sum(LAUNCHES)], LAUNCHES)
    t = make_sampler(2, W)
    t.set_moments(n, mean, m2)
    for x in (s, t):
        x.test_chain_set(rows[:, sum(LAUNCHES):])
        x.moments_accumulate()
    equal_bits(s.moments(), t.moments())
    mr.check(*s.moments(), rows, what=extra)


def test_refusals(lib_loaded):
    """A hooked launch cannot be folded twice; the hook before seed is a state error; a
    launch of no rows counts as a launch."""
    from olpefit_amd import _lib
    from olpefit_amd.core import OlpeError
    s = make_sampler(2)
    with pytest.raises(OlpeError) as e:
        s.test_chain_set(np.zeros((3, 4, 17)))
    assert e.value.code == _lib.ESTATE
    s.seed([1, 2, 3])
    with pytest.raises(OlpeError) as e:                  # no launch yet
        s.moments_accumulate()
    assert e.value.code == _lib.ESTATE
    rows = mr.chain_rows(3, 10, 17)
    for part in (rows, rows[:, :0]):
        s.test_chain_set(part)
        s.moments_accumulate()
        with pytest.raises(OlpeError) as e:
            s.moments_accumulate()
        assert e.value.code == _lib.ESTATE
    mr.check(*s.moments(), rows)
    assert s.count == 0                                  # the iteration count is untouched
    with pytest.raises(ValueError):
        s.test_chain_set(np.zeros((3, 4, 16)))


def test_hooked_launch_feeds_a_fold_object(lib_loaded):
    """The hook's launch is a launch to the *_fold_ctx entry points too: a corner object
    folds the hooked rows from the device chain once (a second fold of the same launch is
    refused) and counts what it counts from the same rows on the host."""
    from olpefit_amd.core import OlpeError
    from olpefit_amd.corner import Corner
    W, ps = 5, 17
    rows = mr.chain_rows(W, 70, ps, seed=3)
    s = make_sampler(2, W)
    s.test_chain_set(rows)
    ranges = Corner.ranges_of(rows)
    a, b = Corner(ranges, fine_bins=64), Corner(ranges, fine_bins=64)
    a.fold(s)
    with pytest.raises(OlpeError):
        a.fold(s)
    b.fold_rows(rows)
    ca, cb = a.counts(), b.counts()
    assert ca["n"] == cb["n"] == W * 70
    np.testing.assert_array_equal(ca["h1"], cb["h1"])
    np.testing.assert_array_equal(ca["h2"], cb["h2"])


# ---------------------------------------------------------------------------------------
# the summary kernels on uploaded per-walker pairs

@pytest.mark.parametrize("W", [1, 255, 256, 257, 300, 65537])
@pytest.mark.parametrize("nsrc", [2, 3])
def test_summary_sums(lib_loaded, nsrc, W):
    """olpe_moments_summary over adversarial per-walker pairs uploaded with set_moments (no
    chain): means 1e6 + 1e-3 normal in the even columns and O(1) in the odd ones, M2 over 12
    decades across walkers; W = 255 .. 257 and 300 around stage 1's 256 walkers per block (257:
    a last block of one walker), 65,537 = 257 stage-1 partials, so stage 2 takes its second
    loop iteration.  Against long-double sums of the uploaded values: |d sum mean| <= W u sum
    |mean|, |d sum M2| <= W u sum M2, |d D2| <= (W + 3) u D2 (centre and means are exact
    inputs; each term's difference, square and sum round once, the sums in trees no deeper
    than W); tries / accepts totals exact; without a centre the third block is exactly 0."""
    ps = PS[nsrc]
    np_ = ps - 1
    rng = np.random.RandomState(W + nsrc)
    mean = rng.normal(size=(W, ps))
    mean[:, ::2] = 1e6 + 1e-3 * mean[:, ::2]
    m2 = 10.0 ** rng.uniform(-6.0, 6.0, size=(W, ps))
    tries = rng.randint(0, 2 ** 31, size=(W, np_)).astype(np.float64)
    acc = np.floor(tries * rng.uniform(size=(W, np_)))
    s = make_sampler(nsrc, W)
    s.set_state(np.zeros((W, ps)), tries, acc)
    s.set_moments(100, mean, m2)
    lm, lq = mean.astype(LD), m2.astype(LD)
    centre = (lm.sum(axis=0, dtype=LD) / LD(W)).astype(np.float64)
    d2 = ((lm - centre.astype(LD)) ** 2).sum(axis=0, dtype=LD)
    out = s.moments_summary(centre)
    assert out[0] == 100 and out[1] == W
    e_mean = np.abs(out[2:2 + ps].astype(LD) - lm.sum(axis=0, dtype=LD))
    e_m2 = np.abs(out[2 + ps:2 + 2 * ps].astype(LD) - lq.sum(axis=0, dtype=LD))
    e_d2 = np.abs(out[2 + 2 * ps:2 + 3 * ps].astype(LD) - d2)
    b_mean = W * LD(U) * np.abs(lm).sum(axis=0, dtype=LD)
    b_m2 = W * LD(U) * lq.sum(axis=0, dtype=LD)
    b_d2 = (W + 3) * LD(U) * d2
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"nsrc {nsrc} W {W}: err/bound sum mean {float(np.max(e_mean / b_mean)):.3g}, "
              f"sum M2 {float(np.max(e_m2 / b_m2)):.3g}, "
              f"D2 {float(np.nanmax(np.where(b_d2 > 0, e_d2 / b_d2, 0))):.3g}")
    assert np.all(e_mean <= b_mean), (e_mean / b_mean)
    assert np.all(e_m2 <= b_m2), (e_m2 / b_m2)
    assert np.all(e_d2 <= b_d2), (e_d2, b_d2)
    np.testing.assert_array_equal(out[2 + 3 * ps:2 + 3 * ps + np_], tries.sum(axis=0))
    np.testing.assert_array_equal(out[2 + 3 * ps + np_:], acc.sum(axis=0))
    bare = s.moments_summary()
    assert np.array_equal(bare[2 + 2 * ps:2 + 3 * ps], np.zeros(ps))
    np.testing.assert_array_equal(bare[:2 + 2 * ps], out[:2 + 2 * ps])
    np.testing.assert_array_equal(bare[2 + 3 * ps:], out[2 + 3 * ps:])


# ---------------------------------------------------------------------------------------
# rows -> Gelman-Rubin

def test_gelman_rubin_end_to_end(lib_loaded):
    """Hooked rows (37 walkers, 379 rows in five launches, walker means 1e-3 apart about
    1e6) through the fold, the two-round summary and step3.summary_from_moments, against
    the Gelman-Rubin formulas of apf_step3.py:258-278 in long double over the rows.  std,
    gr_psrf and gr_rc within rel(sum M2) + rel(D2) + 16 u, where rel(sum M2) = the walkers' M2
    bounds summed over sum M2, plus W u, and rel(D2) = [2 sum_w |mean_w - c| (e_w + e_c) + W (e
    + e_c)^2] / D2 + (W + 3) u with e_w walker w's mean bound, e the largest, e_c = W u A the
    pooled centre's; the mean within e + e_c."""
    from olpefit_amd import step3
    W, launches, ps = 37, LAUNCHES[:5], 17
    N = sum(launches)
    rng = np.random.RandomState(5)
    sig = 10.0 ** rng.uniform(-3.0, -1.0, size=ps)
    rows = 1e6 + 1e-3 * rng.normal(size=(W, 1, ps)) + sig * rng.normal(size=(W, N, ps))
    rows[:, :, ps - 1] = 0.1 * (np.arange(W)[:, None] + 1)
    s = make_sampler(2, W)
    fold(s, rows, launches)
    got = step3.summary_from_moments(s.allreduce_moments(), nsrc=2)
    assert got["_rows_per_walker"] == N and got["_walkers"] == W
    x = rows.astype(LD)
    lm, lq = mr.reference(rows)
    bm, bq = mr.bounds(rows)
    A = np.abs(x).max(axis=(0, 1))
    c = lm.sum(axis=0, dtype=LD) / LD(W)                  # = np.mean(p): equal row counts
    d2 = ((lm - c) ** 2).sum(axis=0, dtype=LD)
    e_c = W * LD(U) * A
    e = bm.max(axis=0)
    worst = 0.0
    for k, name in enumerate(step3.NAMES_2[:-1]):
        rel_m2 = bq[:, k].sum(dtype=LD) / lq[:, k].sum(dtype=LD) + W * LD(U)
        rel_d2 = ((2 * (np.abs(lm[:, k] - c[k]) * (bm[:, k] + e_c[k])).sum(dtype=LD)
                   + W * (e[k] + e_c[k]) ** 2) / d2[k] + (W + 3) * LD(U))
        tol = float(rel_m2 + rel_d2 + 16 * LD(U))
        # apf_step3.py:262-276, N rows and M = W walkers, in long double
        Nf, M = LD(N), LD(W)
        w = (LD(1) / M) * (lq[:, k] / Nf).sum(dtype=LD)
        b = (Nf / (M - 1)) * d2[k]
        psrf = (((Nf - 1) / Nf) * w + ((M + 1) / (M * Nf)) * b) / w
        ref = {"std": np.sqrt((lq[:, k].sum(dtype=LD) + Nf * d2[k]) / (Nf * M)),
               "gr_psrf": psrf, "gr_rc": np.sqrt(((16 + 3) // (16 + 1)) * psrf)}
        for key, r in ref.items():
            err = float(abs(LD(got[name][key]) - r) / abs(r))
            worst = max(worst, err / tol)
            assert err <= tol, (name, key, err, tol)
    for k, name in enumerate(step3.NAMES_2):
        assert abs(LD(got[name]["mean"]) - c[k]) <= e[k] + e_c[k], name
    print(f"largest rel err / tolerance {worst:.3g}")


# ---------------------------------------------------------------------------------------
# the float64 image path of olpe_create

@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("nsrc", [2, 3])
def test_float64_image(lib_loaded, nsrc, mode):
    """OLPE_DTYPE_F64 in olpe_create.  A float64 copy of a float32 image, with the float32
    image's own noise terms (the Poisson term is computed in the image's precision), is the
    same context: chi_squared and a 60-iteration chain equal bit for bit.  A float64 image
    whose pixels no float32 holds follows the oracle's noise model and chi^2 on the float64
    array (a float32 rounding of the pixels would move chi^2 by about 1e-6 relative)."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler, noise_model
    from oracle import olpe_oracle as ora
    from test_gpu_parity import TOL
    n, W = 32, 5
    img32, truth = synth.make_image(n, nsrc, 0)
    p = np.append(truth, 0.0)
    mask, pois2, rn2, _, _ = noise_model(img32, 1.0, 1, 1, 2)
    chains = []
    for img in (img32, img32.astype(np.float64)):
        s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc, mask=mask, pois2=pois2, readnoise2=rn2)
        s.set_eval_mode(mode)
        chi = s.chi_squared(p)
        s.seed(np.arange(40, 40 + W))
        st = np.tile(p, (W, 1))
        st[:, -1] = chi
        s.set_state(st)
        chains.append((chi, s.run(60, burn_in=0, record_stride=1)))
    assert chains[0][0] == chains[1][0]
    assert np.array_equal(chains[0][1].view(np.uint64), chains[1][1].view(np.uint64))
    assert np.any(chains[0][1][:, 0] != chains[0][1][:, -1])            # the walkers moved
    m = synth.render(truth, n, nsrc)
    img64 = m + np.random.RandomState(1).normal(size=(n, n)) * np.sqrt(38.0 ** 2 + np.abs(m))
    assert np.any(img64 != img64.astype(np.float32))
    s = Sampler(img64, 1.0, 1, 1, 2, nsrc=nsrc)
    s.set_eval_mode(mode)
    dm, err, _, _ = ora.noise_model(img64, 1.0, 1, 1, 2)
    for q in (p, p * 1.01):
        ref = ora.chi_squared(dm, ora.build_analytical_model(q, n, nsrc), err)
        np.testing.assert_allclose(s.chi_squared(q), float(ref), rtol=TOL[mode]["chi"])
