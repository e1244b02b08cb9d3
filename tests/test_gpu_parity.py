"""GPU parity: the HIP path (through the C-ABI) against the golden fixtures produced by
the reference's own code and against the oracle on the same seeded inputs.

Tolerances (fp64):
* RNG streams (raw u32, rand, randint): bit-exact; polar gauss: same draws consumed
  (bit-exact stream position), deviates rel 3.2e-15 (ocml log vs glibc log).
* model pixels: |gpu - ref| <= 1e-13 * max|ref| (ocml exp/sin/cos vs NumPy's differ by
  <= 2 ulp; the per-pixel operation order is the reference's).
* chi^2: rel 1e-12 (summation order differs from NumPy's pairwise sum).
* trajectories: parameter index, dice and accept decision identical at every step;
  proposal, chi^2 and state rel 1e-10.  Flip criterion: an accept decision may only
  differ where |dice - p_accept| < 1e-9 * max(1, p_accept); none occurs in these runs.
* FAST evaluation (separable exp + cross-term recurrence): model pixels
  1e-12 * max|ref|, chi^2 rel 1e-11, trajectories as above with values rel 1e-9.
"""

MODES = ["exact", "fast"]
TOL = {"exact": dict(model=1e-13, chi=1e-12, traj=1e-10),
       "fast": dict(model=1e-12, chi=1e-11, traj=1e-9)}
import numpy as np
import pytest

from oracle import olpe_oracle as ora

pytestmark = pytest.mark.gpu

# *_nan: NaN / -inf / +inf data pixels, dropped by the reference's np.ma chi_squared
# (apf_step2.py:134-137; fixtures from make_golden.py ``nonfinite``)
CASES = ["c32", "c64", "c64_3", "c128_3", "c32_nan", "c64_nan", "c64_3_nan", "c128_3_nan"]


def make_sampler(g, mode="exact", **kw):
    from olpefit_amd.core import Sampler
    s = Sampler(g["image"], 1.0, 1, 1, 2, nsrc=int(g["nsrc"]), **kw)
    s.set_eval_mode(mode)
    return s


def test_rng_streams_bit_exact(golden, lib_loaded):
    g = golden("rng")
    img = golden("c32")
    s = make_sampler(img)
    seeds = g["seeds"].astype(np.uint32)
    s.seed(seeds)
    assert np.array_equal(s.rng_stream("raw", 1500), g["raw"].astype(np.uint32))
    s.seed(seeds)
    assert np.array_equal(s.rng_stream("rand", 400), g["unif"])
    s.seed(seeds)
    gs = s.rng_stream("gauss", 400)
    # the polar method's log() is ocml's, not glibc's: <= 1 ulp apart, so the deviates
    # agree to rounding; the draw COUNT (acceptance of the polar loop) is exact, which
    # the following raw draws prove.
    np.testing.assert_allclose(gs, g["gauss"], rtol=4e-16 * 8, atol=1e-300)
    print("gauss bit-exact fraction:", np.mean(gs == g["gauss"]))
    ref = [np.random.RandomState(int(x)) for x in seeds]
    for r in ref:
        r.standard_normal(400)
    tail = s.rng_stream("raw", 5)
    assert np.array_equal(tail, [r.randint(0, 2 ** 32, size=5, dtype=np.uint64) for r in ref])
    s.seed(seeds)
    assert np.array_equal(s.rng_stream("randint", 400), g["randint16"].astype(float))
    s3 = make_sampler(golden("c64_3"))
    s3.seed(seeds)
    assert np.array_equal(s3.rng_stream("randint", 400), g["randint19"].astype(float))


def test_rng_state_roundtrip(golden, lib_loaded):
    s = make_sampler(golden("c32"))
    s.seed([7, 8, 9])
    s.rng_stream("gauss", 3)                     # leaves a cached deviate
    mt, gc = s.rng_state()
    a = s.rng_stream("gauss", 50)
    s.set_rng_state(mt, gc)
    b = s.rng_stream("gauss", 50)
    assert np.array_equal(a, b)
    ref = np.random.RandomState(7)
    ref.standard_normal(3)
    np.testing.assert_allclose(a[0], ref.standard_normal(50), rtol=3.2e-15)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CASES)
def test_model_matches_reference(golden, lib_loaded, name, mode):
    g = golden(name)
    s = make_sampler(g, mode)
    for k, p in enumerate(g["params"]):
        m = s.build_analytical_model(p)
        ref = g["models"][k]
        err = np.max(np.abs(m - ref))
        assert err <= TOL[mode]["model"] * np.max(np.abs(ref)), (name, k, err)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CASES)
def test_chi2_matches_reference(golden, lib_loaded, name, mode):
    g = golden(name)
    s = make_sampler(g, mode)
    chi = s.chi_squared(g["params"])
    np.testing.assert_allclose(chi, g["chi2"], rtol=TOL[mode]["chi"])
    assert abs(s.chi_squared(g["p_init"]) - g["p_init"][-1]) <= TOL[mode]["chi"] * g["p_init"][-1]


def _check_traj(tr, g, w, L, name, rtol=1e-10):
    r, new, chi, dice, pacc, acc = (tr[w, :L, k] for k in range(6))
    np.testing.assert_array_equal(r.astype(int), g["traj_r"][w, :L], err_msg=name)
    np.testing.assert_array_equal(dice, g["traj_dice"][w, :L], err_msg=name)
    np.testing.assert_allclose(new, g["traj_new"][w, :L], rtol=rtol, err_msg=name)
    np.testing.assert_allclose(chi, g["traj_chi"][w, :L], rtol=rtol, err_msg=name)
    ref_acc = g["traj_acc"][w, :L]
    flips = np.nonzero(acc.astype(bool) != ref_acc)[0]
    for i in flips:      # documented flip criterion
        assert abs(dice[i] - pacc[i]) < 1e-9 * max(1.0, pacc[i]), (name, w, i)
    assert flips.size == 0, f"{name} walker {w}: accept flips at {flips[:5]}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CASES)
def test_trajectories_match_reference(golden, lib_loaded, name, mode):
    """Run the fused kernel from the reference's initial state with the reference's
    seeds and compare every iteration with the reference loop's own trace."""
    g = golden(name)
    s = make_sampler(g, mode)
    seeds = g["seeds"]
    s.seed(seeds)
    s.set_state(np.tile(g["p_init"], (len(seeds), 1)))
    s.enable_trace(True)
    L = int(g["traj_len"].max())
    chain = s.run(L, burn_in=0, record_stride=1)
    tr = s.trace(L)
    for w in range(len(seeds)):
        Lw = int(g["traj_len"][w])
        _check_traj(tr, g, w, Lw, name, TOL[mode]["traj"])
        np.testing.assert_allclose(chain[w, :Lw], g["traj_params"][w, :Lw],
                                   rtol=TOL[mode]["traj"])
        if mode == "fast":
            # the FAST log-normal proposal cur * e^(w g ln10) against the reference's of
            # the same step from the same current value (ratios new / cur where the states
            # already differ by rounding): 1e-14 relative, derived in
            # tests/test_gpu_fast_guards.py::test_seam_runs
            from probe_lib import lognormal_proposal_error
            r = tr[w, :Lw, 0].astype(int)
            i = np.arange(Lw)
            cur = np.vstack([g["p_init"][None], chain[w, :Lw - 1]])[i, r]
            ref_cur = np.vstack([g["p_init"][None], g["traj_params"][w, :Lw - 1]])[i, r]
            err, _ = lognormal_proposal_error(r, tr[w, :Lw, 1], cur, g["traj_new"][w, :Lw],
                                              ref_cur, ora.layout(int(g["nsrc"]))[3])
            assert err.size and err.max() <= 1e-14, (name, w, err.max())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["c32_nan", "c64_nan", "c64_3_nan", "c128_3_nan"])
def test_nonfinite_pixels_dropped_by_the_library(golden, lib_loaded, name, mode):
    """olpe_create drops NaN / -inf data pixels by itself: given only the reference's
    saturation mask (np.ma.masked_greater, apf_step2.py:188), which does not cover them,
    chi^2 still equals the reference's finite values."""
    from olpefit_amd.core import Sampler
    g = golden(name)
    s = Sampler(g["image"], 1.0, 1, 1, 2, nsrc=int(g["nsrc"]), mask=g["mask"])
    s.set_eval_mode(mode)
    chi = s.chi_squared(g["params"])
    assert np.all(np.isfinite(chi))
    np.testing.assert_allclose(chi, g["chi2"], rtol=TOL[mode]["chi"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fill", ["nan", "saturated"])
def test_all_masked_cutout_rejects_everything(golden, lib_loaded, mode, fill):
    """A cutout with no usable pixel (all NaN, or all above the saturation mask): the
    reference's np.ma sum is np.ma.masked, stored as NaN (apf_step2.py:289) and never
    accepted (:144); chi^2 is NaN here too and the trajectory (index, dice, no accept)
    equals the oracle's."""
    g = golden("c32")
    img = np.full((32, 32), np.nan if fill == "nan" else 1e6, np.float32)
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    p0 = g["p_init"].copy()
    with np.errstate(all="ignore"):
        w = ora.Walker(dm, err, p0, 17)
        w.init_chi2()
    assert np.isnan(w.parameters[-1])
    from olpefit_amd.core import Sampler
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=2)
    s.set_eval_mode(mode)
    assert np.isnan(s.chi_squared(p0))
    p0[-1] = np.nan
    s.seed([17])
    s.set_state(p0[None])
    s.enable_trace(True)
    chain = s.run(60, record_stride=1)
    tr = s.trace(60)
    with np.errstate(all="ignore"):
        ref, rtr = w.run(60, trace=True)
    np.testing.assert_array_equal(tr[0, :, 0].astype(int), [t[0] for t in rtr])
    np.testing.assert_array_equal(tr[0, :, 3], [t[3] for t in rtr])
    assert not np.any(tr[0, :, 5]) and not any(t[4] for t in rtr)
    np.testing.assert_array_equal(chain[0], ref)


@pytest.mark.parametrize("name", ["c32", "c64_3"])
def test_accept_min_done_at(golden, lib_loaded, name):
    """The reference loop ran until min(total_tries) >= accept_min (apf_step2.py:300):
    its iteration count is what olpe_done_at reports."""
    g = golden(name)
    s = make_sampler(g)
    s.seed(g["seeds"])
    s.set_state(np.tile(g["p_init"], (len(g["seeds"]), 1)))
    s.run(int(g["traj_len"].max()) + 50, record_stride=0, accept_min=int(g["accept_min"]))
    np.testing.assert_array_equal(s.done_at(), g["traj_len"])
    _, tries, acc = s.get_state()
    assert np.all(tries.sum(axis=1) == int(g["traj_len"].max()) + 50)


def test_split_launches_equal_one_launch(golden, lib_loaded):
    """State, counters, RNG and chain rows persist across launches (burn-in/stride
    bookkeeping of apf_step2.py:342 spans launches)."""
    g = golden("c32")
    seeds = np.arange(1000, 1006)
    a = make_sampler(g)
    a.seed(seeds)
    a.set_state(np.tile(g["p_init"], (6, 1)))
    ca = a.run(300, burn_in=37, record_stride=7)
    b = make_sampler(g)
    b.seed(seeds)
    b.set_state(np.tile(g["p_init"], (6, 1)))
    parts = [b.run(n, burn_in=37, record_stride=7) for n in (13, 100, 1, 186)]
    cb = np.concatenate([p for p in parts if p is not None], axis=1)
    np.testing.assert_array_equal(ca, cb)
    for x, y in zip(a.get_state(), b.get_state()):
        np.testing.assert_array_equal(x, y)
    assert a.count == b.count == 300


@pytest.mark.parametrize("mode", MODES)
def test_long_run_matches_oracle(golden, lib_loaded, mode):
    """4 walkers x 3000 iterations at 32x32 against the oracle (identical seeds):
    the full chains agree, so posterior means/sigmas agree to rounding."""
    g = golden("c32")
    dm, err, _, _ = ora.noise_model(g["image"], 1.0, 1, 1, 2)
    seeds = [11, 12, 13, 14]
    n_it = 3000
    s = make_sampler(g, mode)
    s.seed(seeds)
    s.set_state(np.tile(g["p_init"], (4, 1)))
    chain = s.run(n_it, burn_in=500, record_stride=1)
    for w, sd in enumerate(seeds):
        ref_chain, _ = ora.Walker(dm, err, g["p_init"], sd).run(n_it, burn_in=500)
        np.testing.assert_allclose(chain[w], ref_chain, rtol=10 * TOL[mode]["traj"], atol=1e-9)
    pos = chain[:, :, :4].reshape(-1, 4)
    assert np.all(np.isfinite(pos))


def test_long_run_64_fast_matches_oracle(golden, lib_loaded):
    """64x64 (the unrolled FAST3 row loop, the column-term and shape-table caches,
    accepts refreshing the caches): 2 walkers x 2500 iterations against the oracle."""
    g = golden("c64")
    dm, err, _, _ = ora.noise_model(g["image"], 1.0, 1, 1, 2)
    seeds = [21, 22]
    n_it = 2500
    s = make_sampler(g, "fast")
    s.seed(seeds)
    s.set_state(np.tile(g["p_init"], (2, 1)))
    s.enable_trace(True)
    chain = s.run(n_it, burn_in=0, record_stride=1)
    tr = s.trace(n_it)
    for w, sd in enumerate(seeds):
        ref_chain, ref_tr = ora.Walker(dm, err, g["p_init"], sd).run(n_it, trace=True)
        np.testing.assert_allclose(chain[w], ref_chain, rtol=10 * TOL["fast"]["traj"],
                                   atol=1e-9)
        assert np.array_equal(tr[w, :, 5] > 0.5, np.array([t[4] for t in ref_tr], bool))
    assert 0.05 < tr[:, :, 5].mean() < 0.95          # both outcomes exercised


def test_negative_log_parameter_is_always_rejected(golden, lib_loaded):
    """A log-normal parameter <= 0 proposes NaN (log10), which the reference always
    rejects (NaN chi^2 / masked sum, apf_step2.py:144); same trajectory as the oracle."""
    g = golden("c32")
    dm, err, _, _ = ora.noise_model(g["image"], 1.0, 1, 1, 2)
    p0 = g["p_init"].copy()
    p0[9] = -5.0
    with np.errstate(all="ignore"):
        p0[-1] = float(ora.chi_squared(dm, ora.build_analytical_model(p0, 32), err))
    s = make_sampler(g)
    s.seed([3])
    s.set_state(p0[None])
    s.enable_trace(True)
    chain = s.run(400, record_stride=1)
    tr = s.trace(400)
    w = ora.Walker(dm, err, p0, 3)
    ref, rtr = w.run(400, trace=True)
    assert np.all(chain[0, :, 9] == -5.0)
    np.testing.assert_array_equal(tr[0, :, 5].astype(bool), [t[4] for t in rtr])
    np.testing.assert_allclose(chain[0], ref, rtol=1e-10)


def test_fixed_background_mode(golden, lib_loaded):
    """bkgd_mode=1 fills the background with p[9] (apf_step2.py:126-132)."""
    g = golden("c32")
    s = make_sampler(g, bkgd_mode=1)
    for p in g["params"][:4]:
        ref = ora.build_analytical_model(p, 32, 2, bkgd_mode=1)
        m = s.build_analytical_model(p)
        assert np.max(np.abs(m - ref)) <= 1e-13 * np.max(np.abs(ref))


def test_errors_are_reported(golden, lib_loaded):
    from olpefit_amd.core import OlpeError, Sampler
    with pytest.raises(OlpeError):
        Sampler(np.zeros((8, 9), np.float32))           # non-square
    s = make_sampler(golden("c32"))
    with pytest.raises(OlpeError):
        s.run(10)                                        # not seeded


@pytest.mark.parametrize("case", ["c32", "c64_3"])
def test_rccl_single_rank_collectives(golden, lib_loaded, case):
    """RCCL communicator with one rank on the box's GPU: the all-gather returns the
    walker states and the all-reduced moment sums equal NumPy's over the chain.  c64_3:
    the 3-source layout (PS = 20 rows, OLPE_MOMENTS_LEN(20, 19)) through the same
    uniformity check and collectives (verdict r05 item 2: configs[4]'s exchange,
    3body/apf_step2_3body.py:381-400)."""
    from olpefit_amd.core import Sampler
    g = golden(case)
    s = make_sampler(g)
    s.seed(np.arange(50, 58))
    s.set_state(np.tile(g["p_init"], (8, 1)))
    chain = s.run(40, burn_in=0, record_stride=4)
    s.comm_init(Sampler.comm_unique_id(), 1, 0)
    # RCCL's own view of the communicator (ncclCommCount / ncclCommUserRank)
    assert s.comm_info() == (1, 0)
    st, _, _ = s.get_state()
    np.testing.assert_array_equal(s.allgather_state(), st)
    s.moments_accumulate()
    local = s.allreduce_moments()                        # one rank: this context alone
    ps = s.ps
    assert ps == (17 if int(g["nsrc"]) == 2 else 20) and local.size == 2 + 3 * ps + 2 * (ps - 1)
    mean = chain.mean(axis=1)                            # [W, PS]
    assert local[0] == chain.shape[1] and local[1] == 8
    np.testing.assert_allclose(local[2:2 + ps], mean.sum(axis=0), rtol=1e-12)
    np.testing.assert_allclose(local[2 + 2 * ps:2 + 3 * ps],
                               ((mean - mean.mean(axis=0)) ** 2).sum(axis=0), rtol=1e-9,
                               atol=1e-300)
    # chain concatenation, whole and range by range (bounded receive buffer)
    np.testing.assert_array_equal(s.allgather_chain()[0], chain)
    parts = [s.allgather_chain(w0, 3)[0] for w0 in (0, 3)] + [s.allgather_chain(6, 2)[0]]
    np.testing.assert_array_equal(np.concatenate(parts), chain)
    assert s.allgather_chain(2, 4, out=False) is None
    with pytest.raises(Exception):
        s.allgather_chain(6, 3)                          # past the last walker
    # the moments all-reduce over the communicator equals the local two-pass summary
    np.testing.assert_array_equal(s.allreduce_moments(), local)
    # a receive buffer this rank cannot allocate (over the gather limit) is OLPE_ENOMEM,
    # decided in the same all-reduce as the range check, so every rank returns it
    # instead of the others entering the gather (verdict r03 item 7)
    from olpefit_amd._lib import OlpeError
    s.gather_limit(2048)            # 1 walker x 10 rows x 136 / 160 B fits, 8 walkers do not
    with pytest.raises(OlpeError) as ei:
        s.allgather_chain()
    assert ei.value.code == -3 and "receive buffer" in str(ei.value)
    np.testing.assert_array_equal(s.allgather_chain(0, 1)[0], chain[:1])
    s.gather_limit(0)
    np.testing.assert_array_equal(s.allgather_chain()[0], chain)
    # the failure paths of the protocol (olpe_comm_proto.h; every step of every rank is
    # exercised on CPU by tests/test_comm_protocol.py), here through RCCL itself:
    # 1: the partials allocation fails -> OLPE_ENOMEM from the uniformity check
    s.moments_fault(1)
    with pytest.raises(OlpeError) as ei:
        s.allreduce_moments()
    assert ei.value.code == -3 and "partials" in str(ei.value)
    # 2: the summary launch fails after the check -> both rounds entered, this rank's error
    s.moments_fault(2)
    with pytest.raises(OlpeError) as ei:
        s.allreduce_moments()
    assert ei.value.code == -2 and "forced" in str(ei.value)
    # 3: the check words fail to reach the device -> the poisoned default is all-reduced
    # instead (every rank fails the check); the state and chain gathers too
    s.moments_fault(3)
    for call in (s.allreduce_moments, s.allgather_state, lambda: s.allgather_chain(0, 2)):
        with pytest.raises(OlpeError) as ei:
            call()
        assert ei.value.code == -2 and "check.send" in str(ei.value)
    # 4: round 1's sums fail to come back -> round 2 is still entered (as failed)
    s.moments_fault(4)
    with pytest.raises(OlpeError) as ei:
        s.allreduce_moments()
    assert ei.value.code == -2 and "r1.back" in str(ei.value)
    # ... and the communicator is still usable: the same results once cleared
    s.moments_fault(0)
    np.testing.assert_array_equal(s.allreduce_moments(), local)
    np.testing.assert_array_equal(s.allgather_state(), st)
    np.testing.assert_array_equal(s.allgather_chain()[0], chain)
    assert s.comm_info() == (1, 0)


def test_comm_calls_before_and_after_a_communicator(golden, lib_loaded):
    """Without olpe_comm_init the gathers are OLPE_ESTATE and comm_info has nothing to
    report; the moments summary is this context alone; olpe_comm_timeout validates its
    argument; a second olpe_comm_init replaces the communicator."""
    from olpefit_amd._lib import OlpeError
    from olpefit_amd.core import Sampler
    s = make_sampler(golden("c32"))
    s.seed(np.arange(4))
    s.set_state(np.tile(golden("c32")["p_init"], (4, 1)))
    for call in (s.comm_info, s.allgather_state, s.allgather_chain):
        with pytest.raises(OlpeError) as ei:
            call()
        assert ei.value.code == -4, call
    with pytest.raises(OlpeError):
        s.comm_timeout(-1.0)
    s.comm_timeout(30.0)
    for _ in range(2):
        s.comm_init(Sampler.comm_unique_id(), 1, 0)
        assert s.comm_info() == (1, 0)
        assert s.allgather_state().shape == (4, 17)


@pytest.mark.parametrize("skip", [1, 2, 3, 5, 619])
def test_rng_streams_misaligned(golden, lib_loaded, skip):
    """Draws that straddle a batch end or the key end (the draw tables' slow paths,
    DESIGN.md §3): after `skip` raw words the polar attempts (4 words) and rand()
    pairs (2 words) no longer align with the 624-word key, so some are assembled
    across the twist.  Same deviates as RandomState, and the same draw count (the raw
    tail is bit-exact)."""
    s = make_sampler(golden("c32"))
    seeds = np.array([4, 77, 2 ** 31 + 9], np.uint32)
    for kind in ("gauss", "rand"):
        s.seed(seeds)
        s.rng_stream("raw", skip)
        got = s.rng_stream(kind, 900)
        tail = s.rng_stream("raw", 3)
        for w, sd in enumerate(seeds):
            r = np.random.RandomState(int(sd))
            r.randint(0, 2 ** 32, size=skip, dtype=np.uint64)
            ref = r.standard_normal(900) if kind == "gauss" else r.random_sample(900)
            if kind == "gauss":
                np.testing.assert_allclose(got[w], ref, rtol=3.2e-15, atol=1e-300)
            else:
                assert np.array_equal(got[w], ref)
            assert np.array_equal(tail[w], r.randint(0, 2 ** 32, size=3, dtype=np.uint64))


def test_bench_size_walkers_match_oracle(lib_loaded):
    """BASELINE configs[2] at full size (65,536 walkers, 64x64 two-source synthetic
    cutout, FAST evaluation, the bench's seeds and start): a walker's chain does not
    depend on the ensemble around it, so sampled walkers equal the oracle run of their
    seeds; all chains stay finite."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    n, W, n_it = 64, 65536, 40
    img, _ = synth.make_image(n, 2, 0)
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    p0 = initial_parameters(img, synth.guess_values(n, 2), 2)
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=2)
    p0[-1] = s.chi_squared(p0)
    seeds = 1000 + np.arange(W)
    s.seed(seeds)
    s.set_state(np.tile(p0, (W, 1)))
    chain = s.run(n_it, burn_in=0, record_stride=4)
    assert chain.shape == (W, n_it // 4, s.ps) and np.all(np.isfinite(chain))
    for w in (0, 1, 4097, 31337, W - 1):
        ref, _ = ora.Walker(dm, err, p0, int(seeds[w])).run(n_it, record_stride=4)
        np.testing.assert_allclose(chain[w], ref, rtol=10 * TOL["fast"]["traj"], atol=1e-9)
    st, tries, acc = s.get_state()
    assert np.all(tries.sum(axis=1) == n_it) and np.all(acc <= tries)


def test_configs1_default_launch_matches_oracle(lib_loaded, monkeypatch):
    """BASELINE configs[1] at full size as bench.py --config 1 launches it: 4,096
    walkers, 64x64 two-source cutout, FAST, 100 iterations per launch at stride 10, two
    launches, the automatic launch shape (one round of the 16-wave sampler with
    progress balancing, whole walkers: DESIGN.md §3).  Sampled walkers -- the ends, the
    middle and one in each eighth of the queue (the persistent grid's workgroups go to
    the 8 XCDs round-robin, so these run on different XCDs) -- equal the oracle run of
    their seeds; every chain is finite and every walker made 200 tries."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    for k in ("OLPE_UNITS", "OLPE_NO_QUEUE", "OLPE_WPB", "OLPE_RING"):
        monkeypatch.delenv(k, raising=False)
    n, W = 64, 4096
    img, _ = synth.make_image(n, 2, 0)
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    p0 = initial_parameters(img, synth.guess_values(n, 2), 2)
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=2)
    p0[-1] = s.chi_squared(p0)
    seeds = 1000 + np.arange(W)
    s.seed(seeds)
    s.set_state(np.tile(p0, (W, 1)))
    parts = [s.run(100, burn_in=0, record_stride=10) for _ in range(2)]
    assert s.last_units() == 1
    chain = np.concatenate(parts, axis=1)
    assert chain.shape == (W, 20, s.ps) and np.all(np.isfinite(chain))
    picks = sorted({0, 1, W // 2 - 1, W - 1} | {k * (W // 8) + 255 for k in range(8)})
    for w in picks:
        ref, _ = ora.Walker(dm, err, p0, int(seeds[w])).run(200, record_stride=10)
        np.testing.assert_allclose(chain[w], ref, rtol=10 * TOL["fast"]["traj"], atol=1e-9,
                                   err_msg=f"walker {w}")
    st, tries, acc = s.get_state()
    assert np.all(tries.sum(axis=1) == 200) and np.all(acc <= tries)
    assert np.array_equal(st, chain[:, -1, :])


def test_configs1_survey_shape_matches_oracle(lib_loaded, monkeypatch):
    """configs[1] as SURVEY.md 8(d) specifies it and bench.py --config 1 now runs it:
    4,096 walkers, 1,000-iteration launches with the chain recorded every iteration
    (apf_step2.py:342-351) and each launch folded into the device moments.  Two
    launches: sampled walkers equal the oracle row for row over all 2,000 iterations, and
    every walker's device (mean, M2) equals NumPy's over its 2,000 rows."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    for k in ("OLPE_UNITS", "OLPE_NO_QUEUE", "OLPE_WPB", "OLPE_RING"):
        monkeypatch.delenv(k, raising=False)
    n, W = 64, 4096
    img, _ = synth.make_image(n, 2, 0)
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    p0 = initial_parameters(img, synth.guess_values(n, 2), 2)
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=2)
    p0[-1] = s.chi_squared(p0)
    seeds = 1000 + np.arange(W)
    s.seed(seeds)
    s.set_state(np.tile(p0, (W, 1)))
    parts = []
    for _ in range(2):
        parts.append(s.run(1000, burn_in=0, record_stride=1))
        s.moments_accumulate()
    chain = np.concatenate(parts, axis=1)
    assert chain.shape == (W, 2000, s.ps) and np.all(np.isfinite(chain))
    for w in (0, 1, W // 2 + 255, W - 1):
        ref, _ = ora.Walker(dm, err, p0, int(seeds[w])).run(2000, record_stride=1)
        np.testing.assert_allclose(chain[w], ref, rtol=10 * TOL["fast"]["traj"], atol=1e-9,
                                   err_msg=f"walker {w}")
    nrow, mean, m2 = s.moments()
    assert nrow == 2000
    np.testing.assert_allclose(mean, chain.mean(axis=1), rtol=1e-12, atol=1e-12)
    dev = chain - chain.mean(axis=1, keepdims=True)
    np.testing.assert_allclose(m2, (dev * dev).sum(axis=1), rtol=1e-8, atol=1e-12)
    st, tries, acc = s.get_state()
    assert np.all(tries.sum(axis=1) == 2000) and np.array_equal(st, chain[:, -1, :])


def test_bench_3source_128_matches_oracle(lib_loaded):
    """BASELINE configs[4]'s workload (3-source 128x128 synthetic cutout, FAST, the
    bench's seeds and start): the third source sits 32 px off-centre, so the whole-grid
    FAST3 guard fails and the per-column guard (fast3_ok_cols) admits FAST3; model and
    chi^2 at the start vector at the FAST tolerance against EXACT, and 3 walkers x 300
    iterations against the oracle run of their seeds."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    n, nsrc, n_it = 128, 3, 300
    img, _ = synth.make_image(n, nsrc, 0)
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
    with np.errstate(all="ignore"):
        ref_model = ora.build_analytical_model(p0, n, nsrc)
        p0[-1] = float(ora.chi_squared(dm, ref_model, err))
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    m = s.build_analytical_model(p0)
    assert np.max(np.abs(m - ref_model)) <= TOL["fast"]["model"] * np.max(np.abs(ref_model))
    assert abs(s.chi_squared(p0) - p0[-1]) <= TOL["fast"]["chi"] * p0[-1]
    W = 4096
    seeds = 1000 + np.arange(W)
    s.seed(seeds)
    s.set_state(np.tile(p0, (W, 1)))
    s.enable_trace(True)
    chain = s.run(n_it, burn_in=0, record_stride=3)
    tr = s.trace(n_it)
    assert np.all(np.isfinite(chain))
    for w in (0, 1777, W - 1):
        ref, rtr = ora.Walker(dm, err, p0, int(seeds[w]), nsrc=nsrc).run(n_it, record_stride=3,
                                                                         trace=True)
        np.testing.assert_allclose(chain[w], ref, rtol=10 * TOL["fast"]["traj"], atol=1e-9)
        assert np.array_equal(tr[w, :, 5] > 0.5, np.array([t[4] for t in rtr], bool))


def test_configs4_full_shard_matches_oracle(lib_loaded, monkeypatch):
    """configs[4]'s per-GPU shard at full size: 16,384 walkers (131,072 over 8 GPUs) on
    the 3-source 128x128 synthetic cutout, FAST, the bench's seeds, start and launch
    shape (100 iterations, stride 10; the automatic choice cuts each walker into 3
    chunks handed between waves).  Two launches; walkers spread over the shard
    (first, last, chunk-boundary neighbours) equal the oracle run of their seeds, every
    chain is finite and every walker tried 200 parameters."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    monkeypatch.delenv("OLPE_UNITS", raising=False)
    monkeypatch.delenv("OLPE_NO_QUEUE", raising=False)
    n, nsrc, W, n_it = 128, 3, 16384, 100
    img, _ = synth.make_image(n, nsrc, 0)
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    p0[-1] = s.chi_squared(p0)
    seeds = 1000 + np.arange(W)
    s.seed(seeds)
    s.set_state(np.tile(p0, (W, 1)))
    c1 = s.run(n_it, burn_in=0, record_stride=10)
    assert s.last_units() == 3
    c2 = s.run(n_it, burn_in=0, record_stride=10)
    chain = np.concatenate([c1, c2], axis=1)
    assert chain.shape == (W, 2 * n_it // 10, s.ps) and np.all(np.isfinite(chain))
    for w in (0, 5461, 5462, 10923, W - 1):
        ref, _ = ora.Walker(dm, err, p0, int(seeds[w]), nsrc=nsrc).run(2 * n_it, record_stride=10)
        np.testing.assert_allclose(chain[w], ref, rtol=10 * TOL["fast"]["traj"], atol=1e-9)
    st, tries, acc = s.get_state()
    assert np.all(tries.sum(axis=1) == 2 * n_it) and np.all(acc <= tries)
    s.close()


def test_walker_queue_equals_static_mapping(golden, lib_loaded, monkeypatch):
    """The persistent sampler hands walkers out from a device counter;
    with more walkers than resident waves (4,099 > 256 CUs x 16) some waves run two.
    Over three launches (the counter is never reset: each launch's base advances by
    W + its waves) every walker's chain, state, counters and RNG equal the static
    one-walker-per-wave mapping's bit for bit."""
    g = golden("c64")
    W = 4099
    seeds = 7000 + np.arange(W)
    out = []
    for no_queue in ("0", "1"):
        monkeypatch.setenv("OLPE_NO_QUEUE", no_queue)
        s = make_sampler(g, "fast")
        s.seed(seeds)
        s.set_state(np.tile(g["p_init"], (W, 1)))
        chains = [s.run(n, burn_in=0, record_stride=5) for n in (30, 45, 25)]
        out.append((chains, s.get_state(), s.rng_state()))
        s.close()
    (ca, sa, ra), (cb, sb, rb) = out
    for x, y in zip(ca, cb):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(sa + ra, sb + rb):
        np.testing.assert_array_equal(x, y)
    assert np.all(sa[1].sum(axis=1) == 100)


def _run_units(g, mode, W, seeds, units, no_queue="0", monkeypatch=None, trace=False,
               accept_min=0):
    monkeypatch.setenv("OLPE_NO_QUEUE", no_queue)
    monkeypatch.setenv("OLPE_UNITS", str(units))
    s = make_sampler(g, mode)
    s.seed(seeds)
    s.set_state(np.tile(g["p_init"], (W, 1)))
    s.enable_trace(trace)
    # launches whose chunk bounds, record rows and burn-in fall at odd places
    chains, traces, used = [], [], []
    for n, burn, stride in ((31, 7, 5), (45, 0, 4), (17, 60, 3)):
        chains.append(s.run(n, burn_in=burn, record_stride=stride, accept_min=accept_min))
        used.append(s.last_units())
        if trace:
            traces.append(s.trace(n))
    out = (chains, traces, s.get_state(), s.rng_state(), s.done_at(), used)
    s.close()
    return out


def _assert_same_run(a, b):
    for x, y in zip(a[0], b[0]):
        if x is None or y is None:
            assert x is None and y is None
        else:
            np.testing.assert_array_equal(x, y)
    for x, y in zip(a[1], b[1]):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(a[2] + a[3], b[2] + b[3]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a[4], b[4])


@pytest.mark.parametrize("mode,units", [("fast", 0), ("fast", 3), ("exact", 0)])
def test_sixteen_wave_sampler_equals_twelve(golden, lib_loaded, monkeypatch, mode, units):
    """The 2-source 64x64 samplers at 16 waves per workgroup (FAST: the default for
    launches of >= 8 rounds of walkers, e.g. configs[2]; one shape-table slot rebuilt in
    place, no shape-table prefetch.  EXACT: always; draw tables without the accept
    thresholds) compute what the 12-wave ones do: chains, traces, state, counters and
    RNG equal bit for bit over launches with odd bounds."""
    g = golden("c64")
    W = 4099 if mode == "fast" else 1031
    seeds = 9000 + np.arange(W)
    runs = []
    for wpb in ("12", "16"):
        monkeypatch.setenv("OLPE_WPB", wpb)
        runs.append(_run_units(g, mode, W, seeds, units, monkeypatch=monkeypatch, trace=True))
    _assert_same_run(*runs)
    assert np.any(runs[0][2][2] > 0)           # some proposals were accepted


@pytest.mark.parametrize("units", [0, 2, 3, 7])
def test_work_units_equal_whole_walkers(golden, lib_loaded, monkeypatch, units):
    """Walkers cut into chunks handed between waves (OLPE_UNITS): 4,099
    walkers (more than the 3,072 resident waves) over three launches give every
    chain row, trace entry, final state, counter, RNG state and done_at bit for bit
    equal to the static one-walker-per-wave mapping.  units = 0 is the automatic
    choice: 2 chunks for each of these launches (4,099 walkers fill 1 1/3 rounds of
    whole walkers, 2 2/3 of half walkers)."""
    g = golden("c64")
    W = 4099
    seeds = 9000 + np.arange(W)
    ref = _run_units(g, "fast", W, seeds, 0, "1", monkeypatch, trace=True, accept_min=4)
    got = _run_units(g, "fast", W, seeds, units, "0", monkeypatch, trace=True, accept_min=4)
    _assert_same_run(got, ref)
    assert got[5] == [units or 2] * 3
    assert ref[5] == [1, 1, 1]


@pytest.mark.parametrize("mode", MODES)
def test_work_units_few_walkers_spin(golden, lib_loaded, monkeypatch, mode):
    """13 walkers cut into 15 chunks: all 195 units are taken at once, so 182 waves
    wait on a hand-off -- every chunk's predecessor runs on another wave, often on
    another XCD.  Results equal whole walkers and the oracle."""
    g = golden("c32")
    W = 13
    seeds = 500 + np.arange(W)
    ref = _run_units(g, mode, W, seeds, 0, "1", monkeypatch)
    got = _run_units(g, mode, W, seeds, 15, "0", monkeypatch)
    _assert_same_run(got, ref)
    assert got[5] == [15, 15, 15]


def test_work_unit_handoff_timeout_is_reported(golden, lib_loaded, monkeypatch):
    """The hand-off wait's time-out path (unit_wait): with the limit forced down to one
    100 MHz tick (OLPE_WAIT_TICKS, a test hook), the waves of 13 walkers cut into 15
    chunks give up on their predecessors and the launch reports the time-out instead of
    returning results; the same launch under the launch's own bound (chunk-scaled, never
    below 30 s) completes with the whole-walker results."""
    g = golden("c32")
    W = 13
    seeds = 600 + np.arange(W)
    monkeypatch.setenv("OLPE_NO_QUEUE", "0")
    monkeypatch.setenv("OLPE_UNITS", "15")
    monkeypatch.setenv("OLPE_WAIT_TICKS", "1")
    s = make_sampler(g, "fast")
    s.seed(seeds)
    s.set_state(np.tile(g["p_init"], (W, 1)))
    with pytest.raises(Exception, match="hand-off timed out"):
        s.run(150, burn_in=0, record_stride=10)
    s.close()
    monkeypatch.delenv("OLPE_WAIT_TICKS")
    s = make_sampler(g, "fast")
    s.seed(seeds)
    s.set_state(np.tile(g["p_init"], (W, 1)))
    chain = s.run(150, burn_in=0, record_stride=10)
    assert s.last_units() == 15 and s.unit_stats()[0] > 0
    s.close()
    monkeypatch.setenv("OLPE_UNITS", "1")
    s = make_sampler(g, "fast")
    s.seed(seeds)
    s.set_state(np.tile(g["p_init"], (W, 1)))
    np.testing.assert_array_equal(s.run(150, burn_in=0, record_stride=10), chain)
    s.close()


def test_work_units_l2_sampler(lib_loaded, monkeypatch):
    """The 128x128 (L2-resident) sampler runs persistent only when it cuts walkers
    into chunks: chunks of 3 and of 5 equal its static mapping bit for bit."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    n, nsrc, W = 128, 3, 3100
    img, _ = synth.make_image(n, nsrc, 0)
    p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
    out = []
    for no_queue, units in (("1", 0), ("0", 3), ("0", 5)):
        monkeypatch.setenv("OLPE_NO_QUEUE", no_queue)
        monkeypatch.setenv("OLPE_UNITS", str(units))
        s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
        p0[-1] = s.chi_squared(p0)
        s.seed(2000 + np.arange(W))
        s.set_state(np.tile(p0, (W, 1)))
        c = s.run(40, burn_in=0, record_stride=3)
        out.append((c, s.get_state(), s.rng_state(), s.last_units()))
        s.close()
    assert [o[3] for o in out] == [1, 3, 5]
    for o in out[1:]:
        np.testing.assert_array_equal(o[0], out[0][0])
        for x, y in zip(o[1] + o[2], out[0][1] + out[0][2]):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("ring,units", [("12", 0), ("12", 1), ("12", 2), ("12", 7)])
def test_ring_sampler_equals_l2_sampler(lib_loaded, monkeypatch, ring, units):
    """The 128x128 lockstep sampler (12 waves per workgroup sharing an LDS ring of the
    cutout filled by LDS-DMA, olpe_device.h LdsRing) against the L2-resident
    sampler's static mapping: 1,001 walkers (a last batch with idle waves) over three launches
    whose chunk bounds, record rows and burn-in fall at odd places, with an accept_min
    stop -- chains, traces, final states, counters, RNG and done_at bit for bit equal."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    n, nsrc, W = 128, 3, 1001
    img, _ = synth.make_image(n, nsrc, 0)
    p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
    out = []
    for rg, no_queue, u in (("0", "1", 0), (ring, "0", units)):
        monkeypatch.setenv("OLPE_RING", rg)
        monkeypatch.setenv("OLPE_NO_QUEUE", no_queue)
        monkeypatch.setenv("OLPE_UNITS", str(u))
        s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
        p0[-1] = s.chi_squared(p0)
        s.seed(3000 + np.arange(W))
        s.set_state(np.tile(p0, (W, 1)))
        s.enable_trace(True)
        chains, traces = [], []
        for it, burn, stride in ((31, 7, 5), (45, 0, 4), (17, 60, 3)):
            chains.append(s.run(it, burn_in=burn, record_stride=stride, accept_min=4))
            traces.append(s.trace(it))
        out.append((chains, traces, s.get_state(), s.rng_state(), s.done_at()))
        s.close()
    (ca, ta, sa, ra, da), (cb, tb, sb, rb, db) = out
    for x, y in zip(ca + ta, cb + tb):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(sa + ra, sb + rb):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(da, db)


def test_ring_sampler_few_walkers_forced_units(lib_loaded, monkeypatch):
    """A lockstep batch must not hold a chunk and its predecessor (the chunk would wait
    for a wave that waits at the batch's barrier): with fewer walkers than a batch the
    ring sampler runs whole walkers even when chunks are forced -- 5 walkers with
    OLPE_UNITS=3 finish (no hand-off timeout) and equal the L2 sampler's run."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    n, nsrc, W = 128, 3, 5
    img, _ = synth.make_image(n, nsrc, 0)
    p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
    out = []
    for rg, no_queue in (("0", "1"), ("12", "0")):
        monkeypatch.setenv("OLPE_RING", rg)
        monkeypatch.setenv("OLPE_NO_QUEUE", no_queue)
        monkeypatch.setenv("OLPE_UNITS", "3")
        s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
        p0[-1] = s.chi_squared(p0)
        s.seed(4000 + np.arange(W))
        s.set_state(np.tile(p0, (W, 1)))
        c = s.run(60, burn_in=0, record_stride=3)
        out.append((c, s.get_state(), s.rng_state(), s.last_units()))
        s.close()
    assert out[1][3] == 1
    np.testing.assert_array_equal(out[0][0], out[1][0])
    for x, y in zip(out[0][1] + out[0][2], out[1][1] + out[1][2]):
        np.testing.assert_array_equal(x, y)


def test_work_units_automatic_choice(lib_loaded, monkeypatch):
    """Between one and eight rounds of the 12-wave sampler's 3,072 resident waves (4,300
    walkers, 64x64, 100 iterations) walkers are cut into chunks so that the rounds fill
    the slots; configs[1]'s 4,096 run whole as one round of the 16-wave sampler and
    configs[2]'s 65,536 whole at 16 waves."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    monkeypatch.delenv("OLPE_UNITS", raising=False)
    monkeypatch.delenv("OLPE_NO_QUEUE", raising=False)
    img, _ = synth.make_image(64, 2, 0)
    p0 = initial_parameters(img, synth.guess_values(64, 2), 2)
    got = {}
    for W in (4096, 4300, 65536):
        s = Sampler(img, 1.0, 1, 1, 2, nsrc=2)
        p0[-1] = s.chi_squared(p0)
        s.seed(1000 + np.arange(W))
        s.set_state(np.tile(p0, (W, 1)))
        s.run(100, burn_in=0, record_stride=10, read_chain=False)
        got[W] = s.last_units()
        s.close()
    assert got[4096] == 1 and got[65536] == 1 and got[4300] > 1, got


@pytest.mark.parametrize("n,nsrc,mode", [(40, 2, "fast"), (40, 2, "exact"), (48, 3, "fast"),
                                         (80, 2, "fast"), (96, 3, "fast"), (128, 2, "fast"),
                                         (24, 2, "fast"), (32, 3, "fast"), (32, 3, "exact"),
                                         (64, 3, "fast"), (256, 2, "fast"), (256, 3, "exact")])
def test_other_cutout_sizes_match_oracle(lib_loaded, n, nsrc, mode):
    """Cutout sides without a dedicated kernel (runtime-n LDS sampler for n <= ~72,
    global-memory sampler above; 128 with two sources; 256, where the FAST3 guard fails
    on the whole grid; n < 32 with several row groups per wave, n not dividing 64) and
    the 3-source 32x32 / 64x64 kernels on synthetic
    frames: model, chi^2 and 3 walkers x 300 iterations against the oracle."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    img, _ = synth.make_image(n, nsrc, 0)
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
    with np.errstate(all="ignore"):
        ref_model = ora.build_analytical_model(p0, n, nsrc)
        p0[-1] = float(ora.chi_squared(dm, ref_model, err))
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    s.set_eval_mode(mode)
    m = s.build_analytical_model(p0)
    assert np.max(np.abs(m - ref_model)) <= TOL[mode]["model"] * np.max(np.abs(ref_model))
    assert abs(s.chi_squared(p0) - p0[-1]) <= TOL[mode]["chi"] * p0[-1]
    seeds = [31, 32, 33]
    s.seed(seeds)
    s.set_state(np.tile(p0, (3, 1)))
    chain = s.run(300, burn_in=0, record_stride=2)
    for w, sd in enumerate(seeds):
        ref, _ = ora.Walker(dm, err, p0, sd, nsrc=nsrc).run(300, record_stride=2)
        np.testing.assert_allclose(chain[w], ref, rtol=10 * TOL[mode]["traj"], atol=1e-9)


@pytest.mark.parametrize("n,nsrc,mode", [(4, 2, "fast"), (5, 3, "fast"), (8, 2, "exact"),
                                         (17, 3, "fast"), (33, 2, "exact"), (65, 2, "fast"),
                                         (127, 3, "fast"), (129, 2, "fast")])
def test_ragged_cutout_sizes_match_oracle(lib_loaded, n, nsrc, mode):
    """Ragged sides: tiny cutouts (4 px, where the saturation mask leaves one pixel, and
    5 px: a few columns per row group, most lanes idle) and odd sides around the 32 / 64
    / 128 kernels (row groups that do not divide 64, one column past a pass).  The truth
    vector of the synthetic frame as the start (a step-1 guess needs a 10 x 10 sky box);
    model, chi^2 and 3 walkers x 200 iterations against the oracle."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    img, truth = synth.make_image(n, nsrc, 1)
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    p0 = np.append(truth, 0.0)
    with np.errstate(all="ignore"):
        ref_model = ora.build_analytical_model(p0, n, nsrc)
        p0[-1] = float(ora.chi_squared(dm, ref_model, err))
    assert np.isfinite(p0[-1])
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    s.set_eval_mode(mode)
    m = s.build_analytical_model(p0)
    assert np.max(np.abs(m - ref_model)) <= TOL[mode]["model"] * np.max(np.abs(ref_model))
    assert abs(s.chi_squared(p0) - p0[-1]) <= TOL[mode]["chi"] * p0[-1]
    seeds = [51, 52, 53]
    s.seed(seeds)
    s.set_state(np.tile(p0, (3, 1)))
    chain = s.run(200, burn_in=0, record_stride=2)
    for w, sd in enumerate(seeds):
        ref, _ = ora.Walker(dm, err, p0, sd, nsrc=nsrc).run(200, record_stride=2)
        np.testing.assert_allclose(chain[w], ref, rtol=10 * TOL[mode]["traj"], atol=1e-9)
    s.close()


def _random_states(n, nsrc, count, rs):
    """Parameter vectors far from the fit: sources anywhere on (and off) the cutout,
    narrow cores of 0.25-6 px and wide components 1-5x wider, any rotation, amplitudes
    over three decades, ratio and background over their ranges."""
    from olpefit_amd import synth
    truth = np.append(synth.truth_params(n, nsrc), 0.0)
    out = np.tile(truth, (count, 1))
    npos = 4 if nsrc == 2 else 6
    out[:, :npos] = rs.uniform(-0.2 * n, 1.2 * n, size=(count, npos))
    o = npos
    out[:, o:o + 2] = rs.uniform(-2.0, 2.0, size=(count, 2))                 # dx, dy
    amp = slice(o + 2, o + 2 + (nsrc))
    out[:, amp] = truth[amp] * 10 ** rs.uniform(-2, 1, size=(count, nsrc))
    r = o + 2 + nsrc
    out[:, r] = rs.uniform(0.0, 1.0, size=count)                             # ratio
    out[:, r + 1] = rs.uniform(1.0, 100.0, size=count)                       # bkgd
    sx = r + 2
    out[:, sx:sx + 2] = rs.uniform(0.25, 6.0, size=(count, 2))               # narrow
    out[:, sx + 2:sx + 4] = out[:, sx:sx + 2] * rs.uniform(1.0, 5.0, size=(count, 2))
    out[:, sx + 4:sx + 6] = rs.uniform(-np.pi, np.pi, size=(count, 2))       # thetas
    return out


@pytest.mark.parametrize("n,nsrc", [(64, 2), (64, 3), (128, 3), (33, 2)])
@pytest.mark.parametrize("mode", MODES)
def test_random_states_chi2_matches_oracle(golden, lib_loaded, n, nsrc, mode):
    """olpe_chi2_batch on 1,500 parameter vectors far from the fit (every FAST guard
    level and fallback the grid allows) against the oracle at the stated tolerances."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    img, _ = synth.make_image(n, nsrc, 2)
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    P = _random_states(n, nsrc, 1500, np.random.RandomState(n + nsrc))
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    s.set_eval_mode(mode)
    got = s.chi_squared(P)
    s.close()
    with np.errstate(all="ignore"):
        ref = np.array([float(ora.chi_squared(dm, ora.build_analytical_model(p, n, nsrc), err))
                        for p in P])
    fin = np.isfinite(ref)
    assert fin.sum() > 1000 and np.array_equal(np.isfinite(got), fin)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=TOL[mode]["chi"], atol=0)


@pytest.mark.parametrize("n,nsrc", [(64, 2), (64, 3), (128, 3)])
def test_random_states_sampler_proposals_match_oracle(golden, lib_loaded, n, nsrc):
    """The bench samplers' sweeps (64x64 LDS kernels, the 128x128 ring) from 1,024
    walkers at random states far from the fit: one traced iteration each, the
    proposal's chi^2 against the oracle's for the same vector (FAST tolerance)."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    img, _ = synth.make_image(n, nsrc, 2)
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    W = 1024
    P = _random_states(n, nsrc, W, np.random.RandomState(7 * n + nsrc))
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    s.set_eval_mode("fast")
    P[:, -1] = s.chi_squared(P)
    s.seed(np.arange(900, 900 + W))
    s.set_state(P)
    s.enable_trace(True)
    s.run(1, burn_in=0, record_stride=0)
    tr = s.trace(1)[:, 0, :]
    s.close()
    checked = 0
    for w in range(W):
        r, new, chi = int(tr[w, 0]), tr[w, 1], tr[w, 2]
        q = P[w].copy()
        q[r] = new
        with np.errstate(all="ignore"):
            ref = float(ora.chi_squared(dm, ora.build_analytical_model(q, n, nsrc), err))
        if not np.isfinite(ref):
            assert not np.isfinite(chi)
            continue
        assert abs(chi - ref) <= TOL["fast"]["chi"] * abs(ref), (w, r, chi, ref)
        checked += 1
    assert checked > 800


@pytest.mark.parametrize("n,nsrc,wpb", [(64, 2, "16"), (64, 2, "12"), (64, 3, "12"),
                                         (128, 2, "12"), (128, 3, "12"), (40, 2, "12")])
@pytest.mark.parametrize("mode", MODES)
def test_nan_proposals_rejected_without_sweep(lib_loaded, monkeypatch, n, nsrc, wpb, mode):
    """A background guessed below 0 (a sky box whose median is negative): every draw of
    it is a log-normal proposal of a negative value, NaN (apf_step2.py:66-69), which the
    reference rejects through its NaN chi^2.  The sampler skips the sweep for such
    proposals (in the 128x128 ring the wave only keeps the phases): the traced chi^2 is
    NaN on exactly those steps and the chains equal the oracle's."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    monkeypatch.setenv("OLPE_WPB", wpb)
    img, truth = synth.make_image(n, nsrc, 6)
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    p0 = np.append(truth, 0.0)
    bk = 9 if nsrc == 2 else 12
    p0[bk] = -3.5
    with np.errstate(all="ignore"):
        p0[-1] = float(ora.chi_squared(dm, ora.build_analytical_model(p0, n, nsrc), err))
    W, it = 16, 200
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    s.set_eval_mode(mode)
    seeds = np.arange(300, 300 + W)
    s.seed(seeds)
    s.set_state(np.tile(p0, (W, 1)))
    s.enable_trace(True)
    chain = s.run(it, burn_in=0, record_stride=1)
    tr = s.trace(it)
    s.close()
    nan_steps = 0
    for w in range(W):
        ref, rtr = ora.Walker(dm, err, p0, int(seeds[w]), nsrc=nsrc).run(it, trace=True)
        np.testing.assert_allclose(chain[w], ref, rtol=10 * TOL[mode]["traj"], atol=1e-9)
        drawn_bk = tr[w, :, 0] == bk
        assert np.all(np.isnan(tr[w, drawn_bk, 2])) and not np.any(tr[w, drawn_bk, 5] > 0.5)
        nan_steps += int(drawn_bk.sum())
    assert nan_steps > 0 and np.all(chain[:, :, bk] == -3.5)


@pytest.mark.parametrize("mode", MODES)
def test_mcds_header_noise_model_matches_oracle(lib_loaded, mode):
    """A frame read out in MCDS (sampmode 3: saturation scaled by multisam / itime,
    readnoise 38 / sqrt(multisam) x sqrt(coadds), apf_step2.py:182-204) with coadds 5:
    the library's chi^2 over the random-state vectors equals the oracle's."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    img, _ = synth.make_image(64, 2, 5)
    img = img * 4.0
    dm, err, _, _ = ora.noise_model(img, 30.0, 5, 8, 3)
    assert 0 < np.ma.count_masked(dm) < 100             # the star's peak saturates
    P = _random_states(64, 2, 200, np.random.RandomState(5))
    s = Sampler(img, 30.0, 5, 8, 3, nsrc=2)
    s.set_eval_mode(mode)
    got = s.chi_squared(P)
    s.close()
    with np.errstate(all="ignore"):
        ref = np.array([float(ora.chi_squared(dm, ora.build_analytical_model(p, 64, 2), err))
                        for p in P])
    np.testing.assert_allclose(got, ref, rtol=TOL[mode]["chi"], atol=0)


@pytest.mark.parametrize("n,nsrc", [(64, 2), (128, 3)])
def test_random_states_trajectories_match_oracle(golden, lib_loaded, n, nsrc):
    """48 walkers started at random states far from the fit, 150 iterations each
    through the bench sampler (FAST): as the chains move, steps pass between FAST3 and
    the fallback sweeps; every recorded state against the oracle's trajectory."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    img, _ = synth.make_image(n, nsrc, 3)
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    W, it = 48, 150
    P = _random_states(n, nsrc, W, np.random.RandomState(11 * n + nsrc))
    with np.errstate(all="ignore"):
        for p in P:
            p[-1] = float(ora.chi_squared(dm, ora.build_analytical_model(p, n, nsrc), err))
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    s.set_eval_mode("fast")
    seeds = np.arange(700, 700 + W)
    s.seed(seeds)
    s.set_state(P)
    chain = s.run(it, burn_in=0, record_stride=1)
    s.close()
    for w in range(W):
        ref, _ = ora.Walker(dm, err, P[w], int(seeds[w]), nsrc=nsrc).run(it)
        np.testing.assert_allclose(chain[w], ref, rtol=10 * TOL["fast"]["traj"], atol=1e-9,
                                   err_msg=f"walker {w}")


@pytest.mark.parametrize("n,nsrc,mode", [(1024, 2, "fast"), (900, 3, "exact"), (600, 2, "exact")])
def test_full_frame_cutouts_match_oracle(lib_loaded, n, nsrc, mode):
    """Frames far beyond the cutout sizes of the bench (a full 1024 x 1024 NIRC2 frame):
    the row tables of four waves no longer fit the LDS, so the sampler runs one-wave
    workgroups and the model / chi^2 kernel fewer vectors per workgroup; model, chi^2
    and 2 walkers x 24 iterations against the oracle (the reference evaluates the whole
    frame every proposal, apf_step2.py:94)."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    img, _ = synth.make_image(n, nsrc, 0)
    dm, err, _, _ = ora.noise_model(img, 1.0, 1, 1, 2)
    p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
    with np.errstate(all="ignore"):
        ref_model = ora.build_analytical_model(p0, n, nsrc)
        p0[-1] = float(ora.chi_squared(dm, ref_model, err))
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    s.set_eval_mode(mode)
    m = s.build_analytical_model(p0)
    assert np.max(np.abs(m - ref_model)) <= TOL[mode]["model"] * np.max(np.abs(ref_model))
    assert abs(s.chi_squared(p0) - p0[-1]) <= TOL[mode]["chi"] * p0[-1]
    seeds = [41, 42]
    s.seed(seeds)
    s.set_state(np.tile(p0, (2, 1)))
    chain = s.run(24, burn_in=0, record_stride=1)
    for w, sd in enumerate(seeds):
        ref, _ = ora.Walker(dm, err, p0, sd, nsrc=nsrc).run(24)
        np.testing.assert_allclose(chain[w], ref, rtol=10 * TOL[mode]["traj"], atol=1e-9)


@pytest.mark.parametrize("core", [(0.3, 0.3, 0.0), (0.3, 0.5, 0.7), (0.6, 0.45, -0.4)])
@pytest.mark.parametrize("wpb", ["12", "16"])
def test_sampler_fallback_sweeps_match_oracle(golden, lib_loaded, core, wpb, monkeypatch):
    """A tiny narrow core (sigma 0.3-0.6 px) fails the FAST3 guard (c S^2 (kc+1)^2 >=
    600), so the sampler's steps take the fallback sweeps inside the 64x64 kernel: the
    V-table (circular core, b = 0) or the exact per-pixel sweep (elongated, rotated
    core), interleaved with FAST3 steps when a proposal widens the core; the shape-table
    cache is invalidated when the V table overwrites it.  3 walkers x 400 iterations
    against the oracle at the FAST tolerance.  At 16 waves (one shape-table slot, no V
    table) the lvl-1 steps take the exact sweep and a rejected shape proposal leaves
    the slot stale."""
    monkeypatch.setenv("OLPE_WPB", wpb)
    g = golden("c64")
    dm, err, _, _ = ora.noise_model(g["image"], 1.0, 1, 1, 2)
    p0 = g["p_init"].copy()
    p0[10], p0[11], p0[14] = core
    with np.errstate(all="ignore"):
        p0[-1] = float(ora.chi_squared(dm, ora.build_analytical_model(p0, 64), err))
    s = make_sampler(g, "fast")
    assert abs(s.chi_squared(p0) - p0[-1]) <= TOL["fast"]["chi"] * p0[-1]
    seeds = [41, 42, 43]
    s.seed(seeds)
    s.set_state(np.tile(p0, (3, 1)))
    s.enable_trace(True)
    chain = s.run(400, burn_in=0, record_stride=1)
    tr = s.trace(400)
    for w, sd in enumerate(seeds):
        ref, rtr = ora.Walker(dm, err, p0, sd).run(400, trace=True)
        np.testing.assert_allclose(chain[w], ref, rtol=10 * TOL["fast"]["traj"], atol=1e-9)
        assert np.array_equal(tr[w, :, 5] > 0.5, np.array([t[4] for t in rtr], bool))


@pytest.mark.parametrize("n,nsrc", [(64, 2), (64, 3), (32, 2), (128, 3)])
def test_exact_sampler_chi2_bitwise_equals_eval(lib_loaded, n, nsrc):
    """The EXACT sampler's sweeps (the 64x64 2-source one with its LDS row tables,
    sweep_exact_rows; the others sweep_exact) perform the operations of the EXACT eval
    kernel (olpe_chi2_batch) on the same values: every recorded chain row's chi^2 equals
    olpe_chi2_batch of that row's parameters bit for bit."""
    from olpefit_amd import synth
    from olpefit_amd.core import Sampler
    from olpefit_amd.pipeline import initial_parameters
    W, n_it = 96, 60
    img, _ = synth.make_image(n, nsrc, 0)
    p0 = initial_parameters(img, synth.guess_values(n, nsrc), nsrc)
    s = Sampler(img, 1.0, 1, 1, 2, nsrc=nsrc)
    s.set_eval_mode("exact")
    p0[-1] = s.chi_squared(p0)
    s.seed(7000 + np.arange(W))
    s.set_state(np.tile(p0, (W, 1)))
    chain = s.run(n_it, burn_in=0, record_stride=3)
    rows = chain.reshape(-1, s.ps)
    acc = s.get_state()[2].sum()
    assert acc > 0 and np.all(np.isfinite(rows))
    np.testing.assert_array_equal(s.chi_squared(rows), rows[:, -1])
    s.close()


def test_one_shot_run_gibbs_c_abi(golden, lib_loaded):
    """olpe_run_gibbs (SURVEY.md §8(b)'s one-shot entry point, host buffers in and out)
    called through ctypes as INTEGRATION.md binds it: state, counters and chain equal
    the oracle's run of the same seeds (burn-in 40, every iteration recorded)."""
    import ctypes as C
    g = golden("c32")
    dm, err, _, _ = ora.noise_model(g["image"], 1.0, 1, 1, 2)
    s = make_sampler(g)
    W, n_it, burn = 3, 250, 40
    seeds = np.array([5, 6, 7], np.uint32)
    s.seed(seeds)
    state = np.ascontiguousarray(np.tile(g["p_init"], (W, 1)))
    tries = np.zeros((W, 16))
    accepts = np.zeros((W, 16))
    nrec = n_it - burn + 1
    chain = np.empty((W, nrec, 17))
    pd = C.POINTER(C.c_double)
    rc = lib_loaded.olpe_run_gibbs(s._ctx, state.ctypes.data_as(pd), tries.ctypes.data_as(pd),
                                   accepts.ctypes.data_as(pd), W, n_it, burn, 1,
                                   chain.ctypes.data_as(pd))
    assert rc == 0, lib_loaded.olpe_last_error()
    for w, sd in enumerate(seeds):
        walker = ora.Walker(dm, err, g["p_init"], int(sd))
        ref, _ = walker.run(n_it, burn_in=burn)
        np.testing.assert_allclose(chain[w], ref, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(state[w], ref[-1], rtol=1e-9)
    assert np.all(tries.sum(axis=1) == n_it) and np.all(accepts <= tries)


def test_fixed_background_trajectories_match_oracle(golden, lib_loaded):
    """bkgd_mode=1 (background = p[9], apf_step2.py:126-132, the build's --fixed-bkgd):
    2 walkers x 500 iterations of the sampler against the oracle in the same mode."""
    g = golden("c64")
    dm, err, _, _ = ora.noise_model(g["image"], 1.0, 1, 1, 2)
    p0 = g["p_init"].copy()
    with np.errstate(all="ignore"):
        p0[-1] = float(ora.chi_squared(dm, ora.build_analytical_model(p0, 64, 2, bkgd_mode=1),
                                       err))
    for mode in MODES:
        s = make_sampler(g, mode, bkgd_mode=1)
        s.seed([17, 18])
        s.set_state(np.tile(p0, (2, 1)))
        chain = s.run(500, burn_in=0, record_stride=1)
        for w, sd in enumerate([17, 18]):
            ref, _ = ora.Walker(dm, err, p0, sd, bkgd_mode=1).run(500)
            np.testing.assert_allclose(chain[w], ref, rtol=10 * TOL[mode]["traj"], atol=1e-9)


@pytest.mark.parametrize("mode", MODES)
def test_degenerate_runs(golden, lib_loaded, mode):
    """Edge cases of the loop bookkeeping (apf_step2.py:300-351): an empty ensemble is
    refused, a zero-iteration launch changes nothing, a launch that ends inside the
    burn-in records no rows, and a single walker / a walker count that fills no
    workgroup evenly (13) follow the oracle."""
    from olpefit_amd.core import OlpeError
    g = golden("c64")
    dm, err, _, _ = ora.noise_model(g["image"], 1.0, 1, 1, 2)
    s = make_sampler(g, mode)
    with pytest.raises(OlpeError):
        s.seed([])
    for seeds in ([7], list(range(40, 53))):
        s.seed(seeds)
        s.set_state(np.tile(g["p_init"], (len(seeds), 1)))
        before = s.get_state()
        assert s.run(0, burn_in=0, record_stride=1) is None
        for x, y in zip(before, s.get_state()):
            np.testing.assert_array_equal(x, y)
        assert s.count == 0
        assert s.run(50, burn_in=80, record_stride=1) is None      # inside the burn-in
        chain = s.run(70, burn_in=80, record_stride=3)             # rows at 80, 83, ..., 119
        assert chain.shape == (len(seeds), 14, 17) and s.count == 120
        for w in (0, len(seeds) - 1):
            ref, _ = ora.Walker(dm, err, g["p_init"], seeds[w]).run(120, burn_in=80,
                                                                     record_stride=3)
            np.testing.assert_allclose(chain[w], ref, rtol=10 * TOL[mode]["traj"], atol=1e-9)


def test_moments_fold_matches_numpy(golden, lib_loaded):
    """olpe_moments_accumulate over several launches (odd row counts, a launch with no
    rows, 300 walkers: two summary blocks) keeps every walker's running mean and M2 of
    all its recorded rows: equal to NumPy's two-pass values over the concatenated
    chain (mean rel 1e-13, M2 rel 1e-10); the summary sums, the pooled-centre
    deviations and the tries / accepts totals follow; a launch cannot be folded twice;
    get / set round-trips (checkpoints)."""
    from olpefit_amd import step3
    from olpefit_amd.core import OlpeError
    g = golden("c32")
    W = 300
    s = make_sampler(g, "fast")
    s.seed(np.arange(70, 70 + W))
    s.set_state(np.tile(g["p_init"], (W, 1)))
    parts = []
    for n in (57, 3, 1, 140):
        c = s.run(n, burn_in=20, record_stride=3)
        s.moments_accumulate()
        if c is not None:
            parts.append(c)
    with pytest.raises(OlpeError):
        s.moments_accumulate()
    chain = np.concatenate(parts, axis=1)               # [W, N, PS]
    n, mean, m2 = s.moments()
    assert n == chain.shape[1] == (201 - 20) // 3 + 1
    ref_mean = chain.mean(axis=1)
    ref_m2 = ((chain - ref_mean[:, None, :]) ** 2).sum(axis=1)
    np.testing.assert_allclose(mean, ref_mean, rtol=1e-13)
    # a column a walker never changed has M2 = 0 here and NumPy's rounding of its mean
    # squared otherwise: absolute slack n (10 eps |mean|)^2
    slack = n * (10 * np.finfo(float).eps * np.abs(ref_mean)) ** 2
    assert np.all(np.abs(m2 - ref_m2) <= 1e-10 * np.abs(ref_m2) + slack)
    # and within the derived bounds of the long-double reference, unchanged columns exact
    import moments_restatement as mr
    print("mean, M2 err / bound:", mr.check(n, mean, m2, chain))
    centre = ref_mean.mean(axis=0)
    summ = s.moments_summary(centre)
    ps, np_ = s.ps, s.np_
    _, tries, acc = s.get_state()
    assert summ[0] == n and summ[1] == W
    np.testing.assert_allclose(summ[2:2 + ps], ref_mean.sum(axis=0), rtol=1e-13)
    np.testing.assert_allclose(summ[2 + ps:2 + 2 * ps], ref_m2.sum(axis=0), rtol=1e-10)
    np.testing.assert_allclose(summ[2 + 2 * ps:2 + 3 * ps],
                               ((ref_mean - centre) ** 2).sum(axis=0), rtol=1e-9)
    np.testing.assert_array_equal(summ[2 + 3 * ps:2 + 3 * ps + np_], tries.sum(axis=0))
    np.testing.assert_array_equal(summ[2 + 3 * ps + np_:], acc.sum(axis=0))
    # step 3's statistics from the moments equal step3.summary over the chains
    got = step3.summary_from_moments(s.allreduce_moments(), nsrc=2)
    ref = step3.summary(chain.transpose(1, 0, 2), nsrc=2)
    for name, r in ref.items():
        for key in ("mean", "std", "gr_psrf", "gr_rc"):
            np.testing.assert_allclose(got[name][key], r[key], rtol=1e-12, err_msg=(name, key))
    # checkpoint round trip, then one more launch continues the same accumulation
    t = make_sampler(g, "fast")
    t.seed(np.arange(70, 70 + W))
    t.set_state(*s.get_state())
    t.set_rng_state(*s.rng_state())
    t.reset_count(s.count)
    t.set_moments(n, mean, m2)
    for x in (s, t):
        x.run(30, burn_in=20, record_stride=3)
        x.moments_accumulate()
    for a, b in zip(s.moments(), t.moments()):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", ["c32", "c64_3"])
def test_moments_fold_long_launches(golden, lib_loaded, name):
    """The one-wave-per-walker fold (launches of >= 64 rows per walker, round 4) beside
    the column fold (shorter ones), in one accumulation: launches of 97, 5, 64, 150 and
    63 rows (row counts that leave the wave's 3 row groups and 16-row blocks ragged), 2-
    and 3-source column counts (17, 20), 37 walkers (a last block of one wave).  Every
    walker's running mean and M2 equal NumPy's over the concatenated rows."""
    g = golden(name)
    W = 37
    s = make_sampler(g, "fast")
    s.seed(np.arange(500, 500 + W))
    s.set_state(np.tile(g["p_init"], (W, 1)))
    parts = []
    for n in (97, 5, 64, 150, 63):
        parts.append(s.run(n, burn_in=0, record_stride=1))
        s.moments_accumulate()
    chain = np.concatenate(parts, axis=1)
    nrow, mean, m2 = s.moments()
    assert nrow == chain.shape[1] == 379
    ref_mean = chain.mean(axis=1)
    ref_m2 = ((chain - ref_mean[:, None, :]) ** 2).sum(axis=1)
    np.testing.assert_allclose(mean, ref_mean, rtol=1e-13)
    slack = nrow * (10 * np.finfo(float).eps * np.abs(ref_mean)) ** 2
    assert np.all(np.abs(m2 - ref_m2) <= 1e-10 * np.abs(ref_m2) + slack)
    import moments_restatement as mr
    print("mean, M2 err / bound:", mr.check(nrow, mean, m2, chain))

