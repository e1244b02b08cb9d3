"""Per-context proposal widths (olpe_widths_set / olpe_widths_get, Sampler.set_widths).

The sampler reads its jump widths from a buffer of its context instead of the code
object's tables.  With the defaults nothing changes, bit for bit, on every sampler
instance; with other widths every accept decision is the oracle's with the same widths;
widths belong to a context, follow the stream's order, survive chunk hand-offs, and bad
ones are refused with the widths unchanged.

The oracle runs once per case (module cache) and serves both eval modes and both 64x64
workgroup sizes.
"""
import numpy as np
import pytest

from oracle import olpe_oracle as ora
from olpefit_amd import _lib
from test_gpu_desc_patch import (K, SAMPLERS, SEED0, _assert_equal, _final, _sampler, _set_env)
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu


def custom_widths(nsrc):
    """defaults x 4 on even parameter indices, x 0.25 on odd ones (exact in binary)."""
    w = np.array(ora.layout(nsrc)[1], dtype=np.float64)
    w[0::2] *= 4.0
    w[1::2] *= 0.25
    return w


def _launch(s, n_it=K):
    chain = s.run(n_it, burn_in=0, record_stride=1, accept_min=3)
    return (chain, s.trace(n_it)) + _final(s)


# -- 1. defaults ------------------------------------------------------------------------
def test_default_widths_are_the_oracles(golden, lib_loaded):
    for case, ref in (("c32", ora.WIDTHS_2), ("c64_3", ora.WIDTHS_3)):
        s = _sampler(golden(case), "fast", 0, 2)
        got = s.get_widths()
        assert got.dtype == np.float64 and got.shape == ref.shape
        assert np.array_equal(got.view(np.uint64), np.asarray(ref, np.float64).view(np.uint64))
        s.close()


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_default_widths_change_nothing(golden, lib_loaded, monkeypatch, sampler, mode):
    case, W, env = SAMPLERS[sampler]
    _set_env(monkeypatch, env)
    g = golden(case)
    nsrc = int(g["nsrc"])
    s = _sampler(g, mode, 0, W)
    base = _launch(s)
    s.close()
    assert np.any(base[1][:, :, 5] > 0.5) and np.any(base[1][:, :, 5] < 0.5)
    s = _sampler(g, mode, 0, W)
    s.set_widths(np.array(ora.layout(nsrc)[1]))
    _assert_equal(base, _launch(s))
    s.close()
    s = _sampler(g, mode, 0, W)
    s.set_widths(custom_widths(nsrc))
    s.set_widths(None)
    _assert_equal(base, _launch(s))
    s.close()


# -- 2. custom widths against the oracle -------------------------------------------------
#          id            golden    env                    walkers on the device, oracle walkers, iterations
CUSTOM = {"c32": ("c32", {}, 2, 2, 600),
          "c64-wpb12": ("c64", {"OLPE_WPB": "12"}, 2, 2, 300),
          "c64-wpb16": ("c64", {"OLPE_WPB": "16"}, 2, 2, 300),
          "c64_3": ("c64_3", {}, 2, 2, 300),
          "c128_3-ring": ("c128_3", {}, 16, 1, 100)}
_ORACLE = {}


def _oracle_run(golden, case, nw, n_it):
    """(chain [n_it, PS], accepts [n_it]) of walkers SEED0 .. with the custom widths."""
    key = (case, nw, n_it)
    if key not in _ORACLE:
        g = golden(case)
        nsrc = int(g["nsrc"])
        dm, err, _, _ = ora.noise_model(g["image"], 1.0, 1, 1, 2)
        out = []
        for k in range(nw):
            w = ora.Walker(dm, err, g["p_init"], SEED0 + k, nsrc)
            w.widths = custom_widths(nsrc)
            chain, tr = w.run(n_it, trace=True)
            out.append((chain, np.array([t[4] for t in tr], dtype=bool)))
        _ORACLE[key] = out
    return _ORACLE[key]


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("cid", list(CUSTOM))
def test_custom_widths_match_the_oracle(golden, lib_loaded, monkeypatch, cid, mode):
    """Every accept decision is the oracle's with the same widths, and the rows agree
    within test_gpu_parity's trajectory tolerance for the mode (relative, with the same
    figure as the absolute floor for the parameters that pass through zero -- offsets and
    angles whose proposals are additive steps of order 1e-2 .. 1)."""
    from olpefit_amd.core import Sampler
    case, env, W, nw, n_it = CUSTOM[cid]
    _set_env(monkeypatch, env)
    g = golden(case)
    nsrc = int(g["nsrc"])
    s = Sampler(g["image"], 1.0, 1, 1, 2, nsrc=nsrc)
    s.set_eval_mode(mode)
    s.seed(SEED0 + np.arange(W))
    s.set_state(np.tile(g["p_init"], (W, 1)))
    s.set_widths(custom_widths(nsrc))
    s.enable_trace(True)
    chain = s.run(n_it, burn_in=0, record_stride=1)
    tr = s.trace(n_it)
    assert np.array_equal(s.get_widths(), custom_widths(nsrc))
    s.close()
    tol = TOL[mode]["traj"]
    for k, (ref_chain, ref_acc) in enumerate(_oracle_run(golden, case, nw, n_it)):
        frac = ref_acc.mean()
        print(f"{cid} {mode} walker {k}: accepted fraction {frac:.4f}, max rel row error "
              f"{np.max(np.abs(chain[k] - ref_chain) / np.maximum(np.abs(ref_chain), 1.0)):.3e}")
        assert 0.05 < frac < 0.95, (cid, k, frac)          # a condition on the inputs
        np.testing.assert_array_equal(tr[k, :, 5] > 0.5, ref_acc, err_msg=f"{cid} walker {k}")
        np.testing.assert_allclose(chain[k], ref_chain, rtol=tol, atol=tol,
                                   err_msg=f"{cid} walker {k}")


# -- 3. per context ------------------------------------------------------------------------
def test_widths_belong_to_a_context(golden, lib_loaded, monkeypatch):
    """Two samplers alive at once with different widths, their launches interleaved: each
    equals its solo run."""
    _set_env(monkeypatch, {})
    g = golden("c32")
    wa, wb = custom_widths(2), np.array(ora.WIDTHS_2) * 2.0
    solo = []
    for w in (wa, wb):
        s = _sampler(g, "fast", 0, 8)
        s.set_widths(w)
        rows = [s.run(40, burn_in=0, record_stride=1) for _ in range(3)]
        solo.append((np.concatenate(rows, axis=1),) + _final(s))
        s.close()
    a, b = _sampler(g, "fast", 0, 8), _sampler(g, "fast", 0, 8)
    a.set_widths(wa)
    b.set_widths(wb)
    rows = {a: [], b: []}
    for _ in range(3):
        a.run_async(40, 0, 1)
        b.run_async(40, 0, 1)
        for s in (a, b):
            s.sync()
            rows[s].append(s.chain())
    for s, ref in ((a, solo[0]), (b, solo[1])):
        got = (np.concatenate(rows[s], axis=1),) + _final(s)
        for name, x, y in zip(("chain", "state", "tries", "accepts", "mt", "gauss", "done_at"),
                              got, ref):
            np.testing.assert_array_equal(x, y, err_msg=name)
    assert not np.array_equal(solo[0][1], solo[1][1])      # the widths did matter
    a.close()
    b.close()


# -- 4. stream order -----------------------------------------------------------------------
def test_set_widths_follows_the_stream(golden, lib_loaded, monkeypatch):
    """run, set_widths, run with one sync at the end equals the same with a sync after
    every call; the first launch is the default-width one, the second is not."""
    _set_env(monkeypatch, {})
    g = golden("c64")
    w2 = custom_widths(2)
    n = 48

    def sequence(sync, widths=w2):
        s = _sampler(g, "fast", 0, 16)
        s.enable_trace(False)
        s.run_async(n)
        if sync:
            s.sync()
        mid = s.get_state() if sync else None
        if widths is not None:
            s.set_widths(widths)
        if sync:
            s.sync()
        s.run_async(n)
        s.sync()
        out = _final(s)
        got = s.get_widths()
        s.close()
        return out, mid, got
    one, _, w_one = sequence(False)
    each, mid, w_each = sequence(True)
    plain, mid_plain, _ = sequence(True, None)
    for x, y in zip(one, each):
        np.testing.assert_array_equal(x, y)
    assert np.array_equal(w_one, w2) and np.array_equal(w_each, w2)
    for x, y in zip(mid, mid_plain):                   # the first launch ran with the defaults
        np.testing.assert_array_equal(x, y)
    assert not np.array_equal(each[0], plain[0])       # the second did not


# -- 5. chunks -----------------------------------------------------------------------------
@pytest.mark.parametrize("case,env,W", [("c64", {"OLPE_WPB": "12"}, 13), ("c128_3", {}, 16)])
def test_chunks_run_with_the_contexts_widths(golden, lib_loaded, monkeypatch, case, env, W):
    g = golden(case)
    runs = {}
    for units in (1, 3):
        _set_env(monkeypatch, dict(env, OLPE_UNITS=str(units)))
        s = _sampler(g, "fast", 0, W)
        s.set_widths(custom_widths(int(g["nsrc"])))
        runs[units] = _launch(s)
        assert s.last_units() == units
        s.close()
    assert np.any(runs[1][4] > 0)
    _assert_equal(runs[1], runs[3])


# -- 6. rejected inputs --------------------------------------------------------------------
def test_bad_widths_are_refused_and_change_nothing(golden, lib_loaded):
    from olpefit_amd.core import OlpeError
    for case in ("c32", "c64_3"):
        g = golden(case)
        nsrc = int(g["nsrc"])
        s = _sampler(g, "fast", 0, 2)
        good = custom_widths(nsrc)
        s.set_widths(good)
        logp, lin = ora.layout(nsrc)[3][0], ora.layout(nsrc)[2][0]
        for j, v in ((0, np.nan), (3, 0.0), (5, -0.01), (1, np.inf), (logp, _lib.LOG_WIDTH_MAX * 1.01)):
            bad = good.copy()
            bad[j] = v
            with pytest.raises(OlpeError) as e:
                s.set_widths(bad)
            assert e.value.code == _lib.EINVAL, (j, v)
            assert np.array_equal(s.get_widths(), good)
        # the bound is the log-proposed parameters' alone, and is itself accepted
        ok = good.copy()
        ok[lin] = _lib.LOG_WIDTH_MAX * 4.0
        ok[logp] = _lib.LOG_WIDTH_MAX
        s.set_widths(ok)
        assert np.array_equal(s.get_widths(), ok)
        with pytest.raises(ValueError):
            s.set_widths(good[:-1])
        s.close()
