"""The sampler's model descriptor is patched per draw, not rebuilt.

Between Gibbs iterations the per-wave descriptor in LDS describes the walker's current
state; a draw rewrites only the fields its parameter feeds, and a rejected draw writes
them back from the state.  A launch of one iteration starts from the full build of the
unit prologue and ends before any patched field is read again, so K launches of one
iteration are the unpatched sampler: one launch of K iterations must equal them bit for
bit -- chains (stride 1), traces, states, tries, accepts, RNG and done_at.

The seeds and K below were chosen on the CPU with oracle/olpe_oracle.py (whose draws and
decisions the device reproduces) so that every run covers every parameter class with an
accept and a reject and the three orders of accept / reject that a stale field would
show in; each test asserts that coverage on the device's own trace.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 64
SEED0 = 7400
ENV_KNOBS = ("OLPE_UNITS", "OLPE_NO_QUEUE", "OLPE_WPB", "OLPE_RING")

# sampler instance -> (golden case, walkers, environment)
SAMPLERS = {
    "2src-64-wpb16": ("c64", 32, {"OLPE_WPB": "16"}),
    "2src-64-wpb12": ("c64", 32, {"OLPE_WPB": "12"}),
    "2src-32": ("c32", 32, {}),
    "3src-64": ("c64_3", 32, {}),
    "3src-128-ring": ("c128_3", 16, {}),         # >= 12 walkers: batches of 12, chunks
    "3src-128-few": ("c128_3", 7, {}),           # < 12 walkers: whole walkers
    "3src-128-global": ("c128_3", 16, {"OLPE_RING": "0"}),
}


def param_classes(nsrc):
    """{class name: parameter indices}: the fields of the descriptor a draw feeds
    (olpe_device.h, DescDeps and patch_desc)."""
    if nsrc == 2:
        c = {"x": (0, 2), "y": (1, 3), "DX": (4,), "DY": (5,), "amp": (6, 7), "RATIO": (8,),
             "OFF": (9,)}
        shapes = range(10, 16)
    else:
        c = {"x": (0, 2, 4), "y": (1, 3, 5), "DX": (6,), "DY": (7,), "amp": (8, 9, 10),
             "RATIO": (11,), "OFF": (12,)}
        shapes = range(13, 19)
    for k in shapes:
        c[f"shape{k}"] = (k,)
    return c


def coverage_gaps(nsrc, r, acc, bkgd_mode):
    """What a run [W, K] of drawn indices and accept flags misses of the coverage the
    launch-splitting test needs ([] = covered)."""
    classes = param_classes(nsrc)
    cls_of = {}
    for name, idx in classes.items():
        for k in idx:
            cls_of[k] = name
    if nsrc == 2 and bkgd_mode == 0:
        assert cls_of[12] == "shape12"           # Layout<2>::BG_QUIRK: sigma_x of the wide set
    names = sorted(classes)
    cid = np.vectorize(lambda k: names.index(cls_of[int(k)]))(r)
    gaps = []
    for j, name in enumerate(names):
        for flag, what in ((True, "accept"), (False, "reject")):
            if not np.any((cid == j) & (acc == flag)):
                gaps.append(f"no {what} of class {name}")
    a0, a1, c0, c1 = acc[:, :-1], acc[:, 1:], cid[:, :-1], cid[:, 1:]
    if not np.any(~a0 & (c0 != c1)):
        gaps.append("no reject followed by a draw of another class")
    if not np.any(a0 & ~a1 & (c0 == c1)):
        gaps.append("no accept followed by a reject of the same class")
    if not np.any(a0 & a1 & (c0 != c1)):
        gaps.append("no accept followed by an accept of another class")
    return gaps


def _sampler(g, mode, bkgd_mode, W, p0=None):
    from olpefit_amd.core import Sampler
    s = Sampler(g["image"], 1.0, 1, 1, 2, nsrc=int(g["nsrc"]), bkgd_mode=bkgd_mode)
    s.set_eval_mode(mode)
    p0 = np.array(g["p_init"] if p0 is None else p0, dtype=np.float64)
    p0[-1] = s.chi_squared(p0)                   # the start's chi^2 in this mode
    s.seed(SEED0 + np.arange(W))
    s.set_state(np.tile(p0, (W, 1)))
    s.enable_trace(True)
    return s


def _final(s):
    return s.get_state() + s.rng_state() + (s.done_at(),)


def _one_launch(g, mode, bkgd_mode, W, n_it, p0=None):
    s = _sampler(g, mode, bkgd_mode, W, p0)
    chain = s.run(n_it, burn_in=0, record_stride=1, accept_min=3)
    out = (chain, s.trace(n_it)) + _final(s)
    s.close()
    return out


def _split_launches(g, mode, bkgd_mode, W, n_it, p0=None):
    s = _sampler(g, mode, bkgd_mode, W, p0)
    rows, tr = [], []
    for _ in range(n_it):
        rows.append(s.run(1, burn_in=0, record_stride=1, accept_min=3))
        tr.append(s.trace(1))
    out = (np.concatenate(rows, axis=1), np.concatenate(tr, axis=1)) + _final(s)
    s.close()
    return out


def _assert_equal(a, b):
    names = ("chain", "trace", "state", "tries", "accepts", "mt", "gauss", "done_at")
    for name, x, y in zip(names, a, b):
        np.testing.assert_array_equal(x, y, err_msg=name)


def _set_env(monkeypatch, env):
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("bkgd_mode", [0, 1])
@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_one_launch_equals_single_iteration_launches(golden, lib_loaded, monkeypatch, sampler,
                                                     mode, bkgd_mode):
    case, W, env = SAMPLERS[sampler]
    _set_env(monkeypatch, env)
    g = golden(case)
    whole = _one_launch(g, mode, bkgd_mode, W, K)
    tr = whole[1]
    gaps = coverage_gaps(int(g["nsrc"]), tr[:, :, 0].astype(int), tr[:, :, 5] > 0.5, bkgd_mode)
    assert not gaps, gaps
    _assert_equal(whole, _split_launches(g, mode, bkgd_mode, W, K))


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("case,env", [("c64", {"OLPE_WPB": "16"}), ("c64_3", {}),
                                      ("c128_3", {})])
def test_nan_proposals_patch_nothing(golden, lib_loaded, monkeypatch, case, env, mode):
    """A start whose log-normal background is below 0: every draw of it proposes NaN
    (the reference's log10 of a negative), which sweeps nothing, rejects, and must leave
    the descriptor as it is for the ordinary draws around it."""
    _set_env(monkeypatch, env)
    g = golden(case)
    nsrc = int(g["nsrc"])
    bg = 9 if nsrc == 2 else 12
    p0 = np.array(g["p_init"], dtype=np.float64)
    p0[bg] = -abs(p0[bg]) - 1.0
    W = 16
    whole = _one_launch(g, mode, 1, W, K, p0)
    tr = whole[1]
    r, nv, acc = tr[:, :, 0].astype(int), tr[:, :, 1], tr[:, :, 5] > 0.5
    assert np.all(np.isnan(nv[r == bg])) and not np.any(acc[r == bg])
    assert not np.any(np.isnan(nv[r != bg]))
    # NaN draws between ordinary ones, after accepts and after rejects
    nan0, nan1 = r[:, :-1] == bg, r[:, 1:] == bg
    assert np.any(nan0 & ~nan1) and np.any(~nan0 & nan1 & acc[:, :-1])
    assert np.any(~nan0 & nan1 & ~acc[:, :-1]) and np.any(acc[r != bg])
    _assert_equal(whole, _split_launches(g, mode, 1, W, K, p0))


@pytest.mark.parametrize("case,env", [("c64", {"OLPE_WPB": "16"}), ("c64", {"OLPE_WPB": "12"}),
                                      ("c128_3", {})])
def test_chunks_reestablish_the_descriptor(golden, lib_loaded, monkeypatch, case, env):
    """13 walkers cut into 3 and into 7 chunks: a chunk starts on another wave from the
    full build of the handed-over state, and equals the walker run whole."""
    g = golden(case)
    runs = {}
    for units in (1, 3, 7):
        _set_env(monkeypatch, dict(env, OLPE_UNITS=str(units)))
        s = _sampler(g, "fast", 0, 13)
        chain = s.run(K, burn_in=0, record_stride=1, accept_min=3)
        runs[units] = (chain, s.trace(K)) + _final(s)
        assert s.last_units() == units
        s.close()
    assert np.any(runs[1][4] > 0)                # some proposals were accepted
    _assert_equal(runs[1], runs[3])
    _assert_equal(runs[1], runs[7])
