"""The fold objects' hand-off between streams (olpefit_amd/csrc/olpe_fold.h): one object
folds a launch of one sampler, host rows on its own stream, then a launch of another
sampler, with no host synchronisation in between.  Each step must run behind the one
before it -- "an earlier fold on another context's stream included" -- or the state is
that of another order, or of rows not yet written.

The same three sets of rows folded from the host, in the same order, run the same kernels
on the same values: the comparison is as strict as each object's own device-chain test
(np.array_equal on counts, sums and sample bits).

Shapes: a 32x32 two-source frame, 67 walkers (no multiple of a wave, more than one block of
the per-walker kernels), launches of 3 and 65 rows and 5 host rows per walker.
"""
import json

import numpy as np
import pytest

from olpefit_amd import synth
from olpefit_amd.astrometry import Astrometry
from olpefit_amd.autocorr import Autocorr
from olpefit_amd.core import Sampler
from olpefit_amd.corner import Corner
from olpefit_amd.pipeline import initial_parameters
from olpefit_amd.residuals import Residuals

pytestmark = pytest.mark.gpu

W, N1, NA, N2 = 67, 3, 5, 65
ROWS = N1 + NA + N2


def walker_major(x):           # [W][rows][PS], as a launch's chain lies
    return x


def time_major(x):             # [rows][W][PS], as step 3's chains lie
    return np.ascontiguousarray(np.transpose(x, (1, 0, 2)))


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def make_corner(s, p0):
    rg = Corner.ranges_from_summary(p0, np.maximum(0.02 * np.abs(p0), 0.05), k=5.0)
    return Corner(rg, bins=20, fine_bins=2048)


def same_corner(a, b):
    a, b = a.counts(), b.counts()
    assert a["n"] == b["n"] == W * ROWS
    assert np.array_equal(a["h1"], b["h1"]) and np.array_equal(a["h2"], b["h2"])
    assert a["h2"].sum() > 0


def same_resid(a, b):
    sa, sb = a.state(), b.state()
    assert sa["n"] == sb["n"] == W * ROWS and sa["n_bad"] == sb["n_bad"] == 0
    for k in ("pivot", "s1", "s2", "best"):
        assert np.array_equal(sa[k], sb[k], equal_nan=True), k
    pa, pb = a.images(), b.images()
    for k in pa:
        assert np.array_equal(pa[k], pb[k], equal_nan=True), k


def same_acf(a, b):
    sa, sb = a.state(), b.state()
    assert (sa["n"], sa["series"], sa["skipped"]) == (sb["n"], sb["series"], sb["skipped"]) \
        == (W * ROWS, 3 * W, 0)
    assert np.array_equal(sa["C"], sb["C"])
    assert sa["C"][:, 0].max() > 0


def same_astrom(a, b):
    assert a.rows == b.rows == ROWS
    assert json.dumps(a.finalize(3.0)) == json.dumps(b.finalize(3.0))
    for x, y in zip(a.samples(0), b.samples(0)):
        assert x.shape == (ROWS, W) and np.array_equal(bits(x), bits(y))


# name -> (constructor(sampler, p0), the layout fold_rows takes, the comparison,
#          a check of the state after reset() and one more fold of 65 rows, or None)
OBJECTS = {
    "astrometry": (lambda s, p0: Astrometry(W, ROWS, pixscale=9.952, rotation_angle=15.0),
                   time_major, same_astrom, None),
    "corner": (make_corner, walker_major, same_corner,
               lambda d: d.counts()["n"] == W * N2),
    "residuals": (lambda s, p0: Residuals(s), walker_major, same_resid,
                  lambda d: d.state()["n"] == W * N2),
    "autocorr": (lambda s, p0: Autocorr(s.ps, 64), walker_major, same_acf,
                 lambda d: (d.state()["n"], d.state()["series"]) == (W * N2, W)),
}


@pytest.fixture(scope="module")
def samplers(lib_loaded):
    """Two samplers on one frame, 67 walkers each at the start vector, different seeds."""
    img, _ = synth.make_image(32, 2, 0)
    p0 = initial_parameters(img, synth.guess_values(32, 2), 2)
    with Sampler(img, 1.0, 1, 1, 2, nsrc=2) as s1, Sampler(img, 1.0, 1, 1, 2, nsrc=2) as s2:
        p0[-1] = s1.chi_squared(p0)
        p0.setflags(write=False)
        s1.seed(np.arange(1, W + 1))
        s2.seed(np.arange(1001, 1001 + W))
        yield s1, s2, p0


@pytest.mark.parametrize("name", list(OBJECTS))
def test_folds_of_two_samplers_and_host_rows_keep_their_order(samplers, name):
    s1, s2, p0 = samplers
    make, layout, same, after_reset = OBJECTS[name]
    A = np.tile(p0, (W, NA, 1))
    for s in (s1, s2):
        s.set_state(np.tile(p0, (W, 1)))
    with make(s1, p0) as dev, make(s1, p0) as host:
        assert s1.run_async(N1, 0, 1) == N1
        dev.fold(s1)                                  # behind s1's launch
        dev.fold_rows(layout(A))                      # own stream, behind the fold on s1's
        assert s2.run_async(N2, 0, 1) == N2
        dev.fold(s2)                                  # s2's stream, behind both
        s1.sync()
        s2.sync()
        chain1, chain2 = s1.chain(), s2.chain()
        assert chain1.shape == (W, N1, s1.ps) and chain2.shape == (W, N2, s2.ps)
        assert not np.array_equal(chain1, chain2[:, :N1])
        for rows in (chain1, A, chain2):
            host.fold_rows(layout(rows))
        same(dev, host)
        if after_reset is not None:
            dev.reset()
            dev.fold(s2)                              # forgotten with the state
            assert after_reset(dev)
