"""The 64-row FAST3 sweep, bit for bit.

sweep_fast3's fully unrolled 64-row path (olpe_device.h, NT = 64) takes the narrow
shape-table row from registers through a DPP broadcast inside the fma
(v_fmac_f64_dpp ... row_newbcast) instead of reading it from LDS: the same fmas on the
same operands, so every chain row, every traced chi^2 and every accept decision equals
what the sweep with two LDS reads per row computed.  tests/data/sweep_bits.json holds
that sweep's results (tools/record_sweep_bits.py, recorded once on the MI355X with the
library of the commit before the change); the cases are tests/sweep_bits_cases.py's:
the 12- and 16-wave 2-source samplers and the 3-source one from the step-1 style start,
and the 2-source ones on a frame with the sources at rows 2.3 and 61.7.
"""
import numpy as np
import pytest

import sweep_bits_cases as sb
from test_gpu_fast_guards import assert_follows_oracle, guard_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recording():
    return sb.load_recording()


@pytest.mark.parametrize("cid", list(sb.CASES))
def test_sweep_bits_equal_the_recording(lib_loaded, monkeypatch, recording, cid):
    """Chain, trace and final state equal the recording's; accepted and rejected shape
    proposals of both sets occurred (the in-place rebuild of the single table slot of
    the 16-wave sampler and its stale path, the two slots of the others); the edge
    cases also follow the oracle by test_gpu_fast_guards' criterion, which ties the
    recording to something other than the library it was made with."""
    nsrc, start, _ = sb.CASES[cid]
    p0 = sb.frame(nsrc, start)[3]
    assert guard_state(p0, sb.N, nsrc)["fast3"], "the start vector must take FAST3"
    chain, tr, state = sb.run_case(cid, monkeypatch.setenv,
                                   lambda k: monkeypatch.delenv(k, raising=False))
    oc = sb.shape_outcomes(nsrc, tr)
    print(f"SWEEP BITS {cid}: shape proposals {oc}")
    assert all(v >= 1 for v in oc.values()), oc
    if start == "edge":
        assert_follows_oracle(chain, tr, sb.oracle_run(nsrc, start))
    got, want = sb.digest(chain, tr, state), recording[cid]
    assert got["shape"] == want["shape"]
    assert got["final_state"] == want["final_state"]
    assert got["chain_sha256"] == want["chain_sha256"]
    assert got["trace_sha256"] == want["trace_sha256"]
