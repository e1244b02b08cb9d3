"""The kernels of the two sample-store objects (olpe_astrom.hip, olpe_phot.hip), the shared
stage-2 kernel (olpe_reduce.h) and the select kernels (olpe_select.h) included: no scratch,
no spill, and the occupancy they had before the block reductions were shared, checked from
the compiler's resource usage as test_acf_resources does."""
import pytest

from resource_usage import kernel_resources

# unit -> {kernel (as its mangled name holds it): waves / SIMD at the least}.  8 is the most a
# kernel of 64 VGPRs or fewer gets; phot_fold_kernel's 36 KB LDS tile allows four workgroups of
# four waves on a CU's 160 KiB.
KERNELS = {
    "olpe_astrom.hip": {"astrom_fold_kernelE": 8, "astrom_correct_kernelE": 8,
                        "astrom_reduce_stage1E": 8, "reduce_stage2_kernelILi256EE": 8,
                        "select_hist_kernelE": 8, "select_next_kernelE": 8},
    "olpe_phot.hip": {"phot_fold_kernelILi2EE": 4, "phot_fold_kernelILi3EE": 4,
                      "phot_reduce_stage1E": 8, "phot_reduce_stage2E": 8,
                      "select_hist_kernelE": 8, "select_next_kernelE": 8},
}


@pytest.mark.parametrize("unit", list(KERNELS))
def test_store_kernels_have_no_scratch_and_keep_their_occupancy(unit):
    res = kernel_resources(unit)
    assert len(res) == len(KERNELS[unit]), list(res)       # every kernel of the unit is named
    for kern, waves in KERNELS[unit].items():
        hits = [v for k, v in res.items() if kern in k]
        assert len(hits) == 1, (kern, list(res))
        v = hits[0]
        print(f"{unit} {kern}: {v}")
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (kern, v)
        assert v["Occupancy [waves/SIMD]"] >= waves, (kern, v)
