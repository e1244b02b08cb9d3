"""The corner fold kernels (olpe_corner.hip) use no scratch: checked from the compiler's
resource usage, as test_kernel_resources does for the moment folds."""
from resource_usage import kernel_resources


def test_corner_fold_kernels_have_no_scratch():
    """Both lane layouts of the 2-D fold and the 1-D fold: no scratch, no spill, and few
    enough VGPRs for 8 waves per SIMD (the folds hide L2 and LDS-atomic latency with
    occupancy)."""
    res = kernel_resources("olpe_corner.hip")
    for kern, count in (("corner_fold1_kernel", 1), ("corner_fold2_kernel", 2)):
        hits = [v for k, v in res.items() if kern in k]
        assert len(hits) == count, (kern, list(res))
        for v in hits:
            assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (kern, v)
            assert v["VGPRs"] <= 64, (kern, v)
