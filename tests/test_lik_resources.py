"""The pointwise-deviance kernels (olpe_lik.hip) use no scratch, and the fold kernels fit four
waves per SIMD: checked from the compiler's resource usage, as test_resid_resources does
for the residual folds."""
from resource_usage import kernel_resources


def test_lik_kernels_have_no_scratch_and_fit_four_waves():
    """Every kernel of the unit (the shared scan / book / desc kernels as this unit
    instantiates them included): ScratchSize 0, no VGPR spill.  The fold kernels (2 and 3
    sources x both tile heights) hold a tile's 4R accumulators in registers and still use
    at most 128 VGPRs: FP64-dense code needs the four waves per SIMD."""
    res = kernel_resources("olpe_lik.hip")
    for kern, count in (("resid_scan_kernel", 2), ("resid_book_kernel", 2),
                        ("lik_pivot_kernel", 2), ("resid_desc_kernel", 2),
                        ("lik_fold_kernel", 4), ("lik_reduce_kernel", 1),
                        ("lik_point_kernel", 2), ("lik_finalize_kernel", 2)):
        hits = [v for k, v in res.items() if kern in k]
        assert len(hits) == count, (kern, list(res))
    assert len(res) == 17, list(res)
    for kern, v in res.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (kern, v)
        if "lik_fold_kernel" in kern:
            assert v["VGPRs"] + v["AGPRs"] <= 128, (kern, v)
            assert v["Occupancy [waves/SIMD]"] >= 4, (kern, v)
