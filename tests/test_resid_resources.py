"""The residual-image kernels (olpe_resid.hip) use no scratch, and the fold kernels fit four
waves per SIMD: checked from the compiler's resource usage, as test_corner_resources does
for the corner folds."""
from resource_usage import kernel_resources


def test_resid_kernels_have_no_scratch_and_fit_four_waves():
    """Every kernel of the unit: ScratchSize 0, no VGPR spill.  The fold kernels (2 and 3
    sources x both tile heights) hold a tile's 2R accumulators in registers and still use
    at most 128 VGPRs: FP64-dense code needs the four waves per SIMD."""
    res = kernel_resources("olpe_resid.hip")
    for kern, count in (("resid_scan_kernel", 2), ("resid_book_kernel", 2),
                        ("resid_pivot_kernel", 2), ("resid_desc_kernel", 2),
                        ("resid_fold_kernel", 4), ("resid_reduce_kernel", 1),
                        ("resid_finalize_kernel", 2)):
        hits = [v for k, v in res.items() if kern in k]
        assert len(hits) == count, (kern, list(res))
        for v in hits:
            assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (kern, v)
            if kern == "resid_fold_kernel":
                assert v["VGPRs"] + v["AGPRs"] <= 128, (kern, v)
                assert v["Occupancy [waves/SIMD]"] >= 4, (kern, v)
