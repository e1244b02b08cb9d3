"""The detection-map kernels (olpe_detect.hip) use no scratch, and the correlation kernel fits
four waves per SIMD: checked from the compiler's resource usage, as test_resid_resources
does for the residual folds."""
from resource_usage import kernel_resources


def test_detect_kernels_have_no_scratch_and_fit_four_waves():
    """Every kernel of the unit: ScratchSize 0, no VGPR spill.  The fold kernel proper is the
    correlation (2 G n^2 FMAs per sample, a wave's 2 kR accumulators in registers): at most
    128 VGPRs, FP64-dense code needs the four waves per SIMD.  The counts pin
    what the unit instantiates: olpe_samples.h's front end for 2 and 3 sources, the
    correlation once (it does not depend on the number of sources)."""
    res = kernel_resources("olpe_detect.hip")
    counts = (("resid_scan_kernel", 2), ("resid_book_kernel", 2), ("resid_desc_kernel", 2),
              ("detect_rowdesc_kernel", 2), ("detect_index_kernel", 2),
              ("detect_prep_kernel", 2), ("detect_corr_kernel", 1),
              ("detect_planes_kernel", 1), ("detect_stats_kernel", 1),
              ("detect_reduce_kernel", 1))
    assert len(res) == sum(c for _, c in counts), list(res)
    for kern, count in counts:
        hits = [v for k, v in res.items() if kern in k]
        assert len(hits) == count, (kern, list(res))
        for v in hits:
            assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (kern, v)
            if kern == "detect_corr_kernel":
                assert v["VGPRs"] + v["AGPRs"] <= 128, (kern, v)
                assert v["Occupancy [waves/SIMD]"] >= 4, (kern, v)
