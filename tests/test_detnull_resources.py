"""The false-alarm calibration's kernels (olpe_detnull.hip) use no scratch, and the
correlation kernel keeps the registers and occupancy its design rests on: checked from the
compiler's resource usage, as test_detect_resources does for the detection map."""
from resource_usage import kernel_resources


def test_detnull_kernels_have_no_scratch_and_the_correlation_fits_four_waves():
    """Every kernel of the unit, each instantiated once: ScratchSize 0, no VGPR spill.  The
    correlation holds 4 candidate rows x 8 realisations = 32 FP64 sums per lane (64 VGPRs),
    4 table values and addresses: at most 128 VGPRs, so four waves per SIMD stay resident
    (its launch bound asks for 4 to 8).  It needs them: a loop iteration waits for one scalar
    load of 8 realisations' y and 4 LDS reads, then issues 32 FMAs, and only other waves
    cover that wait (FP64-dense code needs the four waves per SIMD)."""
    res = kernel_resources("olpe_detnull.hip")
    kernels = ("detnull_noise_kernel", "detnull_weight_kernel", "detnull_corr_kernel",
               "detnull_stats_kernel")
    assert len(res) == len(kernels), list(res)
    for kern in kernels:
        hits = [v for k, v in res.items() if kern in k]
        assert len(hits) == 1, (kern, list(res))
        v = hits[0]
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (kern, v)
        if kern == "detnull_corr_kernel":
            assert v["VGPRs"] + v["AGPRs"] <= 128, (kern, v)
            assert v["Occupancy [waves/SIMD]"] >= 4, (kern, v)
