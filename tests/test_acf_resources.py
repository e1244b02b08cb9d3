"""The autocorrelation kernels (olpe_acf.hip) use no scratch and the fold kernel fits the
occupancy its design relies on: checked from the compiler's resource usage, as
test_corner_resources does for the corner folds."""
from resource_usage import kernel_resources


def test_acf_kernels_have_no_scratch_and_fit_their_occupancy():
    """Every kernel of the unit: ScratchSize 0, no VGPR spill.  acf_fold_kernel with one lag
    pass (max_lag <= 512) uses at most 96 VGPRs.  Why 96: a workgroup is one wave per column
    of its group, 9 waves for 17 columns in two groups, and two workgroups share a CU's LDS,
    so 18 waves sit on four SIMDs, five on the fullest; 512 VGPRs per lane / 5 waves = 102,
    allocated in steps of 8: 96.  With two passes (max_lag > 512) a staged
    column is at least 10,880 bytes, so a workgroup has at most 7 waves and two workgroups 14,
    four on the fullest SIMD: 128 VGPRs."""
    res = kernel_resources("olpe_acf.hip")
    for kern, count in (("acf_stats_kernel", 1), ("acf_fold_kernel", 2),
                        ("acf_reduce_kernel", 1), ("acf_reduce0_kernel", 1)):
        hits = [v for k, v in res.items() if kern + "E" in k or kern + "I" in k]
        assert len(hits) == count, (kern, list(res))
        for v in hits:
            assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (kern, v)
        if kern == "acf_fold_kernel":
            for passes, vgprs, waves in ((1, 96, 5), (2, 128, 4)):
                (v,) = [v for k, v in res.items() if f"{kern}ILi{passes}E" in k]
                assert v["VGPRs"] + v["AGPRs"] <= vgprs, (kern, passes, v)
                assert v["Occupancy [waves/SIMD]"] >= waves, (kern, passes, v)
