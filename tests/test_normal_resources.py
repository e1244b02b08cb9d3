"""The normal-equations kernels (olpe_normal.hip) use no scratch and fit the occupancy their
design states: checked from the compiler's resource usage, as test_cov_resources does for
the covariance folds."""
from resource_usage import kernel_resources


def test_normal_kernels_have_no_scratch_and_fit_their_occupancy():
    """normal_kernel<NSRC> is a workgroup of 4 waves, one vector each, one on each SIMD.  A
    lane holds P derivatives and P gradient accumulators (2 P doubles: 64 VGPRs at P = 16, 76
    at P = 19) beside the 2 NSRC Gaussians' terms of the pixel in flight; the J^T J tile is 8
    registers (16 with the 16 x 3 block of the 3-source layout) and 6 accumulators hold its
    3 x 3 corner.  Two sources: 512 / 3 = 168 registers, three waves a SIMD, and the 34 KB of
    LDS tiles a workgroup (4 x 64 x 17 doubles) let four workgroups share a CU.  Three
    sources: 256 registers, two waves a SIMD (43 KB of tiles: three workgroups a CU).  The
    per-pixel test kernel fits 128 registers."""
    res = kernel_resources("olpe_normal.hip")
    for nsrc, regs, waves in ((2, 168, 3), (3, 256, 2)):
        kerns = [(f"normal_kernelILi{nsrc}ELb0E", regs, waves),
                 (f"jacobian_kernelILi{nsrc}E", 128, 4)]
        if nsrc == 3:            # the A/B variant with the corner on the matrix core
            kerns.append(("normal_kernelILi3ELb1E", regs, waves))
        for kern, r, w in kerns:
            hits = [v for k, v in res.items() if kern in k]
            assert len(hits) == 1, (kern, list(res))
            v = hits[0]
            assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (kern, v)
            assert v["VGPRs"] + v["AGPRs"] <= r, (kern, v)
            assert v["Occupancy [waves/SIMD]"] >= w, (kern, v)
