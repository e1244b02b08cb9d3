"""The covariance kernels (olpe_cov.hip) use no scratch and the fold kernel fits the
occupancy its design relies on: checked from the compiler's resource usage, as
test_acf_resources does for the autocorrelation folds."""
from resource_usage import kernel_resources

COLS = (4, 8, 12, 16, 20, 24)       # the column counts instantiated (ncols rounded up to 4)
TILES = (64, 128, 256)              # the tile heights (OLPE_COV_TILE; 256 the default)


def test_cov_kernels_have_no_scratch_and_fit_their_occupancy():
    """Every kernel of the unit, every instantiated column count and tile height:
    ScratchSize 0, no VGPR spill.

    cov_fold_kernel is a workgroup of 8 waves, two on each SIMD.  Up to 12 columns (6 column
    blocks of 4 x 4: one block, 16 accumulators, a wave) two workgroups share a CU, which
    hides one's staging behind the other's walk: 4 waves a SIMD, 512 / 4 = 128 VGPRs.  From 16
    columns on a wave holds 2 or 3 blocks (32 or 48 accumulators = 64 or 96 VGPRs) beside the
    next tile's values in flight (up to 16 a thread = 32 VGPRs), which does not fit 128: one
    workgroup has the CU, 2 waves a SIMD, 512 / 2 = 256 VGPRs, and keeps HBM busy through its
    walk with a whole 256-row tile (35 KB at 17 columns) in flight."""
    res = kernel_resources("olpe_cov.hip")
    for kern in ("cov_pivot_kernel", "cov_reduce_kernel", "cov_walker_kernel",
                 "cov_between_kernel"):
        hits = [v for k, v in res.items() if kern + "E" in k]
        assert len(hits) == 1, (kern, list(res))
        assert hits[0]["ScratchSize [bytes/lane]"] == 0 and hits[0]["VGPRs Spill"] == 0, kern
    folds = {k: v for k, v in res.items() if "cov_fold_kernelI" in k}
    assert len(folds) == len(COLS) * len(TILES), list(folds)
    for cp in COLS:
        for tr in TILES:
            (v,) = [v for k, v in folds.items() if f"cov_fold_kernelILi{cp}ELi{tr}E" in k]
            assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (cp, tr, v)
            vgprs, waves = (128, 4) if cp <= 12 else (256, 2)
            assert v["VGPRs"] + v["AGPRs"] <= vgprs, (cp, tr, v)
            assert v["Occupancy [waves/SIMD]"] >= waves, (cp, tr, v)
