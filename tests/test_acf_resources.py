"""The autocorrelation kernels (olpe_acf.hip) use no scratch and the fold kernel fits the
occupancy its design relies on: checked from the compiler's resource usage, as
test_corner_resources does for the corner folds."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_acf_kernels_have_no_scratch_and_fit_their_occupancy():
    """Every kernel of the unit: ScratchSize 0, no VGPR spill.  acf_fold_kernel with one lag
    pass (max_lag <= 512) uses at most 96 VGPRs.  Why 96: a workgroup is one wave per column
    of its group, 9 waves for 17 columns in two groups, and two workgroups share a CU's LDS,
    so 18 waves sit on four SIMDs, five on the fullest; 512 VGPRs per lane / 5 waves = 102,
    allocated in steps of 8: 96.  With two passes (max_lag > 512) a staged
    column is at least 10,880 bytes, so a workgroup has at most 7 waves and two workgroups 14,
    four on the fullest SIMD: 128 VGPRs."""
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    from olpefit_amd import build
    src = os.path.join(build.CSRC, "olpe_acf.hip")
    assert src in build.SOURCES
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC", "-Wall",
                                                  "-Wno-unused-function")]
    cmd = [HIPCC, *flags, "--cuda-device-only", "-c", "-o", os.devnull, src,
           "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    res, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|"
                      r"Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            res[name][m.group(1)] = int(m.group(2))
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
