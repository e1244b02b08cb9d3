"""The corner fold kernels (olpe_corner.hip) use no scratch: checked from the compiler's
resource usage, as test_kernel_resources does for the moment folds."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_corner_fold_kernels_have_no_scratch():
    """Both lane layouts of the 2-D fold and the 1-D fold: no scratch, no spill, and few
    enough VGPRs for 8 waves per SIMD (the folds hide L2 and LDS-atomic latency with
    occupancy)."""
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    from olpefit_amd import build
    assert os.path.join(build.CSRC, "olpe_corner.hip") in build.SOURCES
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC", "-Wall",
                                                  "-Wno-unused-function")]
    cmd = [HIPCC, *flags, "--cuda-device-only", "-c", "-o", os.devnull,
           os.path.join(REPO, "olpefit_amd", "csrc", "olpe_corner.hip"),
           "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    res, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and name:
            res[name][m.group(1)] = int(m.group(2))
    for kern, count in (("corner_fold1_kernel", 1), ("corner_fold2_kernel", 2)):
        hits = [v for k, v in res.items() if kern in k]
        assert len(hits) == count, (kern, list(res))
        for v in hits:
            assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (kern, v)
            assert v["VGPRs"] <= 64, (kern, v)
