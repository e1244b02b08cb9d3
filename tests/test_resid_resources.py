"""The residual-image kernels (olpe_resid.hip) use no scratch, and the fold kernels fit four
waves per SIMD: checked from the compiler's resource usage, as test_corner_resources does
for the corner folds."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_resid_kernels_have_no_scratch_and_fit_four_waves():
    """Every kernel of the unit: ScratchSize 0, no VGPR spill.  The fold kernels (2 and 3
    sources x both tile heights) hold a tile's 2R accumulators in registers and still use
    at most 128 VGPRs: FP64-dense code needs the four waves per SIMD."""
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    from olpefit_amd import build
    src = os.path.join(build.CSRC, "olpe_resid.hip")
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
