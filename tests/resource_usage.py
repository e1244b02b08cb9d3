"""The compiler's resource usage of one HIP unit's kernels, for the *_resources tests of
the fold objects: a device-only compile with the product's flags and
-Rpass-analysis=kernel-resource-usage, its remarks parsed."""
import os
import re
import shutil
import subprocess

import pytest

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def kernel_resources(unit):
    """{mangled kernel name: {"VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill",
    "Occupancy [waves/SIMD]"}} of olpefit_amd/csrc/<unit>, one of the library's sources.
    Skips the calling test where there is no hipcc."""
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    from olpefit_amd import build
    src = os.path.join(build.CSRC, unit)
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
    return res
