"""The compiler's own resource report for csrc/ransac.hip (as tests/test_fpfh_build.py reads it for fpfh.hip): k_pose_score
keeps its poses in registers -- no scratch memory at all -- and nothing in the file is above 128 bytes of it."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "point_cloud_registration_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_ransac_kernels_stay_out_of_scratch(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
                        f"-I{REPO}/include", f"-I{CSRC}", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "ransac.hip"), "-o", str(tmp_path / "r.o")], capture_output=True, text=True, check=True)
    usage, vgpr, name = {}, {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            usage[name] = int(m.group(1))
        m = re.search(r" VGPRs: (\d+)", line)
        if m and name:
            vgpr[name] = int(m.group(1))
    score = [n for n in usage if "k_pose_score" in n]
    print({n: (usage[n], vgpr.get(n)) for n in sorted(usage)})
    # with and without the mask
    assert len(score) == 2, f"the resource report was not parsed: {sorted(usage)}"
    assert sum("k_ransac_fit" in n for n in usage) == 1 and sum("k_ransac_best" in n for n in usage) == 1
    assert all(usage[n] == 0 for n in score)
    assert {n: b for n, b in usage.items() if b > 128} == {}
