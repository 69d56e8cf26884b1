"""The compiler's own resource report for csrc/gicp.hip (as tests/test_seam64_build.py reads it for seam64.hip): every GICP
kernel is there, the reduce and fold kernels stay out of scratch memory altogether, and the covariance kernels -- a k-NN search
and a Jacobi eigen-solver in one kernel -- do not end up there unnoticed."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "point_cloud_registration_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_gicp_kernels_stay_out_of_scratch(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
                        f"-I{REPO}/include", f"-I{CSRC}", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "gicp.hip"), "-o", str(tmp_path / "g.o")], capture_output=True, text=True, check=True)
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            usage[name] = int(m.group(1))
    gicp = {n: b for n, b in usage.items() if "k_gicp_" in n}
    assert sum("k_gicp_cov" in n for n in gicp) == 2 and sum("k_gicp_reduce" in n for n in gicp) == 1 \
        and sum("k_gicp_fold" in n for n in gicp) == 1, f"the resource report was not parsed: {sorted(usage)}"
    assert len(gicp) == len(usage), sorted(set(usage) - set(gicp))
    assert [b for n, b in gicp.items() if "k_gicp_reduce" in n or "k_gicp_fold" in n] == [0, 0]
    assert {n: b for n, b in usage.items() if b > 128} == {}
