"""The compiler's own resource report for csrc/seam64.hip (as tests/test_build_hygiene.py reads it for kernels.hip): the
float64 seam kernels carry a ring search, a ball walk and, for k > 1, the float32 k-NN in one kernel -- none of that may end
up in scratch memory unnoticed."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "point_cloud_registration_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_seam64_kernels_stay_out_of_scratch(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
                        f"-I{REPO}/include", f"-I{CSRC}", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "seam64.hip"), "-o", str(tmp_path / "s.o")], capture_output=True, text=True, check=True)
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            usage[name] = int(m.group(1))
    assert sum("k_nn_query_dd" in n for n in usage) == 3 and sum("k_knn_query_f64" in n for n in usage) == 3, \
        f"the resource report was not parsed: {sorted(usage)}"
    assert {n: b for n, b in usage.items() if b > 128} == {}
