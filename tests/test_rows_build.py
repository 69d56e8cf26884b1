"""Build-time guarantee of csrc/rows.hip that needs no GPU: the compiler's own resource report says that no k_rows
instantiation keeps state in scratch (the pattern of test_build_hygiene.test_hot_kernels_use_no_scratch)."""

import os
import re
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "point_cloud_registration_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_rows_kernels_use_no_scratch(tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
                        f"-I{REPO}/include", f"-I{CSRC}", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "rows.hip"), "-o", str(tmp_path / "rows.o")], capture_output=True, text=True, check=True)
    scratch, vgprs, name = {}, {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r" VGPRs: (\d+)", line)
        if m and name:
            vgprs[name] = int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    rows = {n: b for n, b in scratch.items() if re.match(r"_Z6k_rowsILi\dELi\dEE", n)}
    for n in sorted(rows):
        print(n, "VGPRs", vgprs.get(n), "scratch", rows[n])
    # KIND in {ICP, PLANE, VPLANE, NDT} x MODE in {rows, terms, flags}
    assert sorted(rows) == sorted(f"_Z6k_rowsILi{k}ELi{m}EEv7LinArgs7RowArgs" for k in range(4) for m in range(3))
    assert {n: b for n, b in rows.items() if b != 0} == {}
