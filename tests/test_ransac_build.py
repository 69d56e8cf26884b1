"""The compiler's own resource report for csrc/ransac.hip (as tests/test_fpfh_build.py reads it for fpfh.hip): k_pose_score
keeps its poses in registers -- no scratch memory at all -- and nothing in the file is above 128 bytes of it."""
import os

import pytest

from kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_ransac_kernels_stay_out_of_scratch():
    report = kernel_resources("ransac.hip")
    usage = {n: u["scratch"] for n, u in report.items()}
    vgpr = {n: u["vgprs"] for n, u in report.items()}
    score = [n for n in usage if "k_pose_score" in n]
    print({n: (usage[n], vgpr.get(n)) for n in sorted(usage)})
    # with and without the mask
    assert len(score) == 2, f"the resource report was not parsed: {sorted(usage)}"
    assert sum("k_ransac_fit" in n for n in usage) == 1 and sum("k_ransac_best" in n for n in usage) == 1
    assert all(usage[n] == 0 for n in score)
    assert {n: b for n, b in usage.items() if b > 128} == {}
