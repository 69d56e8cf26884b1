"""The compiler's own resource report for csrc/keypoints.hip (as tests/test_fpfh_build.py reads it for fpfh.hip):
k_iss_saliency keeps the anchor, 9 float64 sums and the Jacobi's matrix per lane, k_iss_nms a count and a flag -- all of it
in registers, none of it in scratch memory."""
import os
import re

import pytest

from kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_iss_kernels_stay_out_of_scratch():
    report = kernel_resources("keypoints.hip")
    usage = {n: u["scratch"] for n, u in report.items()}
    vgprs = {n: u["vgprs"] for n, u in report.items()}
    # k_iss_saliency<cell-sorted / caller order> and k_iss_nms
    sal = [n for n in usage if re.match(r"_Z14k_iss_saliencyILi[01]E", n)]
    nms = [n for n in usage if re.match(r"_Z9k_iss_nms", n)]
    assert len(sal) == 2 and len(nms) == 1, f"the resource report was not parsed: {sorted(usage)}"
    print({n: (vgprs.get(n), usage[n]) for n in sal + nms})
    assert {n: b for n, b in usage.items() if b > 128} == {}
