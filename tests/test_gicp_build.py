"""The compiler's own resource report for csrc/gicp.hip (as tests/test_seam64_build.py reads it for seam64.hip): every GICP
kernel is there, the reduce and fold kernels stay out of scratch memory altogether, and the covariance kernels -- a k-NN search
and a Jacobi eigen-solver in one kernel -- do not end up there unnoticed."""
import os

import pytest

from kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_gicp_kernels_stay_out_of_scratch():
    report = kernel_resources("gicp.hip")
    usage = {n: u["scratch"] for n, u in report.items()}
    gicp = {n: b for n, b in usage.items() if "k_gicp_" in n}
    assert sum("k_gicp_cov" in n for n in gicp) == 2 and sum("k_gicp_reduce" in n for n in gicp) == 1 \
        and sum("k_gicp_fold" in n for n in gicp) == 1, f"the resource report was not parsed: {sorted(usage)}"
    assert len(gicp) == len(usage), sorted(set(usage) - set(gicp))
    assert [b for n, b in gicp.items() if "k_gicp_reduce" in n or "k_gicp_fold" in n] == [0, 0]
    assert {n: b for n, b in usage.items() if b > 128} == {}
