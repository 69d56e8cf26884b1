"""The compiler's own resource report for csrc/ball_moments.hip (as tests/test_iss_build.py reads it for keypoints.hip):
k_ball_moments keeps the anchor, 9 float64 sums and the Jacobi's matrix per lane -- the register list of the hybrid form beside
them -- in registers, none of it in scratch memory."""
import os
import re

import pytest

from kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_ball_kernels_stay_out_of_scratch():
    report = kernel_resources("ball_moments.hip")
    usage = {n: u["scratch"] for n, u in report.items()}
    vgprs = {n: u["vgprs"] for n, u in report.items()}
    # k_ball_moments<radius set / register list / LDS list>, the payload permutations, the target records and the counts
    ball = [n for n in usage if re.match(r"_Z14k_ball_momentsILi[012]E", n)]
    perm = [n for n in usage if re.match(r"_Z11k_ball_permILi[36]ELb[01]E", n)]
    rest = [n for n in usage if re.match(r"_Z(14k_ball_tcov_in|17k_ball_count_perm)", n)]
    assert len(ball) == 3 and len(perm) == 4 and len(rest) == 2, f"the resource report was not parsed: {sorted(usage)}"
    print({n: (vgprs.get(n), usage[n]) for n in ball})
    assert {n: b for n, b in usage.items() if b > 128} == {}
