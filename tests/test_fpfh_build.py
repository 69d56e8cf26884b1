"""The compiler's own resource report for csrc/fpfh.hip (as tests/test_radius_build.py reads it for radius.hip): k_spfh keeps
33 dynamically indexed counters per lane, k_fpfh 33 float64 accumulators, k_feature_nn a whole row of A -- the counters belong
in LDS, the rest in registers, none of it in scratch memory."""
import os
import re

import pytest

from kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_fpfh_kernels_stay_out_of_scratch():
    report = kernel_resources("fpfh.hip")
    usage = {n: u["scratch"] for n, u in report.items()}
    lds = {n: u["lds"] for n, u in report.items()}
    # k_spfh<cell-sorted / caller order>, k_fpfh, k_feature_nn<33 / 64> and its merge
    spfh = [n for n in usage if re.match(r"_Z6k_spfhILi[01]E", n)]
    fpfh = [n for n in usage if re.match(r"_Z6k_fpfh", n)]
    nn = [n for n in usage if re.match(r"_Z12k_feature_nnILi(33|64)E", n)]
    assert len(spfh) == 2 and len(fpfh) == 1 and len(nn) == 2 and sum("k_feature_merge" in n for n in usage) == 1, \
        f"the resource report was not parsed: {sorted(usage)}"
    assert {n: b for n, b in usage.items() if b > 128} == {}
    # the counters of k_spfh: [33 bins][64 lanes] of uint32 in LDS
    assert all(lds[n] == 33 * 64 * 4 for n in spfh)
