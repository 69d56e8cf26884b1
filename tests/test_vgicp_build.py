"""The compiler's own resource report for csrc/vgicp.hip (as tests/test_gicp_build.py reads it for gicp.hip): every kernel of
the translation unit is a k_vgicp_ kernel, the reduce and fold kernels stay out of scratch memory altogether, and no kernel
ends up there unnoticed."""
import os

import pytest

from kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_vgicp_kernels_stay_out_of_scratch():
    report = kernel_resources("vgicp.hip")
    usage = {n: u["scratch"] for n, u in report.items()}
    vgprs = {n: u["vgprs"] for n, u in report.items()}
    vg = {n: b for n, b in usage.items() if "k_vgicp_" in n}
    assert sum("k_vgicp_reduce" in n for n in vg) == 1 and sum("k_vgicp_fold" in n for n in vg) == 1 \
        and sum("k_vgicp_plane_cov" in n for n in vg) == 1, f"the resource report was not parsed: {sorted(usage)}"
    assert len(vg) == len(usage), sorted(set(usage) - set(vg))
    assert [b for n, b in vg.items() if "k_vgicp_reduce" in n or "k_vgicp_fold" in n] == [0, 0]
    assert {n: b for n, b in usage.items() if b > 128} == {}
    # three waves per SIMD (at most 168 registers per lane), where its sibling k_gicp_reduce runs
    reduce_vgprs = [v for n, v in vgprs.items() if "k_vgicp_reduce" in n]
    print(f"k_vgicp_reduce: {reduce_vgprs[0]} VGPRs")
    assert reduce_vgprs and reduce_vgprs[0] <= 168
