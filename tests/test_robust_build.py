"""The compiler's own resource report for the robust and residual kernels of gicp.hip, vgicp.hip, symm.hip and color.hip (as
tests/test_fgr_build.py reads it for fgr.hip): each is there exactly once and stays out of scratch memory, in the shipping build
and in the developer build, and the plain reduce kernels beside them keep the registers they had before the kernels came."""
import os

import pytest

from kernel_resources import HIPCC, kernel_resources

# unit -> (robust kernel, residual kernel, plain reduce kernel, its VGPRs before this feature, VGPR ceiling of the robust kernel)
# ceilings: 128 = four waves per SIMD, 168 = three (512 registers per lane and SIMD, granule 8)
UNITS = {"gicp.hip": ("k_gicp_robust", "k_gicp_residuals", "k_gicp_reduce", 162, 168),
         "vgicp.hip": ("k_vgicp_robust", "k_vgicp_residuals", "k_vgicp_reduce", 156, 168),
         "symm.hip": ("k_symm_robust", "k_symm_residuals", "k_symm_reduce", 122, 168),
         "color.hip": ("k_color_robust", "k_color_residuals", "k_color_reduce", 126, 128)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("defs", [(), ("-DPCR_DEV=1",)], ids=["ship", "dev"])
@pytest.mark.parametrize("unit", sorted(UNITS))
def test_robust_kernels_stay_out_of_scratch(unit, defs):
    robust, resid, plain, plain_vgprs, ceiling = UNITS[unit]
    report = kernel_resources(unit, defs)
    print({n: (u["scratch"], u.get("vgprs")) for n, u in sorted(report.items())})
    for k in (robust, resid, plain):
        assert sum(k in n for n in report) == 1, f"the resource report was not parsed: {sorted(report)}"
    one = lambda k: next(u for n, u in report.items() if k in n)
    assert one(robust)["scratch"] == 0 and one(resid)["scratch"] == 0
    assert one(robust)["vgprs"] <= ceiling
    assert one(resid)["vgprs"] <= 64                           # one point per lane: eight waves per SIMD
    assert one(plain)["vgprs"] == plain_vgprs and one(plain)["scratch"] == 0
