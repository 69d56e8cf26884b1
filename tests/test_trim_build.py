"""The compiler's own resource report for the kernels of the adaptive pass (as tests/test_robust_build.py reads it for the
robust ones): the selection kernels of select.hip and the key and adaptive-reduce kernels of gicp.hip, vgicp.hip, symm.hip
and color.hip are each there exactly once and stay out of scratch memory, in the shipping build and in the developer build.
The adaptive reduce is the robust reduce with its kernel read from device memory into scalar registers, so its ceiling is the
robust kernel's (tests/test_robust_build.py): 128 registers = four waves per SIMD, 168 = three (512 per lane and SIMD, granule
8); a key kernel is the residual kernel with one store per point, eight waves."""
import os

import pytest

from kernel_resources import HIPCC, kernel_resources

# unit -> (key kernel, adaptive reduce, its VGPR ceiling)
UNITS = {"gicp.hip": ("k_gicp_keys", "k_gicp_adaptive", 168), "vgicp.hip": ("k_vgicp_keys", "k_vgicp_adaptive", 168),
         "symm.hip": ("k_symm_keys", "k_symm_adaptive", 168), "color.hip": ("k_color_keys", "k_color_adaptive", 128)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("defs", [(), ("-DPCR_DEV=1",)], ids=["ship", "dev"])
@pytest.mark.parametrize("unit", sorted(UNITS))
def test_adaptive_kernels_stay_out_of_scratch(unit, defs):
    keys, adaptive, ceiling = UNITS[unit]
    report = kernel_resources(unit, defs)
    print({n: (u["scratch"], u.get("vgprs")) for n, u in sorted(report.items())})
    for k in (keys, adaptive):
        assert sum(k in n for n in report) == 1, f"the resource report was not parsed: {sorted(report)}"
    one = lambda k: next(u for n, u in report.items() if k in n)
    assert one(keys)["scratch"] == 0 and one(adaptive)["scratch"] == 0
    assert one(keys)["vgprs"] <= 64
    assert one(adaptive)["vgprs"] <= ceiling


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_selection_kernels():
    """k_select_hist: 1 KiB of LDS (256 uint32 bins), k_select_pick: 2 KiB (256 uint64), k_select_drop: none; eight waves."""
    report = kernel_resources("select.hip")
    print({n: u for n, u in sorted(report.items())})
    one = lambda k: next(u for n, u in report.items() if k in n)
    for k, lds in (("k_select_hist", 1024), ("k_select_pick", 2048), ("k_select_drop", 0)):
        assert sum(k in n for n in report) == 1, sorted(report)
        assert one(k)["scratch"] == 0 and one(k)["lds"] == lds and one(k)["vgprs"] <= 64
