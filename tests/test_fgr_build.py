"""The compiler's own resource report for csrc/fgr.hip (as tests/test_ransac_build.py reads it for ransac.hip): the 29 float64
terms of a match, their fold and the 6 x 7 system of the step all stay in registers -- no scratch memory in any kernel, the
shipping build and the developer build (which adds the single-block form of the loop) alike."""
import os

import pytest

from kernel_resources import HIPCC, kernel_resources

SHIP = ("k_fgr_reduce", "k_fgr_update", "k_fgr_fold", "k_fgr_weight", "k_fgr_tuples")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("defs, kernels", [((), SHIP), (("-DPCR_DEV=1",), SHIP + ("k_fgr_solo",))])
def test_fgr_kernels_stay_out_of_scratch(defs, kernels):
    report = kernel_resources("fgr.hip", defs)
    print({n: (u["scratch"], u.get("vgprs")) for n, u in sorted(report.items())})
    for k in kernels:
        assert sum(k in n for n in report) == 1, f"the resource report was not parsed: {sorted(report)}"
    assert len(report) == len(kernels)                         # k_fgr_solo is in the developer build only
    assert {n: u["scratch"] for n, u in report.items() if u["scratch"] != 0} == {}
    reduce = next(u for n, u in report.items() if "k_fgr_reduce" in n)
    assert reduce["vgprs"] <= 128                              # four waves per SIMD
