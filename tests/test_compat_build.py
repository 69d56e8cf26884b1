"""The compiler's own resource report for csrc/compat.hip (as tests/test_ransac_build.py reads it for ransac.hip): the three
kernels are there, and the row of the matrix a wave holds (eight 64-bit words per lane), the two rows it has in flight and the
float64 tests of k_compat_bits all stay in registers -- no scratch memory in any of them."""
import os

import pytest

from kernel_resources import HIPCC, kernel_resources

KERNELS = ("k_compat_bits", "k_compat_degrees", "k_compat_consensus")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_compat_kernels_stay_out_of_scratch():
    report = kernel_resources("compat.hip")
    print({n: (u["scratch"], u.get("vgprs"), u.get("lds")) for n, u in sorted(report.items())})
    for k in KERNELS:                                           # k_compat_degrees in two forms: one row per wave, four rows per wave
        assert sum(k in n for n in report) == (2 if k == "k_compat_degrees" else 1), f"the resource report was not parsed: {sorted(report)}"
    assert len(report) == len(KERNELS) + 1
    assert {n: u["scratch"] for n, u in report.items() if u["scratch"] != 0} == {}
    for n, u in report.items():
        if "k_compat_degrees" in n:                            # one row per wave: four waves per SIMD at least; four rows: three
            assert u["lds"] == 0 and u["vgprs"] <= (128 if "ILi1E" in n else 168), (n, u)
    consensus = next(u for n, u in report.items() if "k_compat_consensus" in n)
    assert consensus["lds"] <= 80 * 1024                       # row s and a 16-bit score per row: two blocks per CU
