"""The compiler's own resource report for csrc/color.hip (as tests/test_symm_build.py reads it for symm.hip): the unit holds
only k_color_* kernels, the reduce and fold kernels stay out of scratch memory altogether, and the gradient kernels -- a k-NN
search and a 3 x 3 solve in one kernel -- do not end up there unnoticed."""
import os

import pytest

from kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_color_kernels_stay_out_of_scratch():
    report = kernel_resources("color.hip")
    usage = {n: u["scratch"] for n, u in report.items()}
    color = {n: b for n, b in usage.items() if "k_color_" in n}
    count = lambda name: sum(name in n for n in color)
    assert count("k_color_gradient") == 2 and count("k_color_perm") == 2 and count("k_color_reduce") == 1 \
        and count("k_color_fold") == 1 and count("k_color_gather") == 1 and count("k_color_pack") == 1 \
        and count("k_color_unpack") == 1, f"the resource report was not parsed: {sorted(usage)}"
    assert len(color) == len(usage), sorted(set(usage) - set(color))
    assert [b for n, b in color.items() if "k_color_reduce" in n or "k_color_fold" in n] == [0, 0]
    assert {n: b for n, b in usage.items() if b > 128} == {}
    # four waves per SIMD: the reduce kernel stays within 128 registers (COLOR_W = 2)
    assert [u["vgprs"] for n, u in report.items() if "k_color_reduce" in n][0] <= 128
