"""The compiler's own resource report for csrc/symm.hip (as tests/test_gicp_build.py reads it for gicp.hip): the unit holds
only k_symm_* kernels, the reduce and fold kernels stay out of scratch memory altogether, and the normal kernels -- a k-NN
search and a Jacobi eigen-solver in one kernel -- do not end up there unnoticed."""
import os

import pytest

from kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_symm_kernels_stay_out_of_scratch():
    report = kernel_resources("symm.hip")
    usage = {n: u["scratch"] for n, u in report.items()}
    symm = {n: b for n, b in usage.items() if "k_symm_" in n}
    assert sum("k_symm_normals" in n for n in symm) == 2 and sum("k_symm_perm" in n for n in symm) == 2 \
        and sum("k_symm_reduce" in n for n in symm) == 1 and sum("k_symm_fold" in n for n in symm) == 1, \
        f"the resource report was not parsed: {sorted(usage)}"
    assert len(symm) == len(usage), sorted(set(usage) - set(symm))
    assert [b for n, b in symm.items() if "k_symm_reduce" in n or "k_symm_fold" in n] == [0, 0]
    assert {n: b for n, b in usage.items() if b > 128} == {}
    # four waves per SIMD: the reduce kernel stays within 128 registers (SYMM_W = 3)
    assert [u["vgprs"] for n, u in report.items() if "k_symm_reduce" in n][0] <= 128
