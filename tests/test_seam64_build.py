"""The compiler's own resource report for csrc/seam64.hip (as tests/test_build_hygiene.py reads it for kernels.hip): the
float64 seam kernels carry a ring search, a ball walk and, for k > 1, the float32 k-NN in one kernel -- none of that may end
up in scratch memory unnoticed."""
import os

import pytest

from kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_seam64_kernels_stay_out_of_scratch():
    report = kernel_resources("seam64.hip")
    usage = {n: u["scratch"] for n, u in report.items()}
    assert sum("k_nn_query_dd" in n for n in usage) == 3 and sum("k_knn_query_f64" in n for n in usage) == 3, \
        f"the resource report was not parsed: {sorted(usage)}"
    assert {n: b for n, b in usage.items() if b > 128} == {}
