"""The compiler's own resource report for csrc/radius.hip (as tests/test_seam64_build.py reads it for seam64.hip): the radius
kernels carry a ball walk with batched loads, the mean-distance kernels the whole k-NN search -- none of that may end up in
scratch memory unnoticed."""
import os
import re

import pytest

from kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_radius_kernels_stay_out_of_scratch():
    report = kernel_resources("radius.hip")
    usage = {n: u["scratch"] for n, u in report.items()}
    # k_radius<float / double, count / fill>, k_knn_mean_dist<list / collect>, the two unpack kernels
    assert sum(bool(re.match(r"_Z8k_radiusI[fd]Li[01]E", n)) for n in usage) == 4 and sum("k_knn_mean_dist" in n for n in usage) == 2 \
        and sum("k_radius_unpack" in n for n in usage) == 2, f"the resource report was not parsed: {sorted(usage)}"
    # (the unit also instantiates rocPRIM's segmented sort; those kernels are the library's own)
    assert {n: b for n, b in usage.items() if ("k_radius" in n or "k_knn_mean_dist" in n) and "rocprim" not in n and b > 128} == {}
