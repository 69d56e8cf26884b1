"""Build-time guarantee of csrc/rows.hip that needs no GPU: the compiler's own resource report says that no k_rows
instantiation keeps state in scratch (the pattern of test_build_hygiene.test_hot_kernels_use_no_scratch)."""
import os
import re

import pytest

from kernel_resources import HIPCC, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_rows_kernels_use_no_scratch():
    report = kernel_resources("rows.hip")
    scratch = {n: u["scratch"] for n, u in report.items()}
    vgprs = {n: u["vgprs"] for n, u in report.items()}
    rows = {n: b for n, b in scratch.items() if re.match(r"_Z6k_rowsILi\dELi\dEE", n)}
    for n in sorted(rows):
        print(n, "VGPRs", vgprs.get(n), "scratch", rows[n])
    # KIND in {ICP, PLANE, VPLANE, NDT} x MODE in {rows, terms, flags}
    assert sorted(rows) == sorted(f"_Z6k_rowsILi{k}ELi{m}EEv7LinArgs7RowArgs" for k in range(4) for m in range(3))
    assert {n: b for n, b in rows.items() if b != 0} == {}
