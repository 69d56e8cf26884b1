#!/usr/bin/env python3
"""Records tests/golden/g17_fold_bits.npz: the 29 sums of every case of tests/fold_cases.py, as the loaded library returns
them.  Run it ONCE on the build whose bits are the reference (the parent of a change to the folds: PCR_LIB=<its library>), on
an MI355X; tests/test_gpu_fold_bits.py then requires the same bits of the tree's library.
    PCR_LIB=build/exp/libpcr_parent.so python tools/make_golden_fold_bits.py [out.npz]"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import fold_cases as fc  # noqa: E402
from point_cloud_registration_amd import _capi  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "g17_fold_bits.npz")
res = fc.run_all(_capi, _capi.get_context(0))
np.savez_compressed(out, **res)
print(f"{out}: {len(res)} cases, {os.path.getsize(out)} bytes, library {os.environ.get('PCR_LIB', '(the tree)')}")
