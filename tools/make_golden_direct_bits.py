#!/usr/bin/env python3
"""Records tests/golden/g18_direct_bits.npz: what every case of tests/direct_bits_cases.py returns from the loaded library.
Run it ONCE on the build whose bits are the reference (the parent of a change to the host scaffold of the match-list passes or
to the direct VGICP unit: PCR_LIB=<its library>, tools/build_rev_lib.sh), on an MI355X; tests/test_gpu_direct_bits.py then
requires the same bits of the tree's library.
    PCR_LIB=build/exp/libpcr_parent.so python tools/make_golden_direct_bits.py [out.npz]"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import direct_bits_cases as db  # noqa: E402
from point_cloud_registration_amd import _capi  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "g18_direct_bits.npz")
g2 = dict(np.load(os.path.join(REPO, "tests", "golden", "g2_mini_street.npz"), allow_pickle=False))
res = db.run_all(_capi, _capi.get_context(0), g2)
np.savez_compressed(out, **res)
print(f"{out}: {len(res)} cases, {os.path.getsize(out)} bytes, library {os.environ.get('PCR_LIB', '(the tree)')}")
