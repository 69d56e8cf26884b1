#!/usr/bin/env python3
"""Generate tests/golden/g17_seam_f64.npz by IMPORTING the reference (authoring container only, like make_golden.py, whose
pykdtree shim and import path this script takes over):

    python tests/golden/make_golden_seam_f64.py

What the reference's ``KDTree(float64 target).query(float64 queries, k)`` returns for k = 1 and k = 5 on case A of
tests/seam_f64_cases.py: the g9 target and queries a few micrometres off a bisector plane, 500 m from the origin.  Queries
whose first six ranks are not clearly apart are dropped, so the stored neighbours do not depend on how a backend breaks a
tie.  Numeric arrays only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402,F401  (installs the pykdtree shim and puts the reference on the path)
from point_cloud_registration.kdtree import KDTree  # noqa: E402  (the reference's seam)
import seam_f64_cases as sc  # noqa: E402


def g17():
    target, q = sc.case_a()
    tree = KDTree(target)
    d6, _ = tree.query(q, k=6)
    assert d6.dtype == np.float64
    keep = np.all((d6[:, 1:] - d6[:, :-1]) >= 1e-9 * d6[:, 1:], axis=1)
    assert keep.sum() >= 900, int(keep.sum())
    rows = np.nonzero(keep)[0]
    d1, i1 = tree.query(q[rows], k=1)
    d5, i5 = tree.query(q[rows], k=5)
    out = {"rows": rows.astype(np.int64), "query": q[rows],
           "k1_dist": np.asarray(d1, np.float64).reshape(-1), "k1_idx": np.asarray(i1, np.int64).reshape(-1),
           "k5_dist": np.asarray(d5, np.float64), "k5_idx": np.asarray(i5, np.int64)}
    path = os.path.join(HERE, "g17_seam_f64.npz")
    np.savez_compressed(path, **out)
    print(f"G17: {len(rows)} of {len(q)} queries kept, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    g17()
