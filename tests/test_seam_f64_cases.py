"""The inputs of tests/seam_f64_cases.py can tell a float64 query seam from a float32 one (CPU only): on each of them the
answer changes in hundreds of rows when the query, or query and target, are rounded to float32 -- and never through the tie
rule, so a GPU result that equals the brute force got there by the float64 distances alone."""
import numpy as np
import pytest

import seam_f64_cases as sc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _rounded(q):
    return q.astype(np.float32).astype(np.float64)


def test_case_a_rounding_the_query_moves_the_neighbour():
    target, q = sc.case_a()
    d, i = sc.brute(target, q, 6)
    _, ir = sc.brute(target, _rounded(q), 1)
    differ = int((i[:, 0] != ir[:, 0]).sum())
    print(f"case A: {differ} of {len(q)} nearest neighbours differ once the query is rounded to float32")
    assert differ >= 200
    assert sc.distinct_ranks(d)
    gap = float(np.min((d[:, 1:] - d[:, :-1]) / d[:, 1:]))
    print(f"case A: smallest relative gap between consecutive ranks {gap:.2e}")


def test_case_b_pairs_collapse_in_float32(orc):
    target, q = sc.case_b()
    t32 = target.astype(np.float32)
    same = int(np.all(t32[0::2] == t32[1::2], axis=1).sum())
    print(f"case B: {same} of 2000 pairs are one point in float32")
    assert same >= 1000
    d65, i65 = sc.brute(target, q, 65)
    assert sc.distinct_ranks(d65)
    for k, least in ((1, 200), (4, 300), (17, 800), (64, 900)):
        _, i32 = orc.knn_brute(t32, q.astype(np.float32), k)
        differ = int(np.any(i65[:, :k] != i32, axis=1).sum())
        print(f"case B, k = {k}: {differ} of {len(q)} rows differ from the all-float32 answer")
        assert differ >= least, k


def test_case_c_centroids(orc):
    vox = orc.TargetVoxels(sc.case_c_cloud(), 1.0)
    means = np.asarray(vox.mean, np.float64)
    assert means.shape == (1493, 3) and np.abs(means).max() < 16.0          # (one float32 binade: steps of 1e-6 m at the rim)
    q = sc.case_c_queries(means)
    d, i = sc.brute(means, q, 21)
    _, ir = sc.brute(means, _rounded(q), 1)
    differ = int((i[:, 0] != ir[:, 0]).sum())
    print(f"case C: {differ} of {len(q)} nearest centroids differ once the query is rounded to float32")
    assert differ >= 30
    assert sc.distinct_ranks(d)
