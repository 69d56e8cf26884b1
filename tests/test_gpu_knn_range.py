"""k-NN and normals over the rest of their range (csrc/knn_normals.hip): the LDS list KnnList at k = 21..64 (32 KB of
dynamic LDS per one-wave block at k = 64), clouds smaller than k, query counts around the one-wave block, the refusals
of check_k, normals at large k -- and, in a child process each, the documented switches PCR_KNN_REG=0 (the LDS list for
k <= 16 too) and PCR_KNN_SPARSE_FIRST=0 (normals in array order) under the suite's own k <= 16 assertions.
Distances and indices are bit-exact against brute force, ties ordered by the smaller original index."""

import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from test_gpu_parity import CONSTRUCTED_CLOUDS, _assert_smallest_eigvec, capi, constructed_cloud, ctx, orc  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clouds(capi, ctx):
    """name -> (points, queries, target): built once, shared by the tests below and left unchanged."""
    out = {}
    for case in CONSTRUCTED_CLOUDS:
        pts, q = constructed_cloud(case)
        out[case] = (pts, q, capi.Target.points(ctx, pts))
    return out


@pytest.fixture(scope="module")
def brute64(orc, clouds):
    """The 64 nearest neighbours of every query by brute force; the first k columns are the answer for k <= 64
    (the k-th best under the order (distance, index) does not depend on how many more are kept)."""
    return {case: orc.knn_brute(pts, q, 64) for case, (pts, q, _) in clouds.items()}


@pytest.mark.parametrize("case", CONSTRUCTED_CLOUDS)
@pytest.mark.parametrize("k", [21, 32, 33, 63, 64])
def test_knn_large_k(clouds, brute64, case, k):
    pts, q, t = clouds[case]
    d, i = t.knn_query(q, k)
    do, io = brute64[case]
    assert d.shape == i.shape == (len(q), k)
    assert np.array_equal(d, do[:, :k])
    assert np.array_equal(i, io[:, :k])


def test_brute_force_prefix_is_the_smaller_k(orc, clouds, brute64):
    """What brute64 relies on, on the cloud with the most ties."""
    pts, q, _ = clouds["lattice"]
    d, i = orc.knn_brute(pts, q, 33)
    assert np.array_equal(d, brute64["lattice"][0][:, :33]) and np.array_equal(i, brute64["lattice"][1][:, :33])


@pytest.mark.parametrize("k", [41, 64])
def test_knn_cloud_smaller_than_k(capi, orc, ctx, k):
    """n = 40 < k: the 40 points in order, then distance +inf and index n, the convention test_fuzz_knn pins at n = 3."""
    rng = np.random.default_rng(4100)
    pts = rng.uniform(-3, 3, (40, 3)).astype(np.float32)
    q = np.vstack([pts, rng.uniform(-5, 5, (60, 3)).astype(np.float32)])
    d, i = capi.Target.points(ctx, pts).knn_query(q, k)
    do, io = orc.knn_brute(pts, q, k)
    assert np.array_equal(d, do) and np.array_equal(i, io)
    assert np.all(np.isposinf(d[:, 40:])) and np.all(i[:, 40:] == 40)
    assert np.all(np.isfinite(d[:, :40])) and np.array_equal(np.sort(i[:, :40], axis=1), np.tile(np.arange(40), (100, 1)))


@pytest.mark.parametrize("m", [1, 63, 64, 65])
def test_knn_query_counts_around_one_block(clouds, brute64, m):
    pts, q, t = clouds["two_scales"]
    d, i = t.knn_query(q[:m], 33)
    assert np.array_equal(d, brute64["two_scales"][0][:m, :33]) and np.array_equal(i, brute64["two_scales"][1][:m, :33])


@pytest.mark.parametrize("k", [0, 65])
def test_k_out_of_range_is_refused(clouds, k):
    pts, q, t = clouds["sheet"]
    with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
        t.knn_query(q[:10], k)
    with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
        t.estimate_normals(k, compat=True)
    d, i = t.knn_query(q[:10], 1)                        # and the target still answers
    assert np.all(np.isfinite(d)) and np.all((i >= 0) & (i < len(pts)))


@pytest.mark.parametrize("case", ["sheet", "dense_spot"])
@pytest.mark.parametrize("k", [33, 64])
def test_normals_large_k(orc, clouds, case, k):
    pts, _, t = clouds[case]
    n_gpu = t.estimate_normals(k, compat=True)
    rows = np.arange(0, len(pts), max(len(pts) // 150, 1))
    _, ip = orc.knn_brute(pts, pts[rows], k)
    full = np.zeros((len(pts), k), np.int64)
    full[rows] = ip
    _assert_smallest_eigvec(pts, full, n_gpu, rows, f"{case} k={k}")
    assert np.allclose(np.linalg.norm(n_gpu, axis=1), 1, atol=1e-5)


@pytest.mark.parametrize("k", [33, 64])
def test_normals_large_k_g6(capi, orc, ctx, g6, k):
    pts = g6["points"]
    t = capi.Target.points(ctx, pts)
    d, i = t.knn_query(pts, k)
    do, io = orc.knn_brute(pts, pts, k)
    assert np.array_equal(i, io) and np.array_equal(d, do)
    n_gpu = t.estimate_normals(k, compat=True)
    n_orc = orc.normals_from_knn(pts, io, compat=True)
    dots = np.abs(np.sum(n_gpu.astype(np.float64) * n_orc, axis=1))
    print(f"g6 k={k}: {len(pts)} points, share of |dot| > 1 - 1e-6: {np.mean(dots > 1 - 1e-6):.5f}")
    assert np.mean(dots > 1 - 1e-6) >= 0.999            # same float32 covariance, same eigen-solver


@pytest.mark.parametrize("switches, expr", [
    ({"PCR_KNN_REG": "0", "PCR_KNN_SPARSE_FIRST": "0"}, "fuzz_knn or knn_constructed or knn_and_normals or normals_full_scale"),
    ({"PCR_KNN_SPARSE_FIRST": "0"}, "normals_full_scale")], ids=["list_for_every_k", "collect_in_array_order"])
def test_knn_switches_in_a_child_process(switches, expr):
    """PCR_KNN_REG and PCR_KNN_SPARSE_FIRST are read once per process, so a fresh one runs the suite's own k <= 16
    assertions: with both off, the LDS list in place of the collect path under every one of them; with
    PCR_KNN_SPARSE_FIRST=0 alone, the collect kernel in array order on the 1.06 M-point normals (the only cloud with
    more than 1024 blocks of 64 points, where the sparse-first order applies; with PCR_KNN_REG=0 the list kernel never
    reorders, so that branch needs a run of its own) against the same fixtures.  One child at a time."""
    env = dict(os.environ, **switches)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(REPO, "tests", "test_gpu_parity.py"), "-m", "gpu", "-x", "-q",
                        "-k", expr, "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=900, env=env, cwd=REPO)
    tail = r.stdout[-1500:]
    assert r.returncode == 0, tail + r.stderr[-500:]
    assert " passed" in tail and "skipped" not in tail.splitlines()[-1], tail
    print(tail.splitlines()[-1])
