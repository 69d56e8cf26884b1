"""Exact radius search (csrc/radius.hip), the bounded k-NN of KDTree.query, the mean k-NN distance and the outlier filters on
the GPU: offsets, indices and distances bit-equal to the yardsticks of tests/radius_cases.py -- the oracle's brute force over
the whole target cut at d <= r for float32, a NumPy brute force for float64."""

import os
import subprocess
import sys

import numpy as np
import pytest

import point_cloud_registration_amd as pcr

from conftest import REPO
from radius_cases import (RADII, bounded_knn_ref, brute_rows, cut_rows, mean_distance_ref, planted_sheet, radius_ref_f32, radius_ref_f64,
                          sequential_mean, shifted_two_scales)
from test_gpu_parity import CONSTRUCTED_CLOUDS, capi, ctx, orc  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def targets(capi, orc, ctx):
    """case -> point target over the case's cloud: built once, shared and left unchanged."""
    return {case: capi.Target.points(ctx, brute_rows(orc, case)[0]) for case in CONSTRUCTED_CLOUDS}


def assert_csr_equal(got, want):
    (d, i, off), (dr, ir, offr) = got, want
    assert off.dtype == i.dtype == np.int64 and d.dtype == dr.dtype
    assert np.array_equal(off, offr)
    assert np.array_equal(i, ir)
    assert np.array_equal(d, dr)


@pytest.mark.parametrize("case, r", [(c, r) for c in CONSTRUCTED_CLOUDS for r in RADII[c]])
def test_radius_constructed_cases(orc, targets, case, r):
    pts, q, d, i = brute_rows(orc, case)
    want = cut_rows(d, i, r)
    t = targets[case]
    counts = t.radius_count(q, r)
    assert counts.dtype == np.int64 and np.array_equal(counts, np.diff(want[2]))
    assert_csr_equal(t.radius_query(q, r), want)
    assert np.all(counts[450:] == 0)                                     # the far group
    print(f"{case} r={r}: {int(want[2][-1])} entries, longest segment {int(counts.max())}, at exactly r {int(np.sum(want[0] == np.float32(r)))}")
    if (case, r) == ("lattice", 10.0):
        assert np.all(counts[:450] == 1728)
    if (case, r) == ("dense_spot", 0.01):
        assert counts[96] == 4426 and counts.max() == 4446               # the long segments
    if (case, r) == ("duplicates", 0.0):
        assert int(np.sum(want[0] == 0)) == len(want[0]) == 770


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65])
def test_radius_query_counts_around_one_block(orc, targets, m):
    pts, q, d, i = brute_rows(orc, "two_scales")
    t = targets["two_scales"]
    want = cut_rows(d[:m], i[:m], 0.2) if m else (np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(1, np.int64))
    assert np.array_equal(t.radius_count(q[:m], 0.2), np.diff(want[2]))
    assert_csr_equal(t.radius_query(q[:m], 0.2), want)


def test_radius_small_and_empty_clouds(capi, orc, ctx):
    rng = np.random.default_rng(4100)
    pts = rng.uniform(-3, 3, (40, 3)).astype(np.float32)
    q = np.vstack([pts, rng.uniform(-5, 5, (60, 3)).astype(np.float32)])
    t = capi.Target.points(ctx, pts)
    for r in (0.0, 1.5, 20.0):
        assert_csr_equal(t.radius_query(q, r), radius_ref_f32(orc, pts, q, r))
    assert np.array_equal(t.radius_count(q, 20.0), np.full(100, 40))
    empty = pcr.KDTree(np.zeros((0, 3), np.float32))
    assert np.array_equal(empty.query_radius(q, 1.0, count_only=True), np.zeros(100, np.int64))
    d, i, off = empty.query_radius(q, 1.0)
    assert len(d) == len(i) == 0 and np.array_equal(off, np.zeros(101, np.int64))


def test_nan_and_far_queries(orc, targets):
    pts, q, d, i = brute_rows(orc, "sheet")
    t = targets["sheet"]
    bad = q.copy()
    bad[5, 1] = np.nan
    bad[64, 0] = np.inf
    want_d, want_i, want_off = cut_rows(d, i, 0.4)
    counts = np.diff(want_off)
    assert counts[5] > 0 and counts[64] > 0
    got_d, got_i, got_off = t.radius_query(bad, 0.4)
    got_counts = np.diff(got_off)
    assert got_counts[5] == 0 and got_counts[64] == 0
    counts[[5, 64]] = 0
    assert np.array_equal(got_counts, counts) and np.all(got_counts[450:] == 0)
    keep = np.ones(len(want_d), bool)
    for row in (5, 64):
        keep[want_off[row]:want_off[row + 1]] = False
    assert np.array_equal(got_d, want_d[keep]) and np.array_equal(got_i, want_i[keep])


@pytest.mark.parametrize("delta", [-1, 1], ids=["short", "long"])
def test_offsets_that_do_not_match_are_refused(capi, orc, targets, delta):
    """One segment a single entry short / long: an error, and the output arrays keep their sentinels."""
    pts, q, d, i = brute_rows(orc, "duplicates")
    t = targets["duplicates"]
    _, _, off = cut_rows(d, i, 0.3)
    row = int(np.argmax(np.diff(off) > 2))
    wrong = off.copy()
    wrong[row + 1:] += delta
    dist = np.full(int(off[-1]) + 1, -7.0, np.float32)
    idx = np.full(int(off[-1]) + 1, -7, np.int64)
    with pytest.raises(ValueError, match="offsets"):
        t.radius_query(q, 0.3, offsets=wrong, out=(dist, idx))
    assert np.all(dist == -7.0) and np.all(idx == -7)
    for bad in (off + 1, off[::-1].copy()):                              # not starting at 0, decreasing
        with pytest.raises(ValueError, match="offsets"):
            t.radius_query(q, 0.3, offsets=bad, out=(dist, idx))
    assert np.all(dist == -7.0) and np.all(idx == -7)
    got = t.radius_query(q, 0.3, offsets=off, out=(dist, idx))            # and the target still answers
    assert np.array_equal(got[0][:off[-1]], cut_rows(d, i, 0.3)[0]) and got[0][-1] == -7.0


def test_refusals_of_the_library(capi, ctx, targets):
    t = targets["sheet"]
    q = np.zeros((3, 3), np.float32)
    L = capi.lib()
    cnt, off = np.zeros(3, np.int64), np.zeros(4, np.int64)
    for r in (-1.0, np.nan, np.inf):
        assert L.pcr_radius_count(t.handle, q, 3, r, cnt) == capi.PCR_ERR_INVALID
        assert L.pcr_radius_query(t.handle, q, 3, r, off, np.zeros(1, np.float32), np.zeros(1, np.int64)) == capi.PCR_ERR_INVALID
    # the _dd pair on a float32-only point target, as pcr_knn_query_f64
    assert L.pcr_radius_count_dd(t.handle, q.astype(np.float64), 3, 1.0, cnt) == capi.PCR_ERR_INVALID
    assert L.pcr_radius_query_dd(t.handle, q.astype(np.float64), 3, 1.0, off, np.zeros(1), np.zeros(1, np.int64)) == capi.PCR_ERR_INVALID
    vox = capi.Target.voxels(ctx, np.random.default_rng(3).uniform(-2, 2, (5000, 3)).astype(np.float32), 1.0)
    assert L.pcr_radius_count(vox.handle, q, 3, 1.0, cnt) == capi.PCR_ERR_INVALID
    assert L.pcr_radius_count_dd(vox.handle, q.astype(np.float64), 3, 1.0, cnt) == capi.PCR_ERR_INVALID
    assert L.pcr_knn_mean_distance(vox.handle, 5, np.zeros(500)) == capi.PCR_ERR_INVALID
    for k in (0, 65):
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            t.knn_mean_distance(k)
    assert L.pcr_radius_count(t.handle, q[:0].copy(), 0, 1.0, cnt[:0].copy()) == capi.PCR_OK


def test_radius_float64(orc):
    """A float64 tree: float64 queries as they are, float32 queries widened exactly, both through the _dd pair."""
    pts64, q64, q32 = shifted_two_scales()
    tree = pcr.KDTree(pts64)
    assert tree._target.searches_f64()
    for r in (0.1, 0.2):
        for q in (q64, q32):
            d, i, off = tree.query_radius(q, r)
            assert d.dtype == np.float64
            assert_csr_equal((d, i, off), radius_ref_f64(pts64, q, r))
            assert np.array_equal(tree.query_radius(q, r, count_only=True), np.diff(off))
    # the jitter matters: the float32 copy of the same cloud gives other segments somewhere
    tree32 = pcr.KDTree(pts64.astype(np.float32))
    d32, i32, off32 = tree32.query_radius(q64, 0.2)                       # (rounds the float64 queries, as query does)
    assert d32.dtype == np.float32
    assert_csr_equal((d32, i32, off32), radius_ref_f32(orc, pts64.astype(np.float32), q64.astype(np.float32), 0.2))


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join({repo!r}, "tests"))
sys.path.insert(0, {repo!r})
from point_cloud_registration_amd import _capi
from test_gpu_parity import constructed_cloud
out = {{}}
for case, r in {jobs!r}:
    pts, q = constructed_cloud(case)
    t = _capi.Target.points(_capi.get_context(0), pts)
    d, i, off = t.radius_query(q, r)
    out[case + "_d"], out[case + "_i"], out[case + "_off"], out[case + "_heavy"] = d, i, off, np.array(t.index_info()["heavy"])
np.savez({path!r}, **out)
"""


@pytest.mark.parametrize("env, jobs", [({"PCR_RADIUS_CHUNK": "4096"}, [("dense_spot", 0.01)]),
                                       ({"PCR_RADIUS_CHUNK": "4096", "PCR_HEAVY": "1"}, [("dense_spot", 0.01), ("two_scales", 0.2)])],
                         ids=["chunks", "chunks_heavy_index"])
def test_chunked_calls_return_the_same_bits(orc, env, jobs, tmp_path):
    """PCR_RADIUS_CHUNK is read once per process, so a fresh one runs the search in chunks of at most 4096 entries -- the
    4426-entry segment of dense_spot as a chunk of its own -- also over the heavy-cell form of the index."""
    path = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, "-c", CHILD.format(repo=REPO, jobs=jobs, path=path)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **env), cwd=REPO)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    got = np.load(path)
    for case, rad in jobs:
        _, _, d, i = brute_rows(orc, case)
        assert_csr_equal((got[case + "_d"], got[case + "_i"], got[case + "_off"]), cut_rows(d, i, rad))
        assert bool(got[case + "_heavy"]) or "PCR_HEAVY" not in env


def knn_ref_f64(pts, q, k):
    pts, q = np.asarray(pts, np.float64), np.asarray(q, np.float64)
    d, i = np.empty((len(q), k)), np.empty((len(q), k), np.int64)
    n = np.arange(len(pts))
    for row, qi in enumerate(q):
        dx, dy, dz = qi[0] - pts[:, 0], qi[1] - pts[:, 1], qi[2] - pts[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        order = np.lexsort((n, d2))[:k]
        d[row], i[row] = np.sqrt(d2[order]), order
    return d, i


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bounded_knn(orc, dtype):
    """query(q, k > 1, distance_upper_bound = r): the k-NN rows with entries `not (d < r)` set to (inf, n)."""
    pts, q, d, i = brute_rows(orc, "two_scales")
    q = q[:450]
    tree = pcr.KDTree(pts.astype(dtype))
    d64, i64 = (d[:450, :64], i[:450, :64]) if dtype == np.float32 else knn_ref_f64(pts, q, 64)
    plain_d, plain_i = tree.query(q, k=33)
    assert np.array_equal(plain_d, d64[:, :33]) and np.array_equal(plain_i, i64[:, :33])      # the default is the call it always was
    for r in (0.2, float(d64[7, 5])):                                    # (a bound that IS a distance: strictly below)
        want_d, want_i = bounded_knn_ref(d64, i64, 33, r, len(pts))
        got_d, got_i = tree.query(q, k=33, distance_upper_bound=r)
        assert got_d.dtype == dtype and np.array_equal(got_d, want_d) and np.array_equal(got_i, want_i)
        assert np.any(np.isinf(want_d)) and np.any(np.isfinite(want_d))
        cut = np.isinf(got_d)
        assert np.all(cut[:, 1:] >= cut[:, :-1])                         # the masked entries are a suffix


@pytest.fixture(scope="module")
def self_rows(orc):
    """case -> the 64 nearest neighbours of every point within its own cloud (first k columns: the answer for k <= 64)."""
    return {case: orc.knn_brute(brute_rows(orc, case)[0], brute_rows(orc, case)[0], 64)[0] for case in ("two_scales", "duplicates")}


@pytest.mark.parametrize("case", ["two_scales", "duplicates"])
@pytest.mark.parametrize("k", [1, 8, 16, 17, 64])
def test_knn_mean_distance(targets, self_rows, case, k):
    got = targets[case].knn_mean_distance(k)
    assert got.dtype == np.float64 and np.array_equal(got, sequential_mean(self_rows[case][:, :k]))
    if k == 1:
        assert np.all(got == 0)


def test_knn_mean_distance_cloud_smaller_than_k(capi, orc, ctx):
    pts = np.random.default_rng(4100).uniform(-3, 3, (40, 3)).astype(np.float32)
    got = capi.Target.points(ctx, pts).knn_mean_distance(64)
    assert np.array_equal(got, mean_distance_ref(orc, pts, 64))           # 40 found: the sum over 40, divided by 40


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_outlier_filters(orc, dtype):
    cloud32, planted = planted_sheet()
    cloud = cloud32.astype(dtype)
    d8, _ = orc.knn_brute(cloud32, cloud32, 8)
    keep = (d8 <= np.float32(0.4)).sum(axis=1) - 1 >= 3                  # (eight columns decide "at least four within r")
    kept, idx = pcr.remove_radius_outliers(cloud, radius=0.4, min_neighbors=3)
    assert idx.dtype == np.int64 and kept.dtype == dtype
    assert np.array_equal(idx, np.flatnonzero(keep)) and np.array_equal(kept, cloud[idx])
    assert not np.any(np.isin(planted, idx)) and len(idx) > 5000          # all 20 planted points are dropped
    mean_d = mean_distance_ref(orc, cloud32, 20)
    keep = mean_d <= np.mean(mean_d) + 2.0 * np.std(mean_d)
    kept, idx = pcr.remove_statistical_outliers(cloud, k=20, std_ratio=2.0)
    assert idx.dtype == np.int64 and kept.dtype == dtype
    assert np.array_equal(idx, np.flatnonzero(keep)) and np.array_equal(kept, cloud[idx])
    assert not np.any(np.isin(planted, idx)) and 0 < len(idx) < len(cloud)


def test_repeat_and_non_interference(capi, orc, ctx, targets):
    """A repeated call returns the same bits, and a pass over the same target is not disturbed by a radius call."""
    pts, q, _, _ = brute_rows(orc, "two_scales")
    t = targets["two_scales"]
    scan = capi.Scan(ctx, q[:450])
    T = np.eye(4)
    before = capi.linearize(t, scan, capi.ICP, T, 1.0)
    a = t.radius_query(q, 0.2)
    m = t.knn_mean_distance(17)
    after = capi.linearize(t, scan, capi.ICP, T, 1.0)
    b = t.radius_query(q, 0.2)
    assert np.array_equal(before, after) and np.any(before != 0)
    assert_csr_equal(a, b)
    assert np.array_equal(m, t.knn_mean_distance(17))
