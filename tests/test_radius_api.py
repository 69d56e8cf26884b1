"""Radius search, bounded k-NN and the outlier filters: the interface, its refusals, and the yardsticks of
tests/radius_cases.py against themselves.  Needs no GPU."""

import inspect

import numpy as np
import pytest

import point_cloud_registration_amd as pcr
from point_cloud_registration_amd import _capi

from radius_cases import brute_rows, cut_rows, planted_sheet, radius_ref_f64, sequential_mean

NEW_ENTRY_POINTS = ("pcr_radius_count", "pcr_radius_query", "pcr_radius_count_dd", "pcr_radius_query_dd", "pcr_knn_mean_distance")


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture()
def no_gpu(monkeypatch):
    """Any attempt to reach the library or a context fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the GPU was touched before the arguments were checked")
    monkeypatch.setattr(_capi, "lib", refuse)
    monkeypatch.setattr(_capi, "get_context", refuse)


def test_names_are_exported():
    for name in ("remove_radius_outliers", "remove_statistical_outliers"):
        assert name in pcr.__all__ and callable(getattr(pcr, name))
    assert list(inspect.signature(pcr.remove_radius_outliers).parameters) == ["points", "radius", "min_neighbors", "device"]
    p = inspect.signature(pcr.remove_statistical_outliers).parameters
    assert list(p) == ["points", "k", "std_ratio", "device"] and p["k"].default == 20 and p["std_ratio"].default == 2.0
    p = inspect.signature(pcr.KDTree.query_radius).parameters
    assert list(p) == ["self", "points", "r", "count_only"] and p["count_only"].default is False
    for name in ("radius_count", "radius_query", "knn_mean_distance"):
        assert callable(getattr(_capi.Target, name))


def test_prototypes_and_abi_version():
    for name in NEW_ENTRY_POINTS:
        assert name in _capi.PROTOTYPES, name
    assert len(_capi.PROTOTYPES["pcr_radius_query"][1]) == 7 and len(_capi.PROTOTYPES["pcr_radius_query_dd"][1]) == 7
    assert _capi.ABI_VERSION == 5


@pytest.mark.parametrize("r", [-1e-30, -1.0, np.nan, np.inf, -np.inf])
def test_bad_radius_is_refused_before_the_gpu(no_gpu, r):
    pts = np.zeros((4, 3), np.float32)
    tree = pcr.KDTree.__new__(pcr.KDTree)                      # (no device: the radius is checked first)
    with pytest.raises(ValueError, match="radius"):
        tree.query_radius(pts, r)
    with pytest.raises(ValueError, match="radius"):
        tree.query_radius(pts, r, count_only=True)
    target = _capi.Target.__new__(_capi.Target)
    with pytest.raises(ValueError, match="radius"):
        target.radius_count(pts, r)
    with pytest.raises(ValueError, match="radius"):
        target.radius_query(pts, r)
    with pytest.raises(ValueError, match="radius"):
        pcr.remove_radius_outliers(pts, r, 3)


def test_bad_filter_arguments_are_refused_before_the_gpu(no_gpu):
    pts = np.zeros((4, 3), np.float32)
    for bad in (-1, 2.5):
        with pytest.raises(ValueError, match="min_neighbors"):
            pcr.remove_radius_outliers(pts, 0.5, bad)
    for k in (0, 65, -3):
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            pcr.remove_statistical_outliers(pts, k=k)
    for s in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="std_ratio"):
            pcr.remove_statistical_outliers(pts, std_ratio=s)
    for shape in ((4,), (4, 2)):
        with pytest.raises(ValueError, match="shape"):
            pcr.remove_radius_outliers(np.zeros(shape), 0.5, 1)
        with pytest.raises(ValueError, match="shape"):
            pcr.remove_statistical_outliers(np.zeros(shape))


def test_empty_cloud_needs_no_gpu(no_gpu):
    for dtype in (np.float32, np.float64):
        e = np.zeros((0, 3), dtype)
        for kept, idx in (pcr.remove_radius_outliers(e, 0.5, 1), pcr.remove_statistical_outliers(e)):
            assert kept.shape == (0, 3) and kept.dtype == dtype and idx.shape == (0,) and idx.dtype == np.int64


# r -> (largest count, entries at exactly r), computed with the oracle on the lattice of constructed_cloud("lattice"): its
# coordinates are multiples of 0.25, so float32 arithmetic is exact there
LATTICE_PINS = {0.25: (7, 1632), 0.5: (37, 1486), 1.0: (272, 1180)}


@pytest.mark.parametrize("r", sorted(LATTICE_PINS))
def test_references_agree_on_the_lattice(orc, r):
    pts, q, d, i = brute_rows(orc, "lattice")
    dist, idx, off = cut_rows(d, i, r)
    counts = np.diff(off)
    assert (int(counts.max()), int(np.sum(dist == np.float32(r)))) == LATTICE_PINS[r]
    if r == 0.5:
        assert round(float(counts.mean()), 1) == 24.4 and int(np.sum(counts == 0)) == 50
    assert np.all(counts[450:] == 0)                           # the far group
    d64, i64, off64 = radius_ref_f64(pts, q, r)
    assert np.array_equal(off64, off) and np.array_equal(i64, idx)         # identical segments
    on = off[300]                                              # queries ON the lattice: d2 is exact in both, the roots round alike
    assert np.array_equal(d64[:on].astype(np.float32), dist[:on])
    assert np.allclose(d64, dist, rtol=1e-6, atol=0)
    assert d64.dtype == np.float64 and dist.dtype == np.float32 and idx.dtype == i64.dtype == off.dtype == np.int64
    for a, b in zip(off[:-1], off[1:]):                        # every segment ascending by (distance, index)
        assert np.all(np.diff(dist[a:b]) >= 0)
        assert np.all((np.diff(dist[a:b]) > 0) | (np.diff(idx[a:b]) > 0))


def test_sequential_mean_is_a_column_loop():
    """Nearest first in float64, over the finite entries -- not np.sum, whose pairwise order rounds differently."""
    rng = np.random.default_rng(5)
    # (distances over fourteen decades: float32 values of one magnitude add exactly in float64, in any order)
    d = np.sort((10.0 ** rng.uniform(-14, 0, (2000, 64))).astype(np.float32), axis=1)
    d[::7, 40:] = np.inf
    want = np.empty(len(d))
    for row in range(len(d)):
        s, c = 0.0, 0
        for v in d[row]:
            if np.isfinite(v):
                s, c = s + float(v), c + 1
        want[row] = s / c
    got = sequential_mean(d)
    assert np.array_equal(got, want)
    pairwise = np.where(np.isfinite(d), d, 0).astype(np.float64).sum(axis=1) / np.isfinite(d).sum(axis=1)
    assert np.any(pairwise != want), "the case does not tell the two orders apart"
    assert np.array_equal(sequential_mean(np.full((3, 4), np.inf, np.float32)), np.zeros(3))


def test_reference_drops_the_planted_points(orc):
    """The parameters of the filter test (radius 0.4, min_neighbors 3): the oracle's counts drop all 20 planted points."""
    cloud, planted = planted_sheet()
    d, _ = orc.knn_brute(cloud, cloud[planted], 8)
    others = (d <= np.float32(0.4)).sum(axis=1) - 1
    assert np.all(others < 3) and len(planted) == 20
