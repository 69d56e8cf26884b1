"""Inputs of the float64 query seam tests (pure NumPy): three targets with float64 queries placed where rounding the query,
or the target, to float32 changes the answer, and the brute force they are compared with.

The brute force uses the library's own distance expression, ``(dx*dx + dy*dy) + dz*dz`` with ``dx = q - p`` in float64, and
orders by (distance, index): the GPU kernels must agree with it bit for bit (tests/test_gpu_seam_f64.py);
tests/test_seam_f64_cases.py pins, on the CPU, that the inputs can tell a float64 search from a float32 one."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OFFSET = np.array([500.0, -300.0, 20.0])


def brute(target, q, k):
    """The k nearest of every query: (squared distances (m, k), indices (m, k)), rows in (distance, index) order, padded
    with (inf, n) when the target holds fewer than k points."""
    target, q = np.asarray(target, np.float64), np.asarray(q, np.float64)
    n = target.shape[0]
    dx = q[:, None, 0] - target[None, :, 0]
    dy = q[:, None, 1] - target[None, :, 1]
    dz = q[:, None, 2] - target[None, :, 2]
    with np.errstate(over="ignore"):
        d2 = (dx * dx + dy * dy) + dz * dz
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]            # stable: equal distances stay in index order
    d = np.take_along_axis(d2, order, axis=1)
    if k > n:
        d = np.hstack([d, np.full((q.shape[0], k - n), np.inf)])
        order = np.hstack([order, np.full((q.shape[0], k - n), n, order.dtype)])
    return d, order.astype(np.int64)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _nearest_other(points):
    d, i = brute(points, points, 2)
    assert np.all(i[:, 0] == np.arange(points.shape[0])) and np.all(d[:, 1] > 0), "duplicate points"
    return i[:, 1]


@functools.lru_cache(maxsize=None)
def case_a():
    """The g9 target (5000 float64 points near (500, -300, 20)) and 1000 queries next to the bisector plane of a target
    point and its nearest neighbour, a few micrometres to either side: a float32 step there is 3e-5 m."""
    target = np.load(os.path.join(GOLDEN, "g9_q6_f64_target.npz"))["target"]
    assert target.dtype == np.float64 and target.shape == (5000, 3)
    rng = np.random.default_rng(21)
    pick = rng.choice(target.shape[0], 1000, replace=False)
    a, b = target[pick], target[_nearest_other(target)[pick]]
    q = (a + b) / 2 + _unit(b - a) * rng.normal(0.0, 3e-6, (1000, 1))
    return target, q


@functools.lru_cache(maxsize=None)
def case_b():
    """2000 points in a +-10 m cube at (500, -300, 20), each with a twin 1e-6 m away (interleaved: 4000 points; most pairs
    are one point in float32), and 1000 queries on the line through a pair: 3e-7 m before the first point, or 7.5e-7 m
    towards its twin."""
    rng = np.random.default_rng(7)
    base = rng.uniform(-10.0, 10.0, (2000, 3)) + OFFSET
    u = _unit(rng.normal(size=(2000, 3)))
    target = np.empty((4000, 3))
    target[0::2], target[1::2] = base, base + 1e-6 * u
    q = base[:1000] + 3e-7 * u[:1000] * rng.choice([-1.0, 2.5], (1000, 1))
    return target, q


def case_c_cloud():
    from point_cloud_registration_amd.synthetic import street
    return street(120_000, seed=3) * np.float32(0.25)


def case_c_queries(means):
    """800 queries for the centroids of VoxelGrid(1.0) over ``case_c_cloud()``: midpoints between a centroid and its
    nearest other centroid, moved along the pair by a few tenths of a micrometre."""
    means = np.asarray(means, np.float64)
    rng = np.random.default_rng(31)
    pick = rng.choice(means.shape[0], 800, replace=False)
    a, b = means[pick], means[_nearest_other(means)[pick]]
    return (a + b) / 2 + _unit(b - a) * rng.normal(0.0, 3e-7, (800, 1))


def distinct_ranks(d2):
    """True when no two consecutive columns of a brute-force result hold the same distance (the tie rule decides nothing)."""
    return bool(np.all(d2[:, 1:] > d2[:, :-1]))
