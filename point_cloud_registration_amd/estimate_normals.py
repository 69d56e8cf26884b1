"""k-NN PCA normals with the reference's interface (``estimate_normals.py:11-110``), and the same from a ball."""

import numpy as np

from . import _capi
from .kdtree import KDTree


def estimate_normals(points, k=15, compat=True, radius=None, max_nn=None, return_counts=False):
    """Normals (N,3) float32 from the k nearest neighbours of every point (GPU).

    ``radius``: from every point within ``radius`` of the point instead (``max_nn``: its nearest ``max_nn`` of them, at most
    64) -- ``k`` and ``compat`` are then not read.  On a LiDAR sweep the k nearest neighbours lie on the point's own ring
    line; a ball wide enough to reach the next ring does not.  A point with fewer than three points in its ball gets the zero
    normal.  ``return_counts=True`` appends the number of points each normal was estimated from, (N,) int64."""
    _check_neighbourhood(radius, max_nn)
    tree = KDTree(points)
    return estimate_norm_with_tree(points, tree, k=k, compat=compat, radius=radius, max_nn=max_nn, return_counts=return_counts)


def estimate_norm_with_tree(points, kdtree, k=15, compat=True, radius=None, max_nn=None, return_counts=False):
    """``compat=True`` keeps the reference's float32 single-pass covariance
    (estimate_normals.py:56-72); ``False`` uses a centred float64 covariance.  ``radius`` / ``max_nn`` / ``return_counts``:
    as ``estimate_normals``."""
    _check_neighbourhood(radius, max_nn)
    points = np.asarray(points)
    if not isinstance(kdtree, KDTree) or kdtree.n != points.shape[0]:
        kdtree = KDTree(points)
    if radius is not None:
        return kdtree._target.estimate_normals_radius(radius, max_nn, want_counts=return_counts)
    normals = kdtree._target.estimate_normals(k, compat=compat)
    return (normals, np.full(points.shape[0], min(int(k), points.shape[0]), np.int64)) if return_counts else normals


def _check_neighbourhood(radius, max_nn):
    """``radius`` / ``max_nn`` as every class takes them: both None (the k nearest neighbours), or a ball (``_capi.check_ball``)."""
    if radius is None and max_nn is None:
        return None
    return _capi.check_ball(radius, max_nn)


def ball_moments(points, radius, max_nn=None):
    """The moments the ball estimates start from -> (count (N,) int64, mean (N, 3) float64, cov (N, 3, 3) float64): of every
    point's neighbours within ``radius`` (its nearest ``max_nn`` of them), the point itself included; ``include/pcr.h`` states
    the arithmetic."""
    _capi.check_ball(radius, max_nn)
    points = _capi.cloud_f32(points, "points", finite=False)
    count, mean, c = KDTree(points)._target.ball_moments(radius, max_nn)
    return count, mean, c[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def get_norm_lines(points, normals, length=0.1):
    """Line segments point -> point + length * normal for visualisation (estimate_normals.py:91-106)."""
    points = np.asarray(points)
    lines = np.empty((2 * points.shape[0], points.shape[1]), dtype=points.dtype)
    lines[0::2] = points
    lines[1::2] = points + np.asarray(normals) * length
    return lines
