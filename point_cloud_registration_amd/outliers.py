"""Outlier-removal filters for a cloud before ``set_target``: the radius and the statistical filter of Open3D / PCL, on the
MI355X.  The reference has no counterpart; both are one search away from kernels the library has (csrc/radius.hip).

Both build a point index over the cloud and search the **float32 copy** of the points, whatever dtype the array has; the
points returned are rows of the caller's array, in its dtype.
"""

import numpy as np

from . import _capi


def _keep(points, mask):
    kept_idx = np.flatnonzero(mask).astype(np.int64)
    return points[kept_idx], kept_idx


def remove_radius_outliers(points, radius, min_neighbors, device=None):
    """Keep a point iff at least ``min_neighbors`` OTHER points lie within ``radius`` of it (duplicates of the point count):
    ``count - 1 >= min_neighbors`` with ``count`` from the exact radius search, which finds the point itself.

    -> ``(kept_points, kept_idx)``: rows of ``points`` in the caller's dtype and their ascending int64 indices.  The search
    runs over the float32 copy of the points."""
    points = np.asarray(points)
    xyz = _capi.cloud_f32(points, "points", finite=False)
    radius = _capi.check_radius(radius)
    if int(min_neighbors) != min_neighbors or min_neighbors < 0:
        raise ValueError("min_neighbors must be an integer >= 0")
    if len(points) == 0:
        return _keep(points, np.zeros(0, bool))
    count = _capi.Target.points(_capi.get_context(device), xyz).radius_count(xyz, radius)
    return _keep(points, count - 1 >= int(min_neighbors))


def remove_statistical_outliers(points, k=20, std_ratio=2.0, device=None):
    """Keep a point iff its mean distance to its ``k`` nearest neighbours (itself included, as for normals and covariances;
    1 <= k <= 64) is at most ``mu + std_ratio * sigma``, with ``mu = np.mean`` and ``sigma = np.std`` of those means over
    the cloud.  The means come from the GPU (float32 distances summed in float64), the statistics from the host.

    -> ``(kept_points, kept_idx)``: rows of ``points`` in the caller's dtype and their ascending int64 indices.  The search
    runs over the float32 copy of the points."""
    points = np.asarray(points)
    xyz = _capi.cloud_f32(points, "points", finite=False)
    k = _capi.check_k(k)
    std_ratio = float(std_ratio)
    if not np.isfinite(std_ratio):
        raise ValueError("std_ratio must be finite")
    if len(points) == 0:
        return _keep(points, np.zeros(0, bool))
    mean_d = _capi.Target.points(_capi.get_context(device), xyz).knn_mean_distance(k)
    return _keep(points, mean_d <= np.mean(mean_d) + std_ratio * np.std(mean_d))
