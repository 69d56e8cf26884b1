"""ISS keypoints on the MI355X (Zhong 2009; what Open3D's ``compute_iss_keypoints`` does): the points of a cloud whose
neighbourhood has three clearly different extents and whose smallest one is a local maximum.  Kernels in
``csrc/keypoints.hip``, definitions in ``include/pcr.h``.  The reference has no counterpart.

A global registration computes its descriptors at these points only (``compute_fpfh_rows``,
``register_global(keypoints="iss")``) and matches a few thousand rows instead of every point.

Keypoints are computed over the **float32 copy** of the points, whatever dtype the array has, and the same call twice
returns the same rows.
"""

import numpy as np

from . import _capi


def _radius_or_none(r, name):
    if r is None:
        return None
    try:
        return _capi.check_radius(r)
    except ValueError:
        raise ValueError(f"{name} must be finite and >= 0, got {float(r)}") from None


def iss_radii(target, salient_radius=None, non_max_radius=None):
    """The two radii of ``iss_keypoints`` as float32 values: ``None`` -> 6 x (salient) and 4 x (non-maximum) the resolution of
    the target's cloud, resolution = 2 x the mean of ``knn_mean_distance(2)`` in float64 (that mean counts the point itself
    at distance 0)."""
    if salient_radius is None or non_max_radius is None:
        resolution = 2.0 * float(np.mean(target.knn_mean_distance(2), dtype=np.float64))
        if salient_radius is None:
            salient_radius = 6.0 * resolution
        if non_max_radius is None:
            non_max_radius = 4.0 * resolution
    return float(np.float32(salient_radius)), float(np.float32(non_max_radius))


def iss_keypoints(points, salient_radius=None, non_max_radius=None, gamma_21=0.975, gamma_32=0.975, min_neighbors=5,
                  return_saliency=False, device=None):
    """ISS keypoints of ``points`` (N, 3): ascending int64 row indices; with ``return_saliency`` also the (N,) float64
    saliency of every point (the smallest eigenvalue of its scatter matrix where the point is salient, else 0).

    A point is salient when its ``salient_radius`` ball holds at least ``min_neighbors`` points (itself included) and the
    eigenvalues l1 >= l2 >= l3 of their scatter matrix satisfy l2 < ``gamma_21`` l1, l3 < ``gamma_32`` l2 and l3 > 0; it is a
    keypoint when it is salient, its ``non_max_radius`` ball holds at least ``min_neighbors`` points and no other point in
    that ball has a larger saliency (an exact tie goes to the smaller row index).  A radius of ``None``: 6 x (salient) and 4 x
    (non-maximum) the cloud's resolution -- twice the mean distance of ``knn_mean_distance(2)``."""
    xyz = _capi.cloud_f32(points, "points")
    salient_radius = _radius_or_none(salient_radius, "salient_radius")
    non_max_radius = _radius_or_none(non_max_radius, "non_max_radius")
    g21, g32, mn = _capi.check_iss(gamma_21, gamma_32, min_neighbors)
    if len(xyz) == 0:
        rows = np.zeros(0, np.int64)
        return (rows, np.zeros(0, np.float64)) if return_saliency else rows
    target = _capi.Target.points(_capi.get_context(device), xyz)
    rs, rn = iss_radii(target, salient_radius, non_max_radius)
    res = target.iss_keypoints(rs, rn, g21, g32, mn, want_saliency=return_saliency)
    if return_saliency:
        return np.flatnonzero(res[0]).astype(np.int64), res[1]
    return np.flatnonzero(res).astype(np.int64)
