"""FPFH descriptors and exact descriptor matching on the MI355X: the first two thirds of a global registration (what Open3D's
``compute_fpfh_feature`` and a nearest-neighbour search over the features do), kernels in ``csrc/fpfh.hip``, definitions in
``include/pcr.h``.  The reference has no counterpart.  Pose hypotheses from the matches: ``global_registration.py``
(``ransac_pose``, ``register_global``).

Descriptors are computed over the **float32 copy** of the points, whatever dtype the array has.
"""

import numpy as np

from . import _capi


def compute_fpfh(points, normals=None, radius=None, k_normals=15, device=None):
    """FPFH descriptors (N, 33) float32 of ``points`` at ``radius``: for every point the histogram of its own pair features
    plus the distance-weighted, normalised histograms of its neighbours, three blocks of 11 bins that each sum to 200 (a point
    with no neighbour inside the radius gets a zero row).  ``normals`` (N, 3), or ``None`` to estimate them from the
    ``k_normals`` nearest neighbours as ``estimate_normals`` does.  Descriptors at some rows only: ``compute_fpfh_rows``."""
    return _fpfh(points, normals, radius, k_normals, device, None)


def compute_fpfh_rows(points, rows, normals=None, radius=None, k_normals=15, device=None):
    """``compute_fpfh(points, normals, radius, ...)[rows]``, bit for bit, without computing or copying back the other rows'
    second pass: ``rows`` are integer row indices into ``points`` in any order, with no repeats; -> (len(rows), 33) float32 in
    the order given.  (The first pass still covers the whole cloud: the neighbours' histograms are needed.)"""
    rows = np.asarray(rows)
    if rows.ndim != 1:
        raise ValueError("rows must be a vector of row indices")
    if len(rows) and not np.issubdtype(rows.dtype, np.integer):
        raise ValueError("rows must be integer row indices")
    return _fpfh(points, normals, radius, k_normals, device, rows.astype(np.int64))


def _fpfh(points, normals, radius, k_normals, device, rows):
    points = _capi.cloud_f32(points, "points")
    if radius is None:
        raise ValueError("radius is required")
    radius = _capi.check_radius(radius)
    if normals is not None:
        normals = _capi.cloud_f32(normals, "normals")
        if normals.shape != points.shape:
            raise ValueError("normals must have the shape of points")
    else:
        k_normals = _capi.check_k(k_normals)
    order = None
    if rows is not None:
        if len(rows) and (rows.min() < 0 or rows.max() >= len(points)):
            raise ValueError("rows point outside points")
        order = np.argsort(rows, kind="stable")
        rows = np.ascontiguousarray(rows[order])
        if np.any(rows[1:] == rows[:-1]):
            raise ValueError("rows must not repeat")
    if len(points) == 0 or (rows is not None and len(rows) == 0):
        return np.zeros((0, 33), np.float32)
    target = _capi.Target.points(_capi.get_context(device), points, normals)
    if normals is None:
        target.estimate_normals(k_normals, want=False)
    if rows is None:
        return target.fpfh(radius)
    out = np.empty((len(rows), 33), np.float32)
    out[order] = target.fpfh(radius, rows=rows)                          # (sorted on the host, un-sorted here)
    return out


def select_matches(idx_ab, d2_first, d2_second, idx_ba=None, mutual=True, ratio=None):
    """The selection rule of ``match_features`` on the host: from the nearest row of B for every row of A (``idx_ab``, with
    the squared distances of the nearest and the second nearest) and, for ``mutual``, the nearest row of A for every row of B
    (``idx_ba``) -> ``(ia, ib, d2)``, ascending ``ia``.

    ``mutual`` keeps (i, j) iff ``idx_ba[idx_ab[i]] == i``; ``ratio`` keeps i iff ``d2_first <= ratio**2 * d2_second``,
    compared in float64 (Lowe's test on the distances; a second distance of inf passes).  Rows without a match
    (``idx_ab < 0``) are dropped."""
    idx_ab = np.asarray(idx_ab, np.int64)
    d2_first, d2_second = np.asarray(d2_first), np.asarray(d2_second)
    if not idx_ab.shape == d2_first.shape == d2_second.shape or idx_ab.ndim != 1:
        raise ValueError("idx_ab, d2_first and d2_second must be vectors of one length")
    keep = idx_ab >= 0
    if mutual:
        if idx_ba is None:
            raise ValueError("mutual selection needs idx_ba")
        idx_ba = np.asarray(idx_ba, np.int64)
        if np.any(idx_ab >= len(idx_ba)):
            raise ValueError("idx_ab points past idx_ba")
        back = np.full(len(idx_ab), -1, np.int64)
        back[keep] = idx_ba[idx_ab[keep]]
        keep &= back == np.arange(len(idx_ab))
    if ratio is not None:
        ratio = float(ratio)
        if not (np.isfinite(ratio) and ratio >= 0):
            raise ValueError("ratio must be finite and >= 0")
        with np.errstate(invalid="ignore"):                              # (0 * inf: NaN, not kept)
            keep &= d2_first.astype(np.float64) <= ratio * ratio * d2_second.astype(np.float64)
    ia = np.flatnonzero(keep).astype(np.int64)
    return ia, idx_ab[ia], d2_first[ia]


def match_features(features_a, features_b, mutual=True, ratio=None, device=None):
    """Exact nearest-neighbour matching of descriptors: for every row of ``features_a`` (NA, D) its nearest row of
    ``features_b`` (NB, D) by the float32 squared distance, ties to the smaller index (1 <= D <= 64).

    -> ``(ia, ib, dist)``: int64 row indices of the matches kept, ascending ``ia``, and their float32 distances.  ``mutual``
    keeps the pairs that are each other's nearest neighbour (a second search, B against A); ``ratio`` keeps a row only if its
    nearest distance is at most ``ratio`` times its second nearest."""
    fa, fb = np.asarray(features_a), np.asarray(features_b)
    if fa.ndim != 2 or fb.ndim != 2 or fa.shape[1] != fb.shape[1]:
        raise ValueError("features must have shapes (NA, D) and (NB, D)")
    if not 1 <= fa.shape[1] <= 64:
        raise ValueError("features must have 1 to 64 columns")
    if ratio is not None and not (np.isfinite(float(ratio)) and float(ratio) >= 0):
        raise ValueError("ratio must be finite and >= 0")
    if len(fa) == 0 or len(fb) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    ctx = _capi.get_context(device)
    idx_ab, d1, d2 = _capi.feature_match(ctx, fa, fb)
    idx_ba = _capi.feature_match(ctx, fb, fa)[0] if mutual else None
    ia, ib, d2_kept = select_matches(idx_ab, d1, d2, idx_ba, mutual=mutual, ratio=ratio)
    return ia, ib, np.sqrt(d2_kept)
