"""The yardsticks of the radius search and the outlier filters (tests/test_radius_api.py, tests/test_gpu_radius.py).

float32: the CPU oracle's brute force over the WHOLE target, ``orc.knn_brute(pts, q, len(pts))`` -- rows ordered by (squared
distance, index) -- cut at ``d <= np.float32(r)``: the members of a segment are a prefix of their row.
float64: NumPy, d2 = (dx*dx + dy*dy) + dz*dz, members ``sqrt(d2) <= r``, ordered with ``np.lexsort((idx, d2))``.
Mean k-NN distance: the float32 distances of ``orc.knn_brute(pts, pts, k)`` summed in float64 column by column (an explicit
loop: ``np.sum`` adds pairwise, in another order) over the neighbours found.
"""

import numpy as np

from test_gpu_parity import constructed_cloud

# case -> radii of the constructed-cloud test
RADII = {"lattice": [0.25, 0.5, 1.0, 10.0], "dense_spot": [0.001, 0.01], "duplicates": [0.0, 0.3], "sheet": [0.25, 0.4],
         "two_scales": [0.1, 0.2]}

_rows = {}


def brute_rows(orc, case):
    """(pts, q, d, i): every query's distances to ALL points of the case's cloud, nearest first; computed once per case."""
    if case not in _rows:
        pts, q = constructed_cloud(case)
        d, i = orc.knn_brute(pts, q, len(pts))
        for a in (pts, q, d, i):
            a.setflags(write=False)
        _rows[case] = (pts, q, d, i)
    return _rows[case]


def cut_rows(d, i, r):
    """Full brute-force rows -> (dist, idx, offsets) of the radius search at r (float32)."""
    keep = d <= np.float32(r)
    offsets = np.zeros(len(d) + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=offsets[1:])
    return d[keep], i[keep], offsets


def radius_ref_f32(orc, pts, q, r):
    pts, q = np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(q, np.float32)
    if len(q) == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(1, np.int64)
    d, i = orc.knn_brute(pts, q, len(pts))
    return cut_rows(d, i, r)


def radius_ref_f64(pts, q, r):
    """NumPy brute force in float64 (queries widened exactly)."""
    pts, q = np.asarray(pts, np.float64), np.asarray(q, np.float64)
    dist, idx, offsets = [], [], [0]
    n = np.arange(len(pts))
    for qi in q:
        dx, dy, dz = qi[0] - pts[:, 0], qi[1] - pts[:, 1], qi[2] - pts[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        with np.errstate(invalid="ignore"):
            d = np.sqrt(d2)
            keep = np.flatnonzero(d <= np.float64(r))
        keep = keep[np.lexsort((n[keep], d2[keep]))]
        dist.append(d[keep]); idx.append(keep.astype(np.int64)); offsets.append(offsets[-1] + len(keep))
    return (np.concatenate(dist) if dist else np.zeros(0)), (np.concatenate(idx) if idx else np.zeros(0, np.int64)), \
        np.asarray(offsets, np.int64)


def sequential_mean(d):
    """(N, k) float32 k-NN distances, +inf where the cloud ran out -> the float64 mean over the neighbours found, summed
    nearest first."""
    s = np.zeros(len(d), np.float64)
    c = np.zeros(len(d), np.float64)
    for col in range(d.shape[1]):
        found = np.isfinite(d[:, col])
        s = np.where(found, s + d[:, col].astype(np.float64), s)
        c += found
    return s / np.maximum(c, 1.0)


def mean_distance_ref(orc, pts, k):
    pts = np.ascontiguousarray(pts, np.float32)
    return sequential_mean(orc.knn_brute(pts, pts, k)[0])


def bounded_knn_ref(d64, i64, k, r, n):
    """The first k columns of a 64-column brute force with entries ``not (d < r)`` set to (inf, n)."""
    d, i = d64[:, :k].copy(), i64[:, :k].copy()
    out = ~(d < r)
    d[out] = np.inf
    i[out] = n
    return d, i


def planted_sheet():
    """The sheet of constructed_cloud plus 20 points planted at z = +-3: far from everything at radius 0.4."""
    pts, _ = constructed_cloud("sheet")
    rng = np.random.default_rng(71)
    planted = np.hstack([rng.uniform(-4, 4, (20, 2)), np.where(np.arange(20) % 2 == 0, 3.0, -3.0)[:, None]]).astype(np.float32)
    cloud = np.vstack([pts, planted])
    return cloud, np.arange(len(pts), len(cloud))


def shifted_two_scales():
    """two_scales moved by 500 in float64, with a jitter below float32's resolution there (2^-15 m): a float32 copy cannot
    tell the points from their unjittered places, a float64 tree must.  -> (pts64, q64, q32)"""
    pts, q = constructed_cloud("two_scales")
    rng = np.random.default_rng(72)
    pts64 = pts.astype(np.float64) + 500.0 + rng.uniform(-1e-6, 1e-6, pts.shape)
    q64 = q.astype(np.float64) + 500.0 + rng.uniform(-1e-6, 1e-6, q.shape)
    q32 = (q.astype(np.float64) + 500.0).astype(np.float32)
    return pts64, q64, q32
