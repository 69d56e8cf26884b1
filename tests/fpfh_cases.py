"""The yardsticks of the FPFH descriptors and the feature matching (tests/test_fpfh_api.py, tests/test_gpu_fpfh.py): a NumPy
float64 restatement of the definitions in include/pcr.h -- pair features, SPFH counts, FPFH, the float32 sequential squared
distance and the top-2 by key.  NumPy neither fuses nor reorders: every expression below rounds as it is written.

Membership comes from ``radius_cases.radius_ref_f32`` (the oracle's brute force cut at d <= r), minus the pairs at d2 == 0.

Everything in a pair feature is +, -, *, /, sqrt (correctly rounded everywhere) except ``atan2``, which may differ by an ulp
between libraries.  A pair is FRAGILE when that -- or a reading of the role rule at a tie -- could move it to another bin:
  * a bin coordinate within 1e-9 of an interior bin edge 1 .. 10, or theta's within 1e-9 of 0 or 11 (the wrap);
  * ||a1| - |a2|| <= 1e-9 L and the two role assignments give different bins.
A point is EXCLUDED when any of its own pairs, or any pair of any of its neighbours, is fragile.  A cap, not a tolerance: at
most 1 % of a test cloud may be excluded (``assert_cap``).
"""

import numpy as np

from radius_cases import radius_ref_f32

EDGE_EPS = 1e-9
CAP = 0.01


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _coords(n1, n2, d, L):
    """Bin coordinates (m, 3) = alpha, phi, theta of pairs whose roles are settled, and |v|."""
    phi = _dot(n1, d) / L
    v = _cross(d, n1)
    vv = _dot(v, v)
    ok = vv != 0
    vn = np.sqrt(np.where(ok, vv, 1.0))
    v = v / vn[:, None]
    w = _cross(n1, v)
    alpha = np.where(ok, _dot(v, n2), 0.0)
    theta = np.where(ok, np.arctan2(_dot(w, n2), _dot(n1, n2)), 0.0)
    c = np.stack([11.0 * (alpha + 1.0) / 2.0, 11.0 * (phi + 1.0) / 2.0, 11.0 * (theta + np.pi) / (2.0 * np.pi)], axis=1)
    return c, np.sqrt(vv)


def _bins(c):
    with np.errstate(invalid="ignore"):
        return np.clip(np.floor(c), 0, 10).astype(np.int64)


def pair_features(points, normals, I, J):
    """Pairs (p = points[I], q = points[J]) with d2 > 0 -> dict: bins (m, 3) int64 in 0 .. 10, d2 (m,), fragile (m,) bool,
    edge (m,) distance of the closest bin edge, tie (m,) ||a1| - |a2|| / L, vnorm (m,) |d x n1|."""
    P, N = np.asarray(points, np.float32).astype(np.float64), np.asarray(normals, np.float32).astype(np.float64)
    p, q, n_p, n_q = P[I], P[J], N[I], N[J]
    d = q - p
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert np.all(d2 > 0)
    L = np.sqrt(d2)
    a1, a2 = _dot(n_p, d), _dot(n_q, d)
    swap = np.abs(a1) < np.abs(a2)
    s = swap[:, None]
    c, vnorm = _coords(np.where(s, n_q, n_p), np.where(s, n_p, n_q), np.where(s, -d, d), L)
    c_other, _ = _coords(np.where(s, n_p, n_q), np.where(s, n_q, n_p), np.where(s, d, -d), L)
    bins = _bins(c)
    # the closest edge that matters: interior edges 1 .. 10 for all three, 0 and 11 as well for theta
    near = np.abs(c - np.clip(np.round(c), 1, 10))
    near[:, 2] = np.minimum(near[:, 2], np.minimum(np.abs(c[:, 2]), np.abs(c[:, 2] - 11.0)))
    edge = near.min(axis=1)
    tie = np.abs(np.abs(a1) - np.abs(a2)) / L
    fragile = (edge <= EDGE_EPS) | ((tie <= EDGE_EPS) & np.any(bins != _bins(c_other), axis=1))
    return {"bins": bins, "d2": d2, "fragile": fragile, "edge": edge, "tie": tie, "vnorm": vnorm}


def neighbourhoods(orc, points, r):
    """(I, J): every ordered pair (i, j) with j in the neighbourhood of i -- the radius search at r minus d2 == 0."""
    points = np.ascontiguousarray(points, np.float32)
    if len(points) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    _, J, off = radius_ref_f32(orc, points, points, r)
    I = np.repeat(np.arange(len(points)), np.diff(off))
    P = points.astype(np.float64)
    d = P[J] - P[I]
    keep = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) != 0
    return I[keep], J[keep]


def fpfh_ref(orc, points, normals, r):
    """-> dict: counts (n, 33) uint32, k (n,) int64, fpfh (n, 33) float64 (before the rounding to float32), excluded (n,) bool,
    pairs = the pair_features dict, I, J."""
    n = len(points)
    I, J = neighbourhoods(orc, points, r)
    pf = pair_features(points, normals, I, J) if len(I) else \
        {"bins": np.zeros((0, 3), np.int64), "d2": np.zeros(0), "fragile": np.zeros(0, bool), "edge": np.zeros(0), "tie": np.zeros(0),
         "vnorm": np.zeros(0)}
    counts = np.zeros((n, 33), np.int64)
    for f in range(3):
        np.add.at(counts, (I, 11 * f + pf["bins"][:, f]), 1)
    k = np.bincount(I, minlength=n).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        S = np.where(k[:, None] > 0, 100.0 * counts / k[:, None], 0.0)
    A = np.zeros((n, 33))
    np.add.at(A, I, S[J] / pf["d2"][:, None])                           # (sequential, in pair order)
    F = S.copy()
    for f in range(3):
        blk = slice(11 * f, 11 * f + 11)
        tot = np.zeros(n)
        for b in range(11 * f, 11 * f + 11):
            tot = tot + A[:, b]
        with np.errstate(invalid="ignore", divide="ignore"):
            F[:, blk] += np.where(tot[:, None] > 0, 100.0 * A[:, blk] / tot[:, None], 0.0)
    own = np.zeros(n, bool)
    own[I[pf["fragile"]]] = True
    excluded = own.copy()
    excluded[I[own[J]]] = True
    return {"counts": counts.astype(np.uint32), "k": k, "fpfh": F, "excluded": excluded, "pairs": pf, "I": I, "J": J}


def assert_cap(ref, name):
    share = float(np.mean(ref["excluded"])) if len(ref["excluded"]) else 0.0
    assert share <= CAP, f"{name}: {share:.4f} of the points are excluded as fragile, the cap is {CAP}"
    return share


# ---- feature matching -----------------------------------------------------------------------------------------------------
def d2_f32(A, B):
    """(na, nb) float32: the sum over the columns, in order, of (A[i, c] - B[j, c])^2, every step rounded to float32."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    d2 = np.zeros((len(A), len(B)), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(A.shape[1]):
            t = A[:, None, c] - B[None, :, c]
            d2 = d2 + t * t
    return d2


def match_ref(A, B):
    """-> (idx int64, d2_first float32, d2_second float32): the two smallest keys (d2, j) of every row; a NaN distance never
    wins; nothing left: idx = -1 / distance inf."""
    d2 = d2_f32(A, B)
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(d2.shape[1], dtype=np.uint64)[None, :]
    key = np.where(np.isnan(d2), none, key)
    key = np.sort(np.concatenate([key, np.full((len(key), 2), none)], axis=1), axis=1)[:, :2]
    dist = np.where(key == none, np.float32(np.inf), (key >> np.uint64(32)).astype(np.uint32).view(np.float32))
    idx = np.where(key[:, 0] == none, -1, (key[:, 0] & np.uint64(0xFFFFFFFF)).astype(np.int64))
    return idx.astype(np.int64), dist[:, 0].astype(np.float32), dist[:, 1].astype(np.float32)


# ---- the named clouds -----------------------------------------------------------------------------------------------------
MAIN_R = 0.668
SECOND_R = 0.47
_cache = {}


def _unit32(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def rigid(points, normals, yaw=2.0, roll=0.4, t=(3.0, -2.0, 0.5)):
    """The cloud under a yaw about z, then a roll about x, and a translation: transformed in float64, rounded to float32."""
    cz, sz, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(roll), np.sin(roll)
    R = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    moved = (np.asarray(points, np.float64) @ R.T + np.asarray(t, np.float64)).astype(np.float32)
    return moved, (np.asarray(normals, np.float64) @ R.T).astype(np.float32)


def cloud(name):
    """name -> (points float32 (n, 3), normals float32 (n, 3), r); built once, read-only.
    main        street(2048, seed=3) * 0.1, random unit normals of default_rng(3), r = 0.668
    main_moved  the same under ``rigid``
    second      street(4096, seed=3) * 0.1, its analytic normals + N(0, 0.02) noise of default_rng(5), renormalised; r = 0.47
                gives a mean of about 20 neighbours"""
    from point_cloud_registration_amd.synthetic import street, street_normals
    if name not in _cache:
        if name == "main":
            pts = (street(2048, seed=3) * 0.1).astype(np.float32)
            out = pts, _unit32(np.random.default_rng(3).normal(size=(2048, 3))), MAIN_R
        elif name == "main_moved":
            p, nrm, r = cloud("main")
            out = rigid(p, nrm) + (r,)
        elif name == "second":
            full = street(4096, seed=3)
            nrm = street_normals(full).astype(np.float64) + np.random.default_rng(5).normal(0.0, 0.02, (4096, 3))
            out = (full * 0.1).astype(np.float32), _unit32(nrm), SECOND_R
        else:
            raise KeyError(name)
        for a in out[:2]:
            a.setflags(write=False)
        _cache[name] = out
    return _cache[name]


CLOUDS = ("main", "main_moved", "second")
_refs = {}


def cloud_ref(orc, name):
    """fpfh_ref of a named cloud, computed once and shared."""
    if name not in _refs:
        p, nrm, r = cloud(name)
        _refs[name] = fpfh_ref(orc, p, nrm, r)
    return _refs[name]
