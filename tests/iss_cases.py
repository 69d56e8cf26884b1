"""The yardstick of the ISS keypoints (tests/test_iss_api.py, tests/test_gpu_iss.py): a NumPy float64 restatement of the
definitions in include/pcr.h -- support sets, scatter matrices about a set-determined anchor, eigenvalues, saliency and the
non-maximum suppression with its index rule.

Membership comes from ``radius_cases.radius_ref_f32`` (the oracle's brute force cut at d <= r), the point itself and its
duplicates included.  The anchor of a support set is its member with the smallest original index and the members are summed
in ascending original index (the library anchors at and sums by its own cell-sorted order: any set-determined choice gives
the same EXACT ties, and otherwise differs by the order of a few hundred float64 terms).  The sums are formed once per
distinct support set and shared by the points that have it, so equal sets give equal bits here as well.  Eigenvalues:
``np.linalg.eigvalsh``.

A point is FRAGILE-SALIENT when it has k >= min_neighbors and one of |l2 - g21 l1|, |l3 - g32 l2|, |l3| is <= EPS l1: a
rounding could flip its flag.  A point is EXCLUDED when it is fragile-salient, or someone in its non-maximum ball is, or it
is salient and someone else in that ball with a DIFFERENT support set has a saliency within EPS s_i of its own.  Equal
saliency from identical support sets is a tie, settled by the index rule, not fragility.  A cap, not a tolerance: at most
1 % of a test cloud may be excluded (``assert_cap``).
"""

import numpy as np

import fpfh_cases as fc
from radius_cases import cut_rows, radius_ref_f32

EPS = 1e-9
CAP = fc.CAP
GAMMA = 0.975
MIN_NEIGHBORS = 5

# named cloud of fpfh_cases -> the (salient radius, non-maximum radius) pairs the tests use
PARAMS = {"main": [(0.668, 0.445), (0.668, 0.668)], "second": [(0.47, 0.313), (0.47, 0.47)]}
# keypoints the restatement finds there (test_iss_api.test_expected_counts keeps these honest on the CPU)
EXPECTED = {("main", 0): 126, ("main", 1): 48, ("second", 0): 274, ("second", 1): 123}


def _segments(orc, pts, r, brute=None):
    """-> (I, J, count): every ordered pair (i, j) with j in N_r(i), j ascending within i.  ``brute``: the full rows
    ``orc.knn_brute(pts, pts, len(pts))`` that radius_ref_f32 cuts, when the caller already has them."""
    n = len(pts)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    _, J, off = radius_ref_f32(orc, pts, pts, np.float32(r)) if brute is None else cut_rows(brute[0], brute[1], np.float32(r))
    I = np.repeat(np.arange(n), np.diff(off))
    order = np.lexsort((J, I))
    return I[order], J[order].astype(np.int64), np.diff(off).astype(np.int64)


def iss_ref(orc, points, r_salient, r_nonmax, gamma_21=GAMMA, gamma_32=GAMMA, min_neighbors=MIN_NEIGHBORS, brute=None):
    """-> dict: k (n,) int64, eig (n, 3) float64 descending, salient (n,) bool, saliency (n,) float64, set_id (n,) int64 (equal
    iff the support sets are equal), count_nm (n,) int64, keypoint (n,) bool, fragile (n,) bool, excluded (n,) bool, tie (n,)
    bool (salient, and someone else in the non-maximum ball has exactly the same saliency)."""
    pts = np.ascontiguousarray(points, np.float32)
    n = len(pts)
    P = pts.astype(np.float64)
    I, J, k = _segments(orc, pts, r_salient, brute)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(k, out=off[1:])
    # distinct support sets
    ids, set_id, first = {}, np.zeros(n, np.int64), []
    for i in range(n):
        key = J[off[i]:off[i + 1]].tobytes()
        if key not in ids:
            ids[key] = len(first)
            first.append(i)
        set_id[i] = ids[key]
    first = np.asarray(first, np.int64)
    u = len(first)
    # the sums of every distinct set, members in ascending original index, sequentially (np.add.at adds in pair order)
    sel = np.concatenate([np.arange(off[i], off[i + 1]) for i in first]) if u else np.zeros(0, np.int64)
    U = np.repeat(np.arange(u), k[first]) if u else np.zeros(0, np.int64)
    members = J[sel]
    anchor = P[J[off[first]]] if u else np.zeros((0, 3))                 # (the smallest original index of the set)
    d = P[members] - anchor[U]
    s1, s2 = np.zeros((u, 3)), np.zeros((u, 6))
    np.add.at(s1, U, d)
    np.add.at(s2, U, np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                               d[:, 2] * d[:, 2]], axis=1))
    ku = k[first].astype(np.float64)[:, None]
    m = s1 / ku
    c = s2 / ku - np.stack([m[:, 0] * m[:, 0], m[:, 0] * m[:, 1], m[:, 0] * m[:, 2], m[:, 1] * m[:, 1], m[:, 1] * m[:, 2],
                            m[:, 2] * m[:, 2]], axis=1)
    C = np.empty((u, 3, 3))
    C[:, 0, 0], C[:, 0, 1], C[:, 0, 2] = c[:, 0], c[:, 1], c[:, 2]
    C[:, 1, 0], C[:, 1, 1], C[:, 1, 2] = c[:, 1], c[:, 3], c[:, 4]
    C[:, 2, 0], C[:, 2, 1], C[:, 2, 2] = c[:, 2], c[:, 4], c[:, 5]
    eig_u = np.linalg.eigvalsh(C)[:, ::-1] if u else np.zeros((0, 3))
    eig = eig_u[set_id] if n else np.zeros((0, 3))
    l1, l2, l3 = (eig[:, 0], eig[:, 1], eig[:, 2]) if n else (np.zeros(0),) * 3
    enough = k >= min_neighbors
    salient = enough & (l1 > 0) & (l2 < gamma_21 * l1) & (l3 < gamma_32 * l2) & (l3 > 0)
    saliency = np.where(salient, l3, 0.0)
    tol = EPS * l1
    fragile = enough & ((np.abs(l2 - gamma_21 * l1) <= tol) | (np.abs(l3 - gamma_32 * l2) <= tol) | (np.abs(l3) <= tol))
    # the non-maximum suppression
    I2, J2, count_nm = _segments(orc, pts, r_nonmax, brute)
    other = I2 != J2
    Io, Jo = I2[other], J2[other]
    si, sj = saliency[Io], saliency[Jo]
    loses = (sj < si) | ((sj == si) & (Jo > Io))
    beaten = np.zeros(n, bool)
    beaten[Io[~loses]] = True
    keypoint = (saliency > 0) & (count_nm >= min_neighbors) & ~beaten
    excluded = fragile.copy()
    excluded[I2[fragile[J2]]] = True
    close = (si > 0) & (set_id[Io] != set_id[Jo]) & (np.abs(sj - si) <= EPS * si)
    excluded[Io[close]] = True
    tie = np.zeros(n, bool)
    tie[Io[(si > 0) & (sj == si)]] = True
    return {"k": k, "eig": eig, "salient": salient, "saliency": saliency, "set_id": set_id, "count_nm": count_nm, "keypoint": keypoint,
            "fragile": fragile, "excluded": excluded, "tie": tie}


def assert_cap(ref, name):
    share = float(np.mean(ref["excluded"])) if len(ref["excluded"]) else 0.0
    assert share <= CAP, f"{name}: {share:.4f} of the points are excluded as fragile, the cap is {CAP}"
    return share


_refs = {}


def cloud_ref(orc, name, which):
    """iss_ref of a named cloud of fpfh_cases at PARAMS[name][which], computed once (every pair of the cloud from one brute
    force) and shared."""
    if (name, which) not in _refs:
        pts = fc.cloud(name)[0]
        brute = orc.knn_brute(pts, pts, len(pts))
        for w, (rs, rn) in enumerate(PARAMS["main" if name == "main_moved" else name]):
            _refs[(name, w)] = iss_ref(orc, pts, rs, rn, brute=brute)
    return _refs[(name, which)]


def cluster(n, seed=21):
    """The points of test_gpu_fpfh.cluster: n uniform points in a unit cube."""
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
