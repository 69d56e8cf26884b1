"""The yardstick of the radius and hybrid neighbourhoods (tests/test_ball_cases.py, tests/test_gpu_ball.py): a NumPy float64
restatement of the section of include/pcr.h -- sets, order, anchor, float64 sums, covariance, normal and the mode / eps finish
-- and the case clouds.

Membership is ``radius_cases``' rule: the CPU oracle's brute force over the whole cloud, rows ordered by (squared distance,
index), cut at ``d <= np.float32(r)``; the point itself and its duplicates are members, a point with a non-finite coordinate has
the empty set and is nobody's member.  The hybrid set is the first ``max_nn`` entries of that segment, summed in that order
with its first entry as the anchor.  The radius set is summed in ascending original index with the smallest as the anchor (the
library anchors at and sums by its own cell-sorted order: any set-determined choice gives the same exact ties, and otherwise
differs by the order of the terms).  The sums are formed once per distinct set and shared by the points that have it.
Normal: ``numpy.linalg.eigh``'s first eigenvector, zero when count < 3.

``bound``: how far an implementation that follows the same rules in another set-determined order, about another member a' as
the anchor, may land from these figures -- count * 2^-53 * sum|term| (the bound of tests/fgr_cases.py for its sums), the terms
taken at their largest over the choice of a': d' = d - d_a', so |d'_x| <= |d_x| + M_x with M_x = max|d_x| over the set.
  mean_x    terms |a_x| (the anchor is added back) and |d_x| + M_x per member
  cov_xy    terms (|d_x| + M_x)(|d_y| + M_y) per member, and count times (2 M_x)(2 M_y) for the product of the means

A point is FRAGILE when count >= 3 and l1 - l0 < 1e-6 * l2 (eigenvalues ascending): its smallest eigenvector is not determined
to the accuracy the normal test asks.  A cap, not a tolerance: at most 1 % of every case may be fragile (``assert_cap``).
"""

import numpy as np

from radius_cases import cut_rows

FRAGILE = 1e-6
CAP = 0.01
MAX_NN = (0, 1, 3, 16, 17, 64)           # 16 and 17 straddle the switch from the register list to the LDS list
COV_PLANE, COV_RAW = 0, 1
U = 2.0 ** -53


# ---- the case clouds ---------------------------------------------------------------------------------------------------------
def jittered_grid():
    """The jittered 8 x 8 x 8 lattice of pass_cases (points 4 m apart, each moved by k / 64 per axis)."""
    from pass_cases import point_lattice
    return point_lattice()["target32"]


def two_planes():
    """Two noisy planes (sigma = 0.01) meeting at the edge x = z = 0: 600 points on z = 0, 600 on x = 0."""
    rng = np.random.default_rng(4101)
    a = np.stack([rng.uniform(0, 3, 600), rng.uniform(-2, 2, 600), rng.normal(0, 0.01, 600)], axis=1)
    b = np.stack([rng.normal(0, 0.01, 600), rng.uniform(-2, 2, 600), rng.uniform(0, 3, 600)], axis=1)
    return np.concatenate([a, b]).astype(np.float32)


def sphere_shell():
    """901 points on a sphere of radius 2 about (5, -3, 1), radial noise 0.005: a count that is no multiple of 64."""
    rng = np.random.default_rng(4102)
    v = rng.normal(size=(901, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return (np.array([5.0, -3.0, 1.0]) + v * (2.0 + rng.normal(0, 0.005, 901))[:, None]).astype(np.float32)


def lidar():
    """lidar_sweep(2000) with a range noise of 0.08 m.  At the generator's default 0.02 m the THREE nearest points of 1.9 % of
    the ground returns -- neighbours on the return's own ring line, the very sets this unit exists to avoid -- are collinear to
    1e-3 of their extent and fragile by definition (max_nn = 3; 0 % at every other max_nn); at 0.08 m 0.25 % are."""
    from point_cloud_registration_amd.synthetic import lidar_sweep
    return lidar_sweep(2000, seed=0, noise=0.08)


PAIRS = 1


def duplicates_and_faces():
    """500 uniform points in a 4 m cube, PAIRS of them given twice (an exact pair, not a triple: a set of three coincident points
    has a zero covariance and no normal; and one pair only: the three nearest of the pair's points AND of their neighbours
    hold the pair and one more, a collinear set, fragile by definition -- three points of the cloud), and 120 points with one
    or more coordinates on multiples of 0.5 and 1.0 -- cell faces of any grid whose cell is such a fraction."""
    rng = np.random.default_rng(4103)
    base = rng.uniform(0, 4, (500, 3))
    faces = rng.uniform(0, 4, (120, 3))
    on = rng.integers(0, 3, 120)
    faces[np.arange(120), on] = rng.integers(0, 9, 120) * 0.5
    faces[np.arange(40), (on[:40] + 1) % 3] = rng.integers(0, 5, 40) * 1.0
    pts = np.concatenate([base, base[:PAIRS], faces]).astype(np.float32)
    return pts[rng.permutation(len(pts))]


def with_nan():
    """The sphere shell's first 200 points, point 17 with a NaN coordinate."""
    pts = sphere_shell()[:200].copy()
    pts[17, 1] = np.nan
    return pts


def single():
    return np.array([[1.5, -2.0, 0.25]], np.float32)


def empty():
    return np.zeros((0, 3), np.float32)


# name -> (cloud, radii): 0, below the smallest spacing (count 1, or 2 at an exact pair), a typical one (10-60 members),
# one that holds the whole cloud
CASES = {
    "grid": (jittered_grid, (0.0, 0.5, 6.5, 80.0)),
    "planes": (two_planes, (0.0, 1e-4, 0.35, 12.0)),
    "sphere": (sphere_shell, (0.0, 1e-4, 0.5, 9.0)),
    "lidar": (lidar, (0.0, 1e-4, 4.0, 400.0)),
    "duplicates": (duplicates_and_faces, (0.0, 1e-4, 1.0, 16.0)),
    "nan": (with_nan, (0.0, 0.5)),
    "single": (single, (0.0, 1.0)),
    "empty": (empty, (0.0, 1.0)),
}

_clouds = {}


def cloud(name):
    if name not in _clouds:
        pts = np.ascontiguousarray(CASES[name][0](), np.float32)
        pts.setflags(write=False)
        _clouds[name] = pts
    return _clouds[name]


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _six(a, b=None):
    """(m, 3) -> (m, 6): the products xx xy xz yy yz zz of a with b (default: itself)."""
    b = a if b is None else b
    return np.stack([a[:, 0] * b[:, 0], a[:, 0] * b[:, 1], a[:, 0] * b[:, 2], a[:, 1] * b[:, 1], a[:, 1] * b[:, 2], a[:, 2] * b[:, 2]], axis=1)


def full3(c6):
    c6 = np.asarray(c6, np.float64)
    return c6[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(c6.shape[:-1] + (3, 3))


_brute = {}


def segments(orc, points, r, key=None):
    """-> list of n int64 arrays: the radius search's segment of every point against its own cloud, in its order.  ``key``:
    a name under which the brute-force rows of this cloud are kept for the next radius."""
    pts = np.ascontiguousarray(points, np.float32)
    n = len(pts)
    fin = np.isfinite(pts).all(axis=1) if n else np.zeros(0, bool)
    sub = np.flatnonzero(fin)
    segs = [np.zeros(0, np.int64)] * n
    if len(sub) == 0:
        return segs
    if key is None or key not in _brute:
        d, i = orc.knn_brute(pts[sub], pts[sub], len(sub))
        if key is not None:
            _brute[key] = (d, i)
    else:
        d, i = _brute[key]
    _, idx, off = cut_rows(d, i, np.float32(r))
    for s, p in enumerate(sub):
        segs[p] = sub[idx[off[s]:off[s + 1]]].astype(np.int64)
    return segs


def ball_ref(orc, points, r, max_nn=0, key=None):
    """-> dict: count (n,) int64; mean (n, 3), cov (n, 6), lam (n, 3) ascending, normal (n, 3) float64; set_id (n,) int64 (equal
    iff the sets -- for max_nn > 0 the lists -- are equal); fragile (n,) bool; bound_mean (n, 3), bound_cov (n, 6)."""
    pts = np.ascontiguousarray(points, np.float32)
    n = len(pts)
    P = pts.astype(np.float64)
    segs = segments(orc, pts, r, key)
    lists = [s[:max_nn] if max_nn else np.sort(s) for s in segs]
    ids, set_id, first = {}, np.zeros(n, np.int64), []
    for p, l in enumerate(lists):
        k = l.tobytes()
        if k not in ids:
            ids[k] = len(first)
            first.append(p)
        set_id[p] = ids[k]
    u = len(first)
    cnt_u = np.array([len(lists[p]) for p in first], np.int64)
    members = np.concatenate([lists[p] for p in first]) if u else np.zeros(0, np.int64)
    owner = np.repeat(np.arange(u), cnt_u)
    has = cnt_u > 0
    anchor = np.zeros((u, 3))
    anchor[has] = P[[lists[p][0] for p, h in zip(first, has) if h]]
    d = P[members] - anchor[owner]
    s1, s2 = np.zeros((u, 3)), np.zeros((u, 6))
    np.add.at(s1, owner, d)                          # (sequential, in the order of the pairs)
    np.add.at(s2, owner, _six(d))
    kd = np.maximum(cnt_u, 1).astype(np.float64)[:, None]
    m = s1 / kd
    c = s2 / kd - _six(m)
    mean = np.where(has[:, None], anchor + m, 0.0)
    # the bound (module docstring)
    ad = np.abs(d)
    M = np.zeros((u, 3))
    np.maximum.at(M, owner, ad)
    t1, t2 = np.zeros((u, 3)), np.zeros((u, 6))
    np.add.at(t1, owner, ad + M[owner])
    np.add.at(t2, owner, _six(ad + M[owner]))
    cu = cnt_u.astype(np.float64)[:, None]
    bound_mean = cu * U * (np.abs(anchor) + t1)
    bound_cov = cu * U * (t2 + cu * _six(2.0 * M))
    lam, vec = np.linalg.eigh(full3(c)) if u else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    normal = np.where((cnt_u >= 3)[:, None], vec[:, :, 0], 0.0)
    fragile = (cnt_u >= 3) & (lam[:, 1] - lam[:, 0] < FRAGILE * lam[:, 2])
    out = {"count": cnt_u, "mean": mean, "cov": c, "lam": lam, "normal": normal, "fragile": fragile, "bound_mean": bound_mean,
           "bound_cov": bound_cov}
    out = {k: (v[set_id] if n else v[:0]) for k, v in out.items()}
    out["set_id"] = set_id
    out["lists"] = lists
    return out


def cov_finish(ref, mode, eps):
    """The mode / eps finish of the restated raw covariance -> (cov (n, 6) float64, ok (n,) bool).  PCR_COV_PLANE puts
    I - (1 - eps) n n^T in its place, n the smallest eigenvector: (1, 0, 0) for the zero covariance of a set of one member (the
    identity the library's Jacobi starts from: the k-NN estimate's k = 1).  ``ok`` is False where that eigenvector is not
    determined: the fragile points, and the sets of two distinct points (a covariance of rank 1)."""
    n = len(ref["count"])
    if mode == COV_RAW:
        return ref["cov"].copy(), np.ones(n, bool)
    zero = ~np.any(ref["cov"] != 0.0, axis=1) if n else np.zeros(0, bool)
    vec = np.linalg.eigh(full3(ref["cov"]))[1][:, :, 0] if n else np.zeros((0, 3))
    vec[zero] = [1.0, 0.0, 0.0]
    I6 = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0])
    ok = zero | ((ref["count"] >= 3) & ~ref["fragile"])
    return I6 - (1.0 - eps) * _six(vec), ok


def angle_bound(ref):
    """How far the smallest eigenvector of a covariance within ``bound_cov`` of the restated one may turn (radians, Davis-Kahan:
    sin(theta) <= 2 |E| / gap), per point; inf where there is no gap."""
    e = np.sqrt(np.sum(ref["bound_cov"] ** 2 * np.array([1, 2, 2, 1, 2, 1]), axis=1)) if len(ref["count"]) else np.zeros(0)
    gap = ref["lam"][:, 1] - ref["lam"][:, 0] if len(ref["count"]) else np.zeros(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(gap > 0, 2.0 * e / gap, np.inf)


def assert_cap(ref, name):
    share = float(np.mean(ref["fragile"])) if len(ref["fragile"]) else 0.0
    assert share <= CAP, f"{name}: {share:.4f} of the points are fragile, the cap is {CAP}"
    return share


_refs = {}


def case_ref(orc, name, r, max_nn):
    """ball_ref of a case cloud, computed once and shared (one brute force per cloud)."""
    k = (name, float(r), int(max_nn))
    if k not in _refs:
        _refs[k] = ball_ref(orc, cloud(name), r, max_nn, key=name)
    return _refs[k]


def all_cases():
    return [(name, r, m) for name, (_, radii) in CASES.items() for r in radii for m in MAX_NN]
