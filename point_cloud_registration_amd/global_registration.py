"""Global registration on the MI355X: from feature matches to a pose (what Open3D's
``registration_ransac_based_on_feature_matching`` does after the matching), kernels in ``csrc/ransac.hip``, definitions in
``include/pcr.h``.  The reference has no counterpart.

``ransac_pose`` draws pose hypotheses from triples of matches, scores every one of them against every match on the GPU and
refines the winner over its inliers; ``fgr_pose`` (fast global registration, ``csrc/fgr.hip``) runs a graduated robust
Gauss-Newton loop over the matches instead; ``sc2_pose`` (``csrc/compat.hip``) fits consensus sets of the matches'
compatibility graph, for match lists of which a few per cent are right; ``register_global`` chains ``compute_fpfh``,
``match_features`` and ``ransac_pose`` -- over every point, or over keypoints (``keypoints.py``) with descriptors at those rows
only.  The result is an ``init_T`` for ``align`` of any of the local aligners.  Everything is computed over the **float32 copy** of the
points, and the same call twice returns the same bits.
"""

import numpy as np

from . import _capi
from .features import compute_fpfh, compute_fpfh_rows, match_features
from .keypoints import iss_keypoints


def _pairs(source, target, ia, ib):
    """The paired float32 rows source[ia], target[ib]."""
    source, target = _capi.cloud_f32(source, "source", finite=False), _capi.cloud_f32(target, "target", finite=False)
    ia, ib = np.asarray(ia), np.asarray(ib)
    if ia.ndim != 1 or ia.shape != ib.shape:
        raise ValueError("ia and ib must be vectors of one length")
    if len(ia) and not (np.issubdtype(ia.dtype, np.integer) and np.issubdtype(ib.dtype, np.integer)):
        raise ValueError("ia and ib must be integer row indices")
    ia, ib = ia.astype(np.int64), ib.astype(np.int64)
    if len(ia) and (ia.min() < 0 or ia.max() >= len(source) or ib.min() < 0 or ib.max() >= len(target)):
        raise ValueError("ia / ib point outside source / target")
    return _capi.check_pairs(source[ia], target[ib])


def _poses12(Ts):
    """(B, 4, 4) or (4, 4) -> (B, 12) float32: R row-major, then t."""
    Ts = np.asarray(Ts)
    single = Ts.ndim == 2
    if single:
        Ts = Ts[None]
    if Ts.ndim != 3 or Ts.shape[1:] != (4, 4):
        raise ValueError("Ts must have shape (B, 4, 4) or (4, 4)")
    with np.errstate(over="ignore", invalid="ignore"):
        P = np.concatenate([Ts[:, :3, :3].reshape(len(Ts), 9), Ts[:, :3, 3]], axis=1).astype(np.float32)
    return np.ascontiguousarray(P), single


def _T_of(pose12):
    T = np.eye(4)
    T[:3, :3] = np.asarray(pose12[:9], np.float64).reshape(3, 3)
    T[:3, 3] = pose12[9:]
    return T


def score_poses(source, target, ia, ib, Ts, max_dist, return_mask=False, device=None):
    """How many of the correspondences ``source[ia] -> target[ib]`` each pose of ``Ts`` ((B, 4, 4) or (4, 4), rounded to
    float32) brings within ``max_dist``: the float32 inlier rule of ``include/pcr.h``, a NaN pose scores 0.

    -> counts (B,) int32, or an int for a single pose; with ``return_mask`` also the masks (B, M) bool (or (M,))."""
    src, dst = _pairs(source, target, ia, ib)
    P, single = _poses12(Ts)
    res = _capi.pose_score(lambda: _capi.get_context(device), src, dst, P, max_dist, want_mask=return_mask)
    if not return_mask:
        return int(res[0]) if single else res
    return (int(res[0][0]), res[1][0]) if single else res


def fit_rigid(src, dst):
    """The least-squares rigid motion of paired points (Kabsch), float64 on the host: centroids, the 3 x 3 sum of
    (q - c_q)(p - c_p)^T, ``np.linalg.svd`` and the determinant correction -> a (4, 4) pose that maps ``src`` onto ``dst``."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    if src.ndim != 2 or src.shape[1] != 3 or src.shape != dst.shape or len(src) < 3:
        raise ValueError("src and dst must have one shape (N, 3), N >= 3")
    cp, cq = src.mean(axis=0), dst.mean(axis=0)
    H = (dst - cq).T @ (src - cp)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U @ Vt) >= 0 else -1.0])
    T = np.eye(4)
    T[:3, :3] = U @ D @ Vt
    T[:3, 3] = cq - T[:3, :3] @ cp
    return T


def _rmse(T, src, dst, mask):
    """Root mean square residual of the masked rows under T, float64."""
    if not mask.any():
        return np.inf
    p, q = src[mask].astype(np.float64), dst[mask].astype(np.float64)
    r = p @ T[:3, :3].T + T[:3, 3] - q
    return float(np.sqrt(np.mean(np.sum(r * r, axis=1))))


def _round32(T):
    with np.errstate(over="ignore"):
        return T.astype(np.float32).astype(np.float64)


def _proper(T):
    """T with its rotation block replaced by the nearest rotation (float64, by SVD); the translation stays."""
    U, _, Vt = np.linalg.svd(T[:3, :3])
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U @ Vt) >= 0 else -1.0])
    out = T.copy()
    out[:3, :3] = U @ D @ Vt
    return out


def refine_pose(score, src, dst, T, refine_rounds):
    """The refinement of ``ransac_pose`` over a scoring function ``score(T) -> (count, mask)``: -> (T, count, mask, rmse)."""
    T = _round32(T)
    count, mask = score(T)
    rmse = _rmse(T, src, dst, mask)
    for _ in range(int(refine_rounds)):
        if count < 3:
            break
        T2 = _round32(fit_rigid(src[mask], dst[mask]))
        c2, m2 = score(T2)
        r2 = _rmse(T2, src, dst, m2)
        if not (c2 > count or (c2 == count and r2 < rmse)):
            break
        T, count, mask, rmse = T2, c2, m2, r2
    return T, count, mask, rmse


def ransac_pose(source, target, ia, ib, max_dist, n_hypotheses=100_000, seed=0, edge_similarity=0.9, min_edge=0.0,
                refine_rounds=5, return_info=False, device=None):
    """A pose from the correspondences ``source[ia] -> target[ib]`` by RANSAC.

    ``n_hypotheses`` triples of correspondences are drawn by a counter-based generator (hypothesis h depends on ``seed``, h and
    the number of correspondences only); a triple whose edge lengths differ by more than the factor ``edge_similarity``
    between the two sides, or are shorter than ``min_edge``, is dropped; every other gets the rigid motion of its two
    triangles and is scored against all the correspondences at ``max_dist``.  The best -- most inliers, then the smallest h --
    is refined on the host up to ``refine_rounds`` times: Kabsch over the inliers, kept while it gains inliers or, at the same
    count, lowers their RMSE.  There is no early termination.

    -> ``T`` (4, 4) float64, identity when no hypothesis is valid; with ``return_info`` also a dict with ``inliers`` (M,)
    bool, ``count``, ``fitness`` (count / M), ``rmse``, ``hypothesis`` (-1: none valid), ``n_valid`` and ``pose`` -- the 12
    float32 values exactly as scored, to which the inliers, the count and the RMSE belong.  ``T`` is that pose with its rotation
    made orthonormal in float64 (the nearest rotation; entries move by less than 1e-7): a rotation rounded to float32 is
    orthonormal to 1e-8 only, and ``align`` composes its steps onto ``init_T`` without ever restoring that."""
    src, dst = _pairs(source, target, ia, ib)
    refine_rounds = int(refine_rounds)
    if refine_rounds < 0:
        raise ValueError("refine_rounds must be >= 0")
    box = []

    def ctx():
        if not box:
            box.append(_capi.get_context(device))
        return box[0]
    res = _capi.ransac_poses(ctx, src, dst, n_hypotheses, seed, max_dist, edge_similarity, min_edge)
    m = len(src)
    T, count, mask, rmse = np.eye(4), 0, np.zeros(m, bool), np.inf
    pose = res["pose"]
    if res["best"] >= 0:
        def score(Tc):
            c, k = _capi.pose_score(ctx, src, dst, _poses12(Tc)[0], max_dist, want_mask=True)
            return int(c[0]), k[0]
        T, count, mask, rmse = refine_pose(score, src, dst, _T_of(pose), refine_rounds)
        pose = _poses12(T)[0][0]
        T = _proper(T)
    if not return_info:
        return T
    return T, {"pose": pose, "inliers": mask, "count": int(count), "fitness": count / m if m else 0.0, "rmse": rmse, "hypothesis": int(res["best"]),
               "n_valid": int(res["n_valid"])}


def _bbox_diagonal(a):
    return float(np.linalg.norm(a.max(axis=0).astype(np.float64) - a.min(axis=0).astype(np.float64))) if len(a) else 0.0


def fgr_pose(source, target, ia, ib, max_dist, iterations=64, division_factor=1.4, period=4, mu0=None, tuple_scale=0.95, n_tuples=None,
             min_edge=0.0, seed=0, init_T=None, refine_rounds=5, return_info=False, device=None):
    """A pose from the correspondences ``source[ia] -> target[ib]`` by fast global registration (Zhou, Park, Koltun 2016;
    Open3D's ``registration_fgr_based_on_feature_matching`` after the matching): no hypotheses, ``iterations`` Gauss-Newton
    steps over the matches themselves under a Geman-McClure line process (``include/pcr.h``: ``pcr_fgr_pose``).  Its scale
    ``mu`` starts at ``mu0`` -- ``None``: D^2, D the larger bounding-box diagonal of the two matched point sets, where every
    match counts as an inlier -- and is divided by ``division_factor`` every ``period`` iterations down to ``max_dist``^2.

    ``tuple_scale``: the tuple test first.  ``n_tuples`` (``None``: 100 per match, at most 2^26) triples of matches are drawn
    by ``ransac_pose``'s generator from ``seed``; one whose edge lengths agree within the factor ``tuple_scale`` on both sides
    (and are at least ``min_edge``) adds 1 to the multiplicity of its three matches, and a match then counts that often:
    matches no valid triple contains drop out.  ``None`` skips the test.  Fewer than 3 matches left: ``ransac_pose``'s no-match
    result, the identity and count 0.  The loop starts from ``init_T`` (identity) and ends as ``ransac_pose`` does: its pose
    is scored at ``max_dist``, refined up to ``refine_rounds`` times over its inliers and returned with its rotation made
    orthonormal.  Deterministic: the same call twice returns the same bits.

    -> ``T`` (4, 4) float64; with ``return_info`` also a dict with ``pose``, ``inliers``, ``count``, ``fitness``, ``rmse`` as
    for ``ransac_pose`` and ``iterations``, ``status`` (0 ran out, 1 converged, 2 singular), ``mu`` (the last scale),
    ``weights`` (M,) float64 -- the line-process weights under the loop's own pose --, ``mult`` (M,) int32 and ``n_valid``."""
    src, dst = _pairs(source, target, ia, ib)
    m = len(src)
    refine_rounds = int(refine_rounds)
    if refine_rounds < 0:
        raise ValueError("refine_rounds must be >= 0")
    max_dist = _capi.check_distance(max_dist, "max_dist")
    if not max_dist > 0:
        raise ValueError("max_dist must be > 0")
    if mu0 is None:
        D = max(_bbox_diagonal(src), _bbox_diagonal(dst))
        mu0 = D * D if D > 0 else max_dist * max_dist
    mu0, mu_min, division, period, iterations = _capi.check_fgr(mu0, max_dist * max_dist, division_factor, period, iterations)
    T0 = np.eye(4) if init_T is None else _capi._pose16(init_T, "init_T")
    if n_tuples is None:
        n_tuples = min(100 * m, _capi.RANSAC_H_MAX)
    box = []

    def ctx():
        if not box:
            box.append(_capi.get_context(device))
        return box[0]
    if tuple_scale is None:
        mult, n_valid, live = np.ones(m, np.int32), 0, m
    else:
        mult, n_valid = _capi.fgr_tuples(ctx, src, dst, n_tuples, seed, tuple_scale, min_edge)
        live = int(np.count_nonzero(mult))
    T, count, mask, rmse = np.eye(4), 0, np.zeros(m, bool), np.inf
    pose = _poses12(T)[0][0]
    res = {"iterations": 0, "status": 0, "mu": mu0, "weights": np.ones(m)}
    if live >= 3:
        res = _capi.fgr_pose(ctx, src, dst, T0, mu0, mu_min, division, period, iterations, mult=None if tuple_scale is None else mult)

        def score(Tc):
            c, k = _capi.pose_score(ctx, src, dst, _poses12(Tc)[0], max_dist, want_mask=True)
            return int(c[0]), k[0]
        T, count, mask, rmse = refine_pose(score, src, dst, res["T"], refine_rounds)
        pose = _poses12(T)[0][0]
        T = _proper(T)
    if not return_info:
        return T
    return T, {"pose": pose, "inliers": mask, "count": int(count), "fitness": count / m if m else 0.0, "rmse": rmse,
               "iterations": res["iterations"], "status": res["status"], "mu": res["mu"], "weights": res["weights"], "mult": mult,
               "n_valid": int(n_valid)}


def _compat_pairs(source, target, ia, ib, who):
    """``_pairs`` for the compatibility calls: their own limit on the number of matches, said before anything is copied."""
    if np.ndim(ia) == 1 and len(ia) > _capi.COMPAT_M_MAX:
        raise ValueError(f"{who}: {len(ia)} matches, the compatibility matrix takes at most {_capi.COMPAT_M_MAX} (PCR_COMPAT_M_MAX); "
                         'match fewer rows: keypoints="iss", mutual=True or ratio= of register_global / match_features')
    return _pairs(source, target, ia, ib)


def match_compatibility(source, target, ia, ib, max_dist, return_bits=False, device=None):
    """The compatibility graph of the correspondences ``source[ia] -> target[ib]`` (``include/pcr.h``: ``pcr_compat_bits``,
    kernels in ``csrc/compat.hip``): matches i and j are compatible when the lengths ``|p_i - p_j|`` and ``|q_i - q_j|``
    differ by at most ``max_dist`` -- a rigid motion keeps lengths, so right matches are compatible with each other whatever
    the pose.  ``deg1[i]`` counts the matches compatible with i, ``deg2[i]`` sums, over those, the compatible matches the two
    have in common (the second-order measure of SC2-PCR).  Integers throughout: the same call twice returns the same bits.

    -> ``(deg1, deg2)`` (M,) int64; with ``return_bits`` also the matrix as (M, ceil(M / 64)) uint64, bit ``j & 63`` of word
    ``j >> 6`` of row i.  At most ``PCR_COMPAT_M_MAX`` = 32768 matches."""
    src, dst = _compat_pairs(source, target, ia, ib, "match_compatibility")
    src, dst, d = _capi.check_compat(src, dst, max_dist)
    box = []

    def ctx():
        if not box:
            box.append(_capi.get_context(device))
        return box[0]
    deg1, deg2 = _capi.compat_degrees(ctx, src, dst, d)
    if not return_bits:
        return deg1, deg2
    return deg1, deg2, _capi.compat_bits(ctx, src, dst, d)


def sc2_pose(source, target, ia, ib, max_dist, compat_dist=None, n_seeds=64, k=20, refine_rounds=5, return_info=False, device=None):
    """A pose from the correspondences ``source[ia] -> target[ib]`` by consensus sets of their compatibility graph (SC2-PCR,
    Chen et al. 2022), for match lists of which a few per cent are right: there ``ransac_pose`` draws no clean triple (at 1 %
    one in 10^6) and ``fgr_pose`` is not dominated by the right matches.

    The graph is ``match_compatibility`` at ``compat_dist`` (``None``: ``max_dist``).  The ``n_seeds`` matches with the largest
    second-order degree are the seeds; a seed's consensus set is itself and the up to ``k - 1`` matches compatible with it
    that share the most compatible neighbours with it (``include/pcr.h``: ``pcr_compat_consensus``; all of that on the GPU, in
    integers).  Every seed with at least 3 members gets ``fit_rigid`` over its members; the poses, rounded to float32, are
    scored against all matches at ``max_dist`` in one call, and the winner -- most inliers, then the earlier seed -- ends as
    ``ransac_pose`` does: refined up to ``refine_rounds`` times over its inliers and returned with its rotation made
    orthonormal.  This is the one-stage, unweighted form: the paper's second selection stage and its spectral (leading
    eigenvector) weights are left out -- once the winner is refined over all its inliers they add nothing on the cases
    measured (``docs/EXPERIMENTS.md``).  Deterministic: the same call twice returns the same bits.

    -> ``T`` (4, 4) float64; fewer than 3 matches or no seed with 3 members: ``ransac_pose``'s no-match result, the identity
    and count 0.  With ``return_info`` also a dict with ``pose``, ``inliers``, ``count``, ``fitness``, ``rmse`` as for
    ``ransac_pose`` -- and its ``hypothesis`` (the winning seed's position in ``seeds``, -1: none) and ``n_valid`` (the seeds
    that were fitted) -- plus ``deg1``, ``deg2`` (M,) int64, ``seeds`` (S,), ``members`` and ``scores`` (S, k) int32 (-1:
    empty slot), ``seed`` (the winning seed's row, -1: none) and ``counts`` (S,) int32 (-1: fewer than 3 members).
    More than ``PCR_COMPAT_M_MAX`` = 32768 matches: ValueError."""
    src, dst = _compat_pairs(source, target, ia, ib, "sc2_pose")
    m = len(src)
    refine_rounds = int(refine_rounds)
    if refine_rounds < 0:
        raise ValueError("refine_rounds must be >= 0")
    max_dist = _capi.check_distance(max_dist, "max_dist")
    src, dst, d = _capi.check_compat(src, dst, max_dist if compat_dist is None else compat_dist)
    box = []

    def ctx():
        if not box:
            box.append(_capi.get_context(device))
        return box[0]
    res = _capi.compat_consensus(ctx, src, dst, d, n_seeds, k)
    members = res["members"]
    sizes = (members >= 0).sum(axis=1)
    counts = np.full(len(members), -1, np.int32)
    fitted = np.flatnonzero(sizes >= 3)
    T, count, mask, rmse, win = np.eye(4), 0, np.zeros(m, bool), np.inf, -1
    pose = _poses12(T)[0][0]
    if len(fitted):
        Ts = np.stack([fit_rigid(src[members[e, :sizes[e]]], dst[members[e, :sizes[e]]]) for e in fitted])
        counts[fitted] = _capi.pose_score(ctx, src, dst, _poses12(Ts)[0], max_dist)
        win = int(np.argmax(counts))                            # the first of the largest: ties to the earlier seed

        def score(Tc):
            c, msk = _capi.pose_score(ctx, src, dst, _poses12(Tc)[0], max_dist, want_mask=True)
            return int(c[0]), msk[0]
        T, count, mask, rmse = refine_pose(score, src, dst, Ts[int(np.searchsorted(fitted, win))], refine_rounds)
        pose = _poses12(T)[0][0]
        T = _proper(T)
    if not return_info:
        return T
    return T, {"pose": pose, "inliers": mask, "count": int(count), "fitness": count / m if m else 0.0, "rmse": rmse, "hypothesis": win,
               "n_valid": int(len(fitted)), "deg1": res["deg1"], "deg2": res["deg2"], "seeds": res["seeds"], "members": members,
               "scores": res["scores"], "seed": int(res["seeds"][win]) if win >= 0 else -1, "counts": counts}


def _keypoint_rows(rows, n, name):
    rows = np.asarray(rows)
    if rows.ndim != 1 or (len(rows) and not np.issubdtype(rows.dtype, np.integer)):
        raise ValueError(f"keypoints: the {name} rows must be a vector of integer row indices")
    rows = rows.astype(np.int64)
    if len(rows) and (rows.min() < 0 or rows.max() >= n):
        raise ValueError(f"keypoints: the {name} rows point outside {name}")
    if len(np.unique(rows)) != len(rows):
        raise ValueError(f"keypoints: the {name} rows must not repeat")
    return rows


def register_global(source, target, feature_radius, max_dist, normals=None, mutual=True, ratio=None, device=None, keypoints=None,
                    keypoint_args=None, method="ransac", **ransac):
    """Global registration end to end: ``compute_fpfh`` on both clouds at ``feature_radius``, ``match_features`` (source
    against target, ``mutual`` / ``ratio``), then ``ransac_pose`` with the remaining keywords.  ``normals``: ``None`` to
    estimate them, or a pair ``(source_normals, target_normals)``.  ``method="fgr"`` hands the matches and the remaining
    keywords to ``fgr_pose`` instead, ``method="sc2"`` to ``sc2_pose`` (at most 32768 matches: the choice where only a few per
    cent of them are right).

    ``keypoints``: ``None`` describes and matches every point; ``"iss"`` detects ISS keypoints on both clouds
    (``iss_keypoints(cloud, **keypoint_args)``); a pair ``(source_rows, target_rows)`` uses the caller's own.  Descriptors are
    then computed at those rows only (``compute_fpfh_rows``), a few thousand rows are matched instead of every point, and the
    matches are mapped back to rows of ``source`` and ``target`` before ``ransac_pose``.  Fewer than 3 keypoints on either side
    give no matches: ``ransac_pose``'s no-match result."""
    if method not in ("ransac", "fgr", "sc2"):
        raise ValueError('method must be "ransac", "fgr" or "sc2"')
    pose_from_matches = {"ransac": ransac_pose, "fgr": fgr_pose, "sc2": sc2_pose}[method]
    ns, nt = (None, None) if normals is None else normals
    if keypoints is None:
        if keypoint_args is not None:
            raise ValueError("keypoint_args needs keypoints")
        fs = compute_fpfh(source, ns, radius=feature_radius, device=device)
        ft = compute_fpfh(target, nt, radius=feature_radius, device=device)
        ia, ib, _ = match_features(fs, ft, mutual=mutual, ratio=ratio, device=device)
        return pose_from_matches(source, target, ia, ib, max_dist, device=device, **ransac)
    if isinstance(keypoints, str):
        if keypoints != "iss":
            raise ValueError('keypoints must be None, "iss" or a pair (source_rows, target_rows)')
        args = dict(keypoint_args or {})
        if "return_saliency" in args or "device" in args:
            raise ValueError("keypoint_args takes the detector's parameters only")
        ks = iss_keypoints(source, device=device, **args)
        kt = iss_keypoints(target, device=device, **args)
    else:
        if keypoint_args is not None:
            raise ValueError('keypoint_args needs keypoints="iss"')
        try:
            ks, kt = keypoints
        except (TypeError, ValueError):
            raise ValueError('keypoints must be None, "iss" or a pair (source_rows, target_rows)') from None
        ks, kt = _keypoint_rows(ks, len(np.asarray(source)), "source"), _keypoint_rows(kt, len(np.asarray(target)), "target")
    if len(ks) < 3 or len(kt) < 3:
        ia = ib = np.zeros(0, np.int64)
    else:
        fs = compute_fpfh_rows(source, ks, ns, radius=feature_radius, device=device)
        ft = compute_fpfh_rows(target, kt, nt, radius=feature_radius, device=device)
        ia, ib, _ = match_features(fs, ft, mutual=mutual, ratio=ratio, device=device)
        ia, ib = ks[ia], kt[ib]
    return pose_from_matches(source, target, ia, ib, max_dist, device=device, **ransac)
