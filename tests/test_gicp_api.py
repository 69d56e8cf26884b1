"""GICP without a device: the class is exported, refuses what it does not do before touching the GPU, the C ABI carries
its entry points, and the NumPy restatement the GPU tests compare against (tests/gicp_cases.py) agrees with itself."""

import numpy as np
import pytest

import gicp_cases as gc


def test_exported():
    import point_cloud_registration_amd as pcr
    assert "GICP" in pcr.__all__ and issubclass(pcr.GICP, pcr.Registration)
    g = pcr.GICP()
    assert (g.max_iter, g.max_dist, g.tol, g.k, g.eps, g.regularization) == (30, 2, 1e-3, 10, 1e-3, "plane")
    assert pcr.GICP(regularization="raw").regularization == "raw"


def test_refusals_without_a_device():
    import point_cloud_registration_amd as pcr
    with pytest.raises(ValueError):
        pcr.GICP(devices=[0, 0])
    with pytest.raises(ValueError):
        pcr.GICP(comm=object())
    with pytest.raises(ValueError):
        pcr.GICP(regularization="frobenius")
    for k in (0, 65):
        with pytest.raises(ValueError):
            pcr.GICP(k=k)
    g = pcr.GICP()
    src = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="Target is not set."):
        g.align(src)
    with pytest.raises(ValueError, match="Target is not set."):
        g.calc_H_g_e2(np.eye(4), src)
    calls = [lambda: g.linearize(np.eye(4), src), lambda: g.coreset(np.eye(4), src),
             lambda: g.calc_H_g_e2(np.eye(4), src, weights=np.ones(4)), lambda: g.align_batch([src]),
             lambda: g.calc_H_g_e2_batch(np.eye(4)[None], [src])]
    for call in calls:
        with pytest.raises(NotImplementedError, match="GICP"):
            call()


def test_prototypes():
    from point_cloud_registration_amd import _capi
    names = [f"pcr_{side}_{verb}_covariances" for side in ("target", "scan") for verb in ("estimate", "set", "get")]
    for name in names + ["pcr_gicp_linearize", "pcr_gicp_align"]:
        assert name in _capi.PROTOTYPES, name
    assert _capi.ABI_VERSION == 5
    c = np.arange(18.0).reshape(2, 3, 3)
    assert np.array_equal(_capi.cov6(c), np.array([[0, 1, 2, 4, 5, 8], [9, 10, 11, 13, 14, 17]], np.float32))


def brute_knn(points, queries, k):
    P = points.astype(np.float64)
    d2 = ((P[queries][:, None, :] - P[None, :, :]) ** 2).sum(axis=2)
    return np.argsort(d2, axis=1, kind="stable")[:, :k]


def test_covariance_restatement_agrees_with_itself(g2):
    pts = g2["target"]
    q = np.arange(0, 5000, 25)
    nbr = brute_knn(pts, q, 10)
    C, raw, gap = gc.covariance(pts, nbr, "plane", 1e-3)          # (rows of nbr index pts; row r belongs to point q[r])
    for r in range(50):
        ref = np.cov(pts[nbr[r]].astype(np.float64).T, bias=True)
        assert np.allclose(gc.full3(raw[r:r + 1])[0], ref, rtol=1e-10, atol=1e-14)
    lam = np.linalg.eigvalsh(gc.full3(C))
    assert np.max(np.abs(lam - np.array([1e-3, 1.0, 1.0]))) < 1e-12
    assert np.mean(gap > 0.05) >= 0.95
    # padding: a row with 4 real neighbours is the covariance of those 4
    pad = nbr[:1].copy()
    pad[0, 4:] = len(pts)
    raw4 = gc.covariance(pts, pad, "raw")[0]
    assert np.allclose(gc.full3(raw4)[0], np.cov(pts[pad[0, :4]].astype(np.float64).T, bias=True), rtol=1e-10, atol=1e-14)


def test_sum_restatement_agrees_with_itself(g2):
    """Two float64 restatements of the sums on g2 (LAPACK inverse vs adjugate, forward vs reversed order) differ by a few
    ulps of max|H|: far inside the bound the GPU test applies."""
    from point_cloud_registration_amd.math_tools import transform_points
    T, src, tgt = g2["T"], g2["source"], g2["target"]
    md = float(g2["max_dist"])
    mask = g2["nn_dist"] < np.float32(md)
    assert int(mask.sum()) == 1823
    rng = np.random.default_rng(0)
    Cp, Cq_all = gc.random_spd(len(src), rng), gc.random_spd(len(tgt), rng)
    for C in (Cp, Cq_all):
        lam = np.linalg.eigvalsh(gc.full3(C))
        assert lam.min() > 0 and (lam[:, 2] / lam[:, 0]).max() <= 100.0
    tp = transform_points(T.astype(np.float32), src)
    q, Cq = tgt[g2["nn_idx"]], Cq_all[g2["nn_idx"]]
    t, eps_min = gc.terms(T, src, tp, q, Cp, Cq, mask)
    ref, mag = gc.fsum_cols(t)
    bound = gc.sum_bound(int(mask.sum()), eps_min, mag)
    # second restatement: adjugate inverse, per-point loop, reversed order
    R = T[:3, :3]
    d = (tp - q).astype(np.float64)
    J = gc.jacobians(T, src)
    H, g, e2 = np.zeros((6, 6)), np.zeros(6), 0.0
    for i in np.nonzero(mask)[0][::-1]:
        S = gc.full3(Cq[i:i + 1])[0] + R @ gc.full3(Cp[i:i + 1])[0] @ R.T
        adj = np.array([[S[1, 1] * S[2, 2] - S[1, 2] ** 2, S[0, 2] * S[1, 2] - S[0, 1] * S[2, 2], S[0, 1] * S[1, 2] - S[0, 2] * S[1, 1]],
                        [0, S[0, 0] * S[2, 2] - S[0, 2] ** 2, S[0, 1] * S[0, 2] - S[0, 0] * S[1, 2]],
                        [0, 0, S[0, 0] * S[1, 1] - S[0, 1] ** 2]])
        adj = adj + np.triu(adj, 1).T
        M = adj / np.linalg.det(S)
        H += J[i].T @ M @ J[i]
        g += J[i].T @ M @ d[i]
        e2 += d[i] @ M @ d[i]
    other = np.concatenate([H[gc.TRIU], g, [e2]])
    assert np.all(np.abs(other - ref) <= bound)
    Href = gc.unpack28(ref)[0]
    assert np.max(np.abs(H - Href)) <= 1e-13 * np.max(np.abs(Href))
