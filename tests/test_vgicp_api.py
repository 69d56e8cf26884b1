"""VGICP without a device: the class is exported, refuses what it does not do before touching the GPU, the C ABI carries
its entry points, and the NumPy restatement the GPU tests compare against (tests/vgicp_cases.py) agrees with a plain
per-point loop."""

import numpy as np
import pytest

import gicp_cases as gc
import vgicp_cases as vc


def test_exported():
    import point_cloud_registration_amd as pcr
    assert "VGICP" in pcr.__all__ and issubclass(pcr.VGICP, pcr.Registration)
    v = pcr.VGICP()
    assert (v.voxel_size, v.max_iter, v.max_dist, v.tol, v.k, v.eps, v.regularization) == (1.0, 30, 2, 1e-3, 10, 1e-3, "plane")
    v = pcr.VGICP(voxel_size=0.5, max_dist=2.0, k=20, regularization="raw")
    assert (v.voxel_size, v.max_dist, v.k, v.regularization) == (0.5, 2.0, 20, "raw")
    # the scan side is GICP's, not a copy of it
    assert pcr.VGICP._gicp_scan is pcr.GICP._gicp_scan and pcr.VGICP.source_covariance is pcr.GICP.source_covariance
    # ... and the pass is the base class's: no per-class copies of align, calc_H_g_e2 or the stubs
    from point_cloud_registration_amd.gicp import DistributionPass
    for name in ("align", "calc_H_g_e2", "linearize", "coreset", "align_batch", "calc_H_g_e2_batch"):
        assert getattr(pcr.VGICP, name) is getattr(DistributionPass, name) is getattr(pcr.GICP, name), name
        assert name not in vars(pcr.VGICP) and name not in vars(pcr.GICP), name


def test_refusals_without_a_device():
    import point_cloud_registration_amd as pcr
    with pytest.raises(ValueError):
        pcr.VGICP(devices=[0, 0])
    with pytest.raises(ValueError):
        pcr.VGICP(comm=object())
    with pytest.raises(ValueError):
        pcr.VGICP(regularization="frobenius")
    for k in (0, 65):
        with pytest.raises(ValueError):
            pcr.VGICP(k=k)
    v = pcr.VGICP()
    src = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="Target is not set."):
        v.align(src)
    with pytest.raises(ValueError, match="Target is not set."):
        v.calc_H_g_e2(np.eye(4), src)
    with pytest.raises(ValueError, match="Target is not set."):
        v.set_covariance(np.zeros((1, 6)))
    calls = [lambda: v.linearize(np.eye(4), src), lambda: v.coreset(np.eye(4), src),
             lambda: v.calc_H_g_e2(np.eye(4), src, weights=np.ones(4)), lambda: v.align_batch([src]),
             lambda: v.calc_H_g_e2_batch(np.eye(4)[None], [src])]
    for call in calls:
        with pytest.raises(NotImplementedError, match="VGICP"):
            call()


def test_prototypes():
    from point_cloud_registration_amd import _capi
    for name in ("pcr_target_voxels_set_covariances", "pcr_target_voxels_get_covariances", "pcr_vgicp_linearize",
                 "pcr_vgicp_align"):
        assert name in _capi.PROTOTYPES, name
    assert _capi.ABI_VERSION == 5
    for name in ("set_voxel_covariances", "get_voxel_covariances"):
        assert callable(getattr(_capi.Target, name))
    assert callable(_capi.vgicp_linearize) and callable(_capi.vgicp_align)
    c = np.arange(18.0).reshape(2, 3, 3)
    out = _capi.cov6_f64(c)
    assert out.dtype == np.float64 and np.array_equal(out, np.array([[0, 1, 2, 4, 5, 8], [9, 10, 11, 13, 14, 17]], np.float64))


def test_plane_cov_restatement():
    rng = np.random.default_rng(5)
    n = rng.normal(size=(40, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    C = vc.plane_cov(n, 1e-3)
    assert C.shape == (40, 6) and C.dtype == np.float64
    lam = np.linalg.eigvalsh(gc.full3(C))
    assert np.max(np.abs(lam - np.array([1e-3, 1.0, 1.0]))) < 1e-12
    assert np.array_equal(C, vc.plane_cov(-n, 1e-3))                    # the sign of the normal does not matter


def test_sum_restatement_agrees_with_a_per_point_loop(g2):
    """vgicp_cases.terms against a plain per-point numpy.linalg.inv loop on 50 points of g2, from the golden centroid matches."""
    T, src, md = g2["T"], g2["source"], float(g2["max_dist"])
    mu_all, idx = g2["vox_mean"], g2["vox_idx"]
    tp = vc.xform32(T, src)
    dist, brute = vc.nearest_centroid(tp, mu_all)
    assert np.array_equal(brute, idx)                                   # a brute force reproduces the golden matches
    mask = dist < md
    assert int(mask.sum()) == 1785 and np.array_equal(mask, g2["vox_dist"] < md)
    assert np.min(np.abs(dist / md - 1.0)) > 1.3e-3
    rng = np.random.default_rng(0)
    Cp = gc.random_spd(len(src), rng)
    Cv = gc.random_spd(len(mu_all), rng).astype(np.float64)
    t, eps_min = vc.terms(T, src, tp, mu_all[idx], Cp, Cv[idx], mask)
    assert eps_min > 0 and np.all(t[~mask] == 0)
    R = T[:3, :3]
    from point_cloud_registration_amd.math_tools import skew
    for i in np.nonzero(mask)[0][:50]:
        M = np.linalg.inv(gc.full3(Cv[idx[i]][None])[0] + R @ gc.full3(Cp[i][None])[0] @ R.T)
        J = np.hstack([np.eye(3), -R @ skew(src[i].astype(np.float64))])
        d = tp[i].astype(np.float64) - mu_all[idx[i]]
        H, g, e2 = J.T @ M @ J, J.T @ M @ d, d @ M @ d
        ref = np.concatenate([H[gc.TRIU], g, [e2]])
        assert np.allclose(t[i], ref, rtol=1e-10, atol=1e-12 * np.max(np.abs(ref)))
    # the sums of the restatement are the sums of its terms
    H, g, e2, kept = vc.sums(T, src, mu_all, Cp, Cv, md)
    ref = gc.fsum_cols(t)[0]
    assert kept == 1785 and np.array_equal(np.concatenate([H[gc.TRIU], g, [e2]]), ref)
