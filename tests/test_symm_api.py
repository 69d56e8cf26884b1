"""SymmetricICP without a device: the class is exported, refuses what it does not do before touching the GPU, the C ABI
carries its entry points, and the NumPy restatement the GPU tests compare against (tests/symm_cases.py) reproduces PlaneICP's
golden sums where the two objectives coincide."""

import numpy as np
import pytest

import symm_cases as sc
from conftest import step_err


def test_exported():
    import point_cloud_registration_amd as pcr
    assert "SymmetricICP" in pcr.__all__ and issubclass(pcr.SymmetricICP, pcr.Registration)
    s = pcr.SymmetricICP()
    assert (s.max_iter, s.max_dist, s.tol, s.k, s.min_normal_cos) == (30, 2, 1e-3, 10, 0.0)
    assert pcr.SymmetricICP(min_normal_cos=1.0).min_normal_cos == 1.0


def test_refusals_without_a_device():
    import point_cloud_registration_amd as pcr
    with pytest.raises(ValueError):
        pcr.SymmetricICP(devices=[0, 0])
    with pytest.raises(ValueError):
        pcr.SymmetricICP(comm=object())
    for k in (0, 65):
        with pytest.raises(ValueError):
            pcr.SymmetricICP(k=k)
    for c in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            pcr.SymmetricICP(min_normal_cos=c)
    s = pcr.SymmetricICP()
    src = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="Target is not set."):
        s.align(src)
    with pytest.raises(ValueError, match="Target is not set."):
        s.calc_H_g_e2(np.eye(4), src)
    calls = [lambda: s.linearize(np.eye(4), src), lambda: s.coreset(np.eye(4), src),
             lambda: s.calc_H_g_e2(np.eye(4), src, weights=np.ones(4)), lambda: s.align_batch([src]),
             lambda: s.calc_H_g_e2_batch(np.eye(4)[None], [src])]
    for call in calls:
        with pytest.raises(NotImplementedError, match="SymmetricICP"):
            call()


def test_prototypes():
    from point_cloud_registration_amd import _capi
    for name in ("pcr_scan_estimate_normals", "pcr_scan_set_normals", "pcr_scan_get_normals", "pcr_symm_linearize", "pcr_symm_align"):
        assert name in _capi.PROTOTYPES, name
    for name in ("estimate_normals", "set_normals", "get_normals"):
        assert callable(getattr(_capi.Scan, name))
    assert callable(_capi.symm_linearize) and callable(_capi.symm_align)


def test_restatement_is_plane_icp_where_the_normals_agree(g2):
    """R n_p = +-n_q up to the float32 rounding of n_p: m = n_q up to 2^-25 per component, the sums are PlaneICP's.  Measured in
    NumPy: 7.7e-8 of max|H|, 1.8e-7 relative on e2 -- the bounds are that rounding with a margin of about ten and five."""
    T, src, tgt = g2["T"], g2["source"], g2["target"]
    mask = g2["nn_dist"] < np.float32(float(g2["max_dist"]))
    assert int(mask.sum()) == 1823
    n_p, nq = sc.plane_case(g2)
    c = sc.dots(T, n_p, nq[g2["nn_idx"]])
    assert np.all(np.abs(np.abs(c[mask]) - 1.0) < 1e-5) and 0.4 < np.mean(c[mask] < 0) < 0.6
    t = sc.terms(T, src, sc.xform32(T, src), tgt[g2["nn_idx"]], n_p, nq[g2["nn_idx"]], mask)
    ref, bound, kept = sc.reference(t, sc.kept(T, n_p, nq[g2["nn_idx"]], mask))
    assert kept == 1823
    H, g, e2 = sc.unpack28(ref)
    eH = np.max(np.abs(H - g2["T_plane_H"])) / np.max(np.abs(g2["T_plane_H"]))
    ee = abs(e2 - float(g2["T_plane_e2"])) / float(g2["T_plane_e2"])
    se = step_err(H, g, g2["T_plane_H"], g2["T_plane_g"])
    print(f"max|dH| / max|H| {eH:.3e}, |de2| / e2 {ee:.3e}, step error {se:.3e}")
    assert eH <= 2.0 ** -20 and ee <= 2.0 ** -20 and se <= 1e-6
    # the bound itself: a few thousand roundings of the magnitudes, far below the float32 effect above
    assert np.all(bound[:21] <= 1e-12 * np.max(np.abs(ref[:21])))


def test_restatement_sign_and_gate(g2):
    """Negating normals on either side leaves the restated terms unchanged bit for bit; the gate keeps what it should."""
    T, src, tgt = g2["T"], g2["source"], g2["target"]
    mask = g2["nn_dist"] < np.float32(float(g2["max_dist"]))
    n_p, nq = sc.unit_normals(len(src)), g2["plane_normals"][g2["nn_idx"]]
    tp, q = sc.xform32(T, src), tgt[g2["nn_idx"]]
    t = sc.terms(T, src, tp, q, n_p, nq, mask)
    flip = np.random.default_rng(5).random(len(src)) < 0.5
    assert np.array_equal(t, sc.terms(T, src, tp, q, np.where(flip[:, None], -n_p, n_p), nq, mask))
    assert np.array_equal(t, sc.terms(T, src, tp, q, n_p, np.where(flip[:, None], -nq, nq), mask))
    c = sc.dots(T, n_p, nq)
    assert np.min(np.abs(c[mask])) > 1e-6 and 0.4 < np.mean(c[mask] < 0) < 0.6
    keep = sc.kept(T, n_p, nq, mask, 0.5)
    assert int(keep.sum()) == 912 and np.min(np.abs(np.abs(c[mask]) - 0.5)) > 1e-9
    assert not np.any(sc.kept(T, n_p, nq, mask, 1.0))
    nan = n_p.copy()
    nan[0] = np.nan
    assert not sc.kept(T, nan, nq, np.ones(len(src), bool))[0]
