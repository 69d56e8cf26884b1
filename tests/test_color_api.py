"""ColoredICP without a device: the class is exported, refuses what it does not do before touching the GPU, the C ABI carries
its entry points, and the NumPy restatement the GPU tests compare against (tests/color_cases.py) has the properties the
definition promises: exact gradients on a plane, the zero rules, a Jacobian that is the derivative of its residual, PlaneICP's
golden sums at lambda = 1, and a Gauss-Newton loop that converges on the street case."""

import numpy as np
import pytest

import color_cases as cc
import gicp_cases as gc
from conftest import step_err


def test_exported():
    import point_cloud_registration_amd as pcr
    assert "ColoredICP" in pcr.__all__ and issubclass(pcr.ColoredICP, pcr.Registration)
    s = pcr.ColoredICP()
    assert (s.max_iter, s.max_dist, s.tol, s.k, s.lambda_geometric) == (30, 2, 1e-3, 10, 0.968)
    assert pcr.ColoredICP(lambda_geometric=1.0).lambda_geometric == 1.0 and pcr.ColoredICP(lambda_geometric=0).lambda_geometric == 0.0


def test_refusals_without_a_device():
    import point_cloud_registration_amd as pcr
    with pytest.raises(ValueError):
        pcr.ColoredICP(devices=[0, 0])
    with pytest.raises(ValueError):
        pcr.ColoredICP(comm=object())
    for k in (0, 65):
        with pytest.raises(ValueError):
            pcr.ColoredICP(k=k)
    for lam in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError):
            pcr.ColoredICP(lambda_geometric=lam)
    s = pcr.ColoredICP()
    src, inten = np.zeros((4, 3), np.float32), np.zeros(4, np.float32)
    with pytest.raises(ValueError, match="Target is not set."):
        s.align(src, inten)
    with pytest.raises(ValueError, match="Target is not set."):
        s.calc_H_g_e2(np.eye(4), src, inten)
    # shapes are checked before anything is uploaded
    for bad in (np.zeros(3, np.float32), np.zeros((4, 2), np.float32)):
        with pytest.raises(ValueError):
            s.set_target(src, bad)
    with pytest.raises(ValueError):
        s.set_target(src, inten, norm=np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError):
        s.set_target(src, inten, norm=np.zeros((4, 3), np.float32), gradient=np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError):
        s.set_target(src, np.float32([0, 1, np.nan, 0]))
    assert not s.is_target_set()
    calls = [lambda: s.linearize(np.eye(4), src), lambda: s.coreset(np.eye(4), src),
             lambda: s.calc_H_g_e2(np.eye(4), src, inten, weights=np.ones(4)), lambda: s.align_batch([src]),
             lambda: s.calc_H_g_e2_batch(np.eye(4)[None], [src])]
    for call in calls:
        with pytest.raises(NotImplementedError, match="ColoredICP"):
            call()


def test_colours_reduce_to_intensity():
    from point_cloud_registration_amd.colored_icp import as_intensity
    rgb = np.random.default_rng(0).uniform(0, 1, (7, 3))
    out = as_intensity(rgb, 7, "c")
    assert out.dtype == np.float32 and np.array_equal(out, ((rgb[:, 0] + rgb[:, 1] + rgb[:, 2]) / 3.0).astype(np.float32))
    assert np.array_equal(as_intensity(out, 7, "c"), out)


def test_prototypes():
    from point_cloud_registration_amd import _capi
    for name in ("pcr_target_set_intensity", "pcr_target_estimate_color_gradients", "pcr_target_get_color", "pcr_scan_set_intensity",
                 "pcr_scan_get_intensity", "pcr_color_linearize", "pcr_color_align"):
        assert name in _capi.PROTOTYPES, name
    for name in ("set_intensity", "estimate_color_gradients", "get_color"):
        assert callable(getattr(_capi.Target, name))
    for name in ("set_intensity", "get_intensity"):
        assert callable(getattr(_capi.Scan, name))
    assert callable(_capi.color_linearize) and callable(_capi.color_align)


# ----------------------------------------------------------------------------- the restated gradient
def test_restated_gradient_on_a_plane():
    """z = 0 exactly, normals (0, 0, 1), I linear in x and y: the least-squares system is consistent, so the restated gradient
    is the tangent part of the coefficient to the float64 rounding of the 3 x 3 solve (measured: 2.2e-16 absolute on a
    coefficient of size 0.4 at cond(M) up to 2.5e3; the intensities are float32-exact, so nothing else rounds)."""
    rng = np.random.default_rng(11)
    P = np.zeros((300, 3), np.float32)
    P[:, :2] = rng.integers(-2048, 2048, (300, 2)) / 1024.0
    P = np.unique(P, axis=0)
    nrm = np.tile(np.float32([0, 0, 1]), (len(P), 1))
    coef = np.array([0.25, -0.375, 0.5])                                         # (the z part is not tangent)
    I = (P.astype(np.float64) @ coef + 1.0).astype(np.float32)
    assert np.array_equal(I.astype(np.float64), P.astype(np.float64) @ coef + 1.0)
    nbr = cc.knn_brute(P, 10)
    g, cond, w = cc.gradient(P, nrm, I, nbr, full=True)
    err = np.max(np.abs(g - np.array([0.25, -0.375, 0.0])))
    print(f"max |g - coefficient| {err:.3e}, largest cond(M) {cond.max():.3e}")
    assert np.all(w == 9) and err <= 64 * cond.max() * gc.EPS53
    # doubling the intensities doubles the gradient bit for bit; a constant intensity gives exactly zero
    assert np.array_equal(cc.gradient(P, nrm, 2 * I, nbr), 2 * g)
    assert np.array_equal(cc.gradient(P, nrm, np.full(len(P), 0.7, np.float32), nbr), np.zeros((len(P), 3)))
    # flipping normals changes nothing
    flip = np.where(rng.random(len(P))[:, None] < 0.5, -nrm, nrm)
    assert np.array_equal(cc.gradient(P, flip, I, nbr), g)


def test_restated_gradient_zero_rules():
    # collinear points along x with normals z: M = diag(sum x^2, 0, w^2), det == 0 exactly
    L = np.zeros((12, 3), np.float32)
    L[:, 0] = np.arange(12) * 0.25
    nz = np.tile(np.float32([0, 0, 1]), (12, 1))
    I = cc.field(L)
    assert np.ptp(I) > 0.1
    g, cond, w = cc.gradient(L, nz, I, cc.knn_brute(L, 6), full=True)
    assert np.all(w == 5) and np.array_equal(g, np.zeros((12, 3))) and np.all(np.isinf(cond))
    # three points: w = 2 < 3
    P = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    g, _, w = cc.gradient(P, nz[:3], np.float32([0, 1, 2]), cc.knn_brute(P, 10), full=True)
    assert np.all(w == 2) and np.array_equal(g, np.zeros((3, 3)))
    # four points in general position on the plane: a gradient again
    P = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
    g = cc.gradient(P, nz[:4], np.float32([0, 1, 2, 3]), cc.knn_brute(P, 10))
    assert np.max(np.abs(g - [1.0, 2.0, 0.0])) < 1e-12
    # duplicates of the point itself are left out
    P = np.float32([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0]])
    _, _, w = cc.gradient(P, nz[:4], np.float32([0, 0, 1, 2]), cc.knn_brute(P, 10), full=True)
    assert list(w) == [2, 2, 3, 3]


# ----------------------------------------------------------------------------- the restated rows
@pytest.fixture(scope="module")
def g2_color(g2):
    """g2 with colour: I = field(target), the restated k = 10 gradients over a brute-force k-NN, scan intensities from the field
    at the transformed scan."""
    tgt, src, T = g2["target"], g2["source"], g2["T"]
    I_q = cc.field(tgt)
    g_q = cc.gradient(tgt, g2["plane_normals"], I_q, cc.knn_brute(tgt, 10)).astype(np.float32)
    return I_q, g_q, cc.field(cc.xform32(T, src))


def test_colour_jacobian_is_the_derivative(g2, g2_color):
    """J_C against the central difference of r_C under plus(T, h e_i), correspondences fixed.  The difference's own error is
    second order: (h^2 / 6) |r'''|, and r_C is linear in t and trigonometric in the rotation with |p| <= 32 m and |m| <= 8, so
    relative to max|J_C| of the column it is below h^2 = 1e-10; its cancellation adds 2^-53 |r| / h ~ 1e-10.  Asserted: 1e-8
    relative, a margin of a hundred over h^2.  Measured: 3.1e-11."""
    from point_cloud_registration_amd.math_tools import plus
    T, src, tgt = g2["T"], g2["source"], g2["target"]
    I_q, g_q, I_p = g2_color
    j = g2["nn_idx"]
    q, nq = tgt[j], g2["plane_normals"][j]

    def r_c(Tx):
        # (the transformed point in float64: the derivative of the definition, not of its float32 rounding)
        tp = src.astype(np.float64) @ Tx[:3, :3].T + Tx[:3, 3]
        m = cc.tangent(g_q[j], nq)
        return (I_q[j].astype(np.float64) - I_p.astype(np.float64)) + cc._dot3(m, tp - q.astype(np.float64))

    JC = cc.rows(T, src, cc.xform32(T, src), q, nq, I_q[j], g_q[j], I_p)[2]
    # quirk Q2, which every row of this project reproduces: the translation block of J is the derivative with respect to t
    # itself, while plus() moves t by R dt.  So under plus(T, h e_i) the rotation columns are J_C's and the translation
    # columns are J_C[:, :3] R; with respect to t they are J_C[:, :3].  All three are checked, to one tolerance.
    R = T[:3, :3]
    expect = np.concatenate([JC[:, :3] @ R, JC[:, 3:]], axis=1)
    h, worst = 1e-5, 0.0
    for i in range(6):
        e = np.zeros(6)
        e[i] = h
        fd = (r_c(plus(T, e)) - r_c(plus(T, -e))) / (2 * h)
        worst = max(worst, np.max(np.abs(fd - expect[:, i])) / np.max(np.abs(JC[:, i])))
        if i < 3:
            Tp, Tm = T.copy(), T.copy()
            Tp[i, 3] += h
            Tm[i, 3] -= h
            fd = (r_c(Tp) - r_c(Tm)) / (2 * h)
            worst = max(worst, np.max(np.abs(fd - JC[:, i])) / np.max(np.abs(JC[:, i])))
    print(f"max |fd - J_C| / max|J_C| per column {worst:.3e}")
    assert worst <= 1e-8


def test_restatement_is_plane_icp_at_lambda_one(g2, g2_color):
    """lambda = 1: a_C = 0, the colour rows vanish exactly and the restated sums are PlaneICP's.  Measured in NumPy against the
    golden: 7.7e-8 on max|dH| / max|H|, 3.1e-8 relative on e2, step error 1.8e-7 -- the figures of the SymmetricICP twin, the
    distance of the golden's own arithmetic from the float64 terms.  Asserted: 2^-20 (9.5e-7, a margin of twelve) and
    step_err <= 1e-6 (a margin of five), the twin's bounds."""
    T, src, tgt = g2["T"], g2["source"], g2["target"]
    I_q, g_q, I_p = g2_color
    j = g2["nn_idx"]
    mask = g2["nn_dist"] < np.float32(float(g2["max_dist"]))
    assert int(mask.sum()) == 1823
    t = cc.terms(T, src, cc.xform32(T, src), tgt[j], g2["plane_normals"][j], I_q[j], g_q[j], I_p, mask, 1.0)
    assert np.array_equal(t[len(src):], np.zeros((len(src), 28)))
    ref, bound, kept = cc.reference(t, mask)
    assert kept == 1823
    H, g, e2 = cc.unpack28(ref)
    eH = np.max(np.abs(H - g2["T_plane_H"])) / np.max(np.abs(g2["T_plane_H"]))
    ee = abs(e2 - float(g2["T_plane_e2"])) / float(g2["T_plane_e2"])
    se = step_err(H, g, g2["T_plane_H"], g2["T_plane_g"])
    print(f"max|dH| / max|H| {eH:.3e}, |de2| / e2 {ee:.3e}, step error {se:.3e}")
    assert eH <= 2.0 ** -20 and ee <= 2.0 ** -20 and se <= 1e-6
    # a zero gradient adds (1 - lambda) (I_q - I_p)^2 to e2 and nothing else
    lam = 0.5
    t0 = cc.terms(T, src, cc.xform32(T, src), tgt[j], g2["plane_normals"][j], I_q[j], np.zeros_like(g_q[j]), I_p, mask, lam)
    col = t0[len(src):]
    dI = I_q[j].astype(np.float64) - I_p.astype(np.float64)
    assert np.array_equal(col[:, :27], np.zeros((len(src), 27)))
    assert np.allclose(col[mask, 27], (1 - lam) * dI[mask] ** 2, rtol=1e-15, atol=0)


# ----------------------------------------------------------------------------- the restated loop
@pytest.fixture(scope="module")
def street_color():
    target, scan, T_true = gc.align_case()
    nbr = cc.knn_brute(target, 10)
    nrm = cc.pca_normals(target, nbr)
    I_q = cc.field(target)
    g_q = cc.gradient(target, nrm, I_q, nbr).astype(np.float32)
    I_p = cc.field(scan.astype(np.float64) @ T_true[:3, :3].T + T_true[:3, 3])
    return target, scan, T_true, nrm, I_q, g_q, I_p


@pytest.mark.parametrize("lam", [0.968, 0.5])
@pytest.mark.parametrize("max_dist", [2.0, 0.15])
def test_restated_loop_converges(street_color, max_dist, lam):
    target, scan, T_true, nrm, I_q, g_q, I_p = street_color
    T, iters = cc.gn_loop(target, nrm, I_q, g_q, scan, I_p, max_dist, lam, 1e-4)
    dR, dt = np.linalg.norm(T[:3, :3] - T_true[:3, :3]), np.linalg.norm(T[:3, 3] - T_true[:3, 3])
    print(f"max_dist {max_dist} lambda {lam}: {iters} iterations, |dR|_F {dR:.3e}, |dt| {dt:.3e}")
    assert dR < 5e-4 and dt < 5e-4
