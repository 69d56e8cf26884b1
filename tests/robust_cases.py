"""Float64 NumPy restatement of the robust kernels of include/pcr.h and of the passes that use them, shared by
tests/test_robust_cases.py and tests/test_gpu_robust.py.  Nothing here touches the GPU.

The weight table (s the squared residual, c the scale, c2 = c * c taken once):
  huber   s <= c2 ? 1 : c / sqrt(s)          cauchy  1 / (1 + s / c2)
  tukey   s <= c2 ? (1 - s / c2)^2 : 0       gm      (c2 / (c2 + s))^2
What s is: SymmetricICP r r of its row; ColoredICP r r of EACH row after its sqrt(lambda) / sqrt(1 - lambda) factor, a weight
per row; GICP / VGICP d^T M d.  The restated terms of symm_cases / color_cases / dist_cases carry exactly that number in their
last column (the e2 term), so s is read from there and every row of terms is multiplied by its weight.

The end-to-end case (e2e_case): 4096 points of the street surface at 1 : 10 (12 m x 6 m), analytic normals; a scan of 1024 of
them seen from T_true, a small step from the identity, with 0.5 mm noise; 30 % of the scan points moved rigidly by 0.3 m along
(0.6, 0, 0.8) -- off the ground and off two of the walls, inside max_dist = 1.  E2E_ERRORS records the translation error of the
restated Gauss-Newton loop without and with the kernel."""

import numpy as np

import color_cases as cc
import dist_cases as dc
import gicp_cases as gc
import symm_cases as sc
import vgicp_cases as vc

KINDS = ("huber", "cauchy", "tukey", "gm")


def weight(kind, s, c):
    """The table above on an array of s (inf allowed: 0, also for ``None``)."""
    s = np.asarray(s, dtype=np.float64)
    if kind is None:
        return np.where(np.isinf(s), 0.0, 1.0)
    c = np.float64(c)
    c2 = c * c
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == "huber":
            return np.where(s <= c2, 1.0, c / np.sqrt(s))
        if kind == "cauchy":
            return 1.0 / (1.0 + s / c2)
        if kind == "tukey":
            u = 1.0 - s / c2
            return np.where(s <= c2, u * u, 0.0)
        if kind == "gm":
            l = c2 / (c2 + s)
            return l * l
    raise KeyError(kind)


def _weigh(t, keep, kind, c):
    """Rows of unweighted terms (rows outside ``keep`` zero) -> (weighted rows, s per row with inf outside ``keep``)."""
    s = np.where(np.asarray(keep, dtype=bool), t[:, 27], np.inf)
    return t * weight(kind, s, c)[:, None], s


def terms_symm(kind, c, T, src, tp, q, n_p, n_q, mask, min_cos=0.0):
    """symm_cases.terms under the kernel -> (weighted terms (N, 28), unweighted terms, s (N,), keep)."""
    t = sc.terms(T, src, tp, q, n_p, n_q, mask, min_cos)
    keep = sc.kept(T, n_p, n_q, mask, min_cos)
    tw, s = _weigh(t, keep, kind, c)
    return tw, t, s, keep


def terms_color(kind, c, T, src, tp, q, n_q, I_q, g_q, I_p, mask, lam):
    """color_cases.terms under the kernel, a weight per ROW -> (weighted terms (2 N, 28), unweighted terms, s (N, 2), mask)."""
    t = cc.terms(T, src, tp, q, n_q, I_q, g_q, I_p, mask, lam)
    mask = np.asarray(mask, dtype=bool)
    tw, s = _weigh(t, np.concatenate([mask, mask]), kind, c)
    n = len(mask)
    return tw, t, np.stack([s[:n], s[n:]], axis=1), mask


def terms_dist(kind, c, T, src, tp, q, Cp6, Cq6, mask, residual="f32"):
    """dist_cases.terms_closed under the kernel: M -> w M, every term being linear in M
    -> (weighted terms (N, 28), unweighted terms, s (N,), mask, eps_min)."""
    t, eps_min = dc.terms_closed(T, src, tp, q, Cp6, Cq6, mask, residual)
    mask = np.asarray(mask, dtype=bool)
    tw, s = _weigh(t, mask, kind, c)
    return tw, t, s, mask, eps_min


def median_scale(s):
    """c with c2 = the median of the finite s (the lower of the two middle ones: an s of the set, so both sides of every
    kernel's branch at c2 are taken)."""
    f = np.sort(np.asarray(s)[np.isfinite(s)].ravel())
    return float(np.sqrt(f[(len(f) - 1) // 2]))


def reference(tw, t, bound_of_abs_sums):
    """(math.fsum of the weighted terms per column, 1.5 x the plain pass's bound on the sums of the UNWEIGHTED magnitudes)."""
    ref = gc.fsum_cols(tw)[0]
    mag = gc.fsum_cols(t)[1]
    return ref, 1.5 * bound_of_abs_sums(mag)


# ----------------------------------------------------------------------------- the end-to-end case
E2E_MAX_DIST = 1.0
E2E_TOL = 1e-3
E2E_SHIFT = 0.3 * np.array([0.6, 0.0, 0.8])
E2E_OUTLIERS = 0.3
E2E_LAMBDA = 0.968
E2E_EPS = 1e-3
E2E_VOXEL = 1.0
E2E_KIND = "cauchy"
# c: SymmetricICP / ColoredICP in metres (residuals of inliers: the 0.5 mm noise; of the moved points: up to 0.24 m);
# GICP / VGICP in Mahalanobis units, M ~ 1 / (2 eps) = 500 along the normal
E2E_SCALE = {"symm": 0.02, "color": 0.02, "gicp": 0.5, "vgicp": 0.5}
# |t - t_true| of the restated loop (test_robust_cases.py::test_end_to_end prints them): (plain, robust)
E2E_ERRORS = {"symm": (6.883e-2, 1.318e-3), "color": (6.948e-2, 1.871e-3), "gicp": (6.911e-2, 1.444e-3), "vgicp": (7.662e-2, 2.101e-3)}


def _plane_cov32(n, eps=E2E_EPS):
    return vc.plane_cov(n, eps).astype(np.float32)


def e2e_case():
    """dict: target (4096, 3) f32, n_q, I_q, g_q, Cq; scan (1024, 3) f32, n_p, I_p, Cp, moved (1024,) bool; T_true;
    means, Cv, vnorm of the restated voxels (size E2E_VOXEL, at least 6 points)."""
    from point_cloud_registration_amd.synthetic import make_T, street, street_normals
    raw = street(4096, seed=3)
    target = (raw * 0.1).astype(np.float32)
    n_q = street_normals(raw)
    rng = np.random.default_rng(11)
    idx = rng.choice(4096, 1024, replace=False)
    T_true = make_T((0.01, -0.02, 0.015), (0.05, -0.04, 0.03))
    R, t = T_true[:3, :3], T_true[:3, 3]
    scan = (target[idx].astype(np.float64) - t) @ R + rng.normal(0.0, 0.0005, (1024, 3))      # R^T (q - t)
    moved = np.zeros(1024, bool)
    moved[rng.permutation(1024)[:int(E2E_OUTLIERS * 1024)]] = True
    scan[moved] += E2E_SHIFT
    scan = np.ascontiguousarray(scan, dtype=np.float32)
    n_p = (n_q[idx].astype(np.float64) @ R).astype(np.float32)                                 # R^T n
    P = target.astype(np.float64)
    I_q = cc.field(target)
    g_q = np.stack([0.42 * np.cos(2.1 * P[:, 0] + 0.3), -0.34 * np.sin(1.7 * P[:, 1]), 0.13 * np.cos(1.3 * P[:, 2])], axis=1).astype(np.float32)
    # voxels: the points of a cell, at least 6; centroid; the majority normal of its points as the plane of its covariance
    key = np.floor(P / E2E_VOXEL).astype(np.int64)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.ravel()
    means, vnorm = [], []
    for v in np.nonzero(cnt >= 6)[0]:
        m = inv == v
        means.append(P[m].mean(axis=0))
        vnorm.append(np.eye(3)[np.argmax(n_q[m].astype(np.float64).sum(axis=0))])
    means, vnorm = np.array(means), np.array(vnorm)
    out = dict(target=target, n_q=n_q, I_q=I_q, g_q=g_q, Cq=_plane_cov32(n_q), scan=scan, n_p=n_p, I_p=I_q[idx].copy(), Cp=_plane_cov32(n_p),
               moved=moved, T_true=T_true, means=means, vnorm=vnorm, Cv=vc.plane_cov(vnorm, E2E_EPS))
    for a in out.values():
        a.setflags(write=False)
    return out


def _nn32(tp, target):
    dd = tp[:, None, :] - target[None, :, :]                                    # float32
    d2 = (dd[:, :, 0] * dd[:, :, 0] + dd[:, :, 1] * dd[:, :, 1]) + dd[:, :, 2] * dd[:, :, 2]
    j = np.argmin(d2, axis=1)
    return j, np.sqrt(d2[np.arange(len(tp)), j]) < np.float32(E2E_MAX_DIST)


def e2e_terms(family, case, T, kind, c):
    """The weighted terms of one pass of ``family`` over the case at T, correspondences by brute force."""
    scan = case["scan"]
    tp = sc.xform32(T, scan)
    if family == "vgicp":
        dist, j = vc.nearest_centroid(tp, case["means"])
        return terms_dist(kind, c, T, scan, tp, case["means"][j], case["Cp"], case["Cv"][j], dist < E2E_MAX_DIST, "f64")[0]
    j, mask = _nn32(tp, case["target"])
    q = case["target"][j]
    if family == "symm":
        return terms_symm(kind, c, T, scan, tp, q, case["n_p"], case["n_q"][j], mask)[0]
    if family == "color":
        return terms_color(kind, c, T, scan, tp, q, case["n_q"][j], case["I_q"][j], case["g_q"][j], case["I_p"], mask, E2E_LAMBDA)[0]
    return terms_dist(kind, c, T, scan, tp, q, case["Cp"], case["Cq"][j], mask, "f32")[0]


def gn_loop(family, case, kind, c, max_iter=30, tol=E2E_TOL, T0=None):
    """The restated Gauss-Newton loop, as color_cases.gn_loop: plain float64 sums, the step and stop rule of align
    -> (T, iterations)."""
    from point_cloud_registration_amd.math_tools import plus
    T = np.eye(4) if T0 is None else np.array(T0, dtype=np.float64)
    it = 0
    for it in range(max_iter):
        H, g, _ = gc.unpack28(np.sum(e2e_terms(family, case, T, kind, c), axis=0))
        dx = -np.linalg.solve(H, g)
        if np.linalg.norm(dx) < tol:
            break
        T = plus(T, dx)
    return T, it + 1


def t_err(T, case):
    return float(np.linalg.norm(T[:3, 3] - case["T_true"][:3, 3]))
