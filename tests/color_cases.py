"""Float64 NumPy restatement of the colored-ICP definition (include/pcr.h), with its expression order, and the fixtures of
tests/test_color_api.py and tests/test_gpu_color.py.  Nothing here touches the GPU.

Gradient of target point q (unit normal n, intensity I_q) over neighbours q_i, nearest first, those at distance 0 left out
(w remain): e = q_i - q; en = (e0 n0 + e1 n1) + e2 n2; u = e - en n; M += u u^T; b += u (I_i - I_q); M += w^2 n n^T;
s = adj(M) b / det; g = s - (s . n) n, rounded to float32.  Zero when w < 3, when det is not > 0, when a component is not finite.

One correspondence (scan point p with intensity I_p, matched record (q, n, I_q, g), pose T = (R, t)): d = xform(p) - q formed
in float32 and widened; r_G = n . d, J_G = [n, p x (R^T n)]; m = g - (g . n) n; r_C = (I_q - I_p) + m . d, J_C = [m, p x (R^T m)];
the rows scaled by a_G = sqrt(lambda), a_C = sqrt(1 - lambda); terms of the pair: triu(J^T J) (21), J r (6), r r (1) of both.

Bound per entry of the sums: (2 n_kept + 16) 2^-53 sum |term| -- two rows per pair, otherwise the bound of symm_cases."""

import numpy as np

import gicp_cases as gc
import symm_cases as sc

TRIU = gc.TRIU
fsum_cols = gc.fsum_cols
unpack28 = gc.unpack28
xform32 = sc.xform32


def field(P):
    """The intensity field of every test: evaluated in float64 on the float32 coordinates, rounded to float32."""
    P = np.asarray(P, dtype=np.float32).astype(np.float64)
    return (0.5 + 0.2 * np.sin(2.1 * P[:, 0] + 0.3) + 0.2 * np.cos(1.7 * P[:, 1]) + 0.1 * np.sin(1.3 * P[:, 2])).astype(np.float32)


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def gradient(points, normals, intensity, nbr_idx, full=False):
    """Gradients (N, 3) float64 BEFORE the rounding to float32, over given neighbour indices (N, k), nearest first; entries
    >= len(points) are padding and dropped, as are neighbours that coincide with the point.  ``full``: also cond(M) (inf where
    the gradient is zero by rule) and the number of neighbours used."""
    P = np.asarray(points, dtype=np.float32).astype(np.float64)
    Nn = np.asarray(normals, dtype=np.float32).astype(np.float64)
    I = np.asarray(intensity, dtype=np.float32).astype(np.float64)
    nbr = np.asarray(nbr_idx).reshape(len(P), -1)
    n_pts = len(P)
    M = np.zeros((n_pts, 6))
    b = np.zeros((n_pts, 3))
    w = np.zeros(n_pts, dtype=np.int64)
    for c in range(nbr.shape[1]):
        ok = nbr[:, c] < n_pts
        j = np.where(ok, nbr[:, c], 0)
        e = P[j] - P
        # (the kernel leaves out neighbours whose float32 squared distance is not > 0: the point itself and exact duplicates)
        ok &= np.any(e != 0.0, axis=1)
        en = _dot3(e, Nn)
        u = (e - en[:, None] * Nn) * ok[:, None]
        dI = (I[j] - I) * ok
        M += np.stack([u[:, 0] * u[:, 0], u[:, 0] * u[:, 1], u[:, 0] * u[:, 2], u[:, 1] * u[:, 1], u[:, 1] * u[:, 2],
                       u[:, 2] * u[:, 2]], axis=1)
        b += u * dI[:, None]
        w += ok
    ww = (w * w).astype(np.float64)
    n0, n1, n2 = Nn[:, 0], Nn[:, 1], Nn[:, 2]
    M += ww[:, None] * np.stack([n0 * n0, n0 * n1, n0 * n2, n1 * n1, n1 * n2, n2 * n2], axis=1)
    a_, d_, e_, b_, f_, c_ = (M[:, i] for i in range(6))                    # xx xy xz yy yz zz
    f2, d2, e2 = f_ * f_, d_ * d_, e_ * e_
    bc, ac, ab = b_ * c_, a_ * c_, a_ * b_
    dc, de, ef = d_ * c_, d_ * e_, e_ * f_
    af, df, eb = a_ * f_, d_ * f_, e_ * b_
    det = a_ * bc + 2 * de * f_ - a_ * f2 - b_ * e2 - c_ * d2
    good = (w >= 3) & (det > 0.0)
    with np.errstate(all="ignore"):
        dd = np.where(good, det, 1.0)
        c0, c1, c2 = (bc - f2) / dd, -(dc - ef) / dd, (df - eb) / dd
        c3, c4, c5 = (ac - e2) / dd, -(af - de) / dd, (ab - d2) / dd
        s = np.stack([(c0 * b[:, 0] + c1 * b[:, 1]) + c2 * b[:, 2], (c1 * b[:, 0] + c3 * b[:, 1]) + c4 * b[:, 2],
                      (c2 * b[:, 0] + c4 * b[:, 1]) + c5 * b[:, 2]], axis=1)
        sn = _dot3(s, Nn)
        g = s - sn[:, None] * Nn
        good &= np.all(np.isfinite(g.astype(np.float32)), axis=1)
    g = np.where(good[:, None], g, 0.0)
    if not full:
        return g
    cond = np.full(n_pts, np.inf)
    if np.any(good):
        cond[good] = np.linalg.cond(gc.full3(M[good]))
    return g, cond, w


def gradient_bound(g_ref, cond):
    """Per point: one float32 ulp of the largest component plus the float64 conditioning of the 3 x 3 solve."""
    big = np.max(np.abs(g_ref), axis=1)
    return 2.0 ** -23 * big + 64.0 * cond * gc.EPS53 * big


def tangent(g, n):
    """m = g - (g . n) n, float64, from float32 inputs."""
    g = np.asarray(g, dtype=np.float32).astype(np.float64)
    n = np.asarray(n, dtype=np.float32).astype(np.float64)
    return g - _dot3(g, n)[:, None] * n


def plane_rows(T, src, v, d):
    """PlaneICP's row with v in the place of the normal: (J (N, 6), v . d (N,))."""
    R = np.asarray(T, dtype=np.float64)[:3, :3]
    p = np.asarray(src, dtype=np.float32).astype(np.float64)
    r = _dot3(v, d)
    ra = R[0, 0] * v[:, 0] + R[1, 0] * v[:, 1] + R[2, 0] * v[:, 2]                                     # R^T v
    rb = R[0, 1] * v[:, 0] + R[1, 1] * v[:, 1] + R[2, 1] * v[:, 2]
    rc = R[0, 2] * v[:, 0] + R[1, 2] * v[:, 1] + R[2, 2] * v[:, 2]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([v[:, 0], v[:, 1], v[:, 2], -z * rb + y * rc, z * ra - x * rc, -y * ra + x * rb], axis=1), r


def rows(T, src, tp, q, n_q, I_q, g_q, I_p):
    """The two unscaled rows of every pair: (J_G, r_G, J_C, r_C).  ``tp`` = the float32 transformed scan; ``q``, ``n_q``,
    ``I_q``, ``g_q`` = the matched float32 target record of every scan point."""
    d = (np.asarray(tp, dtype=np.float32) - np.asarray(q, dtype=np.float32)).astype(np.float64)       # float32 subtraction
    n = np.asarray(n_q, dtype=np.float32).astype(np.float64)
    JG, rG = plane_rows(T, src, n, d)
    JC, md = plane_rows(T, src, tangent(g_q, n_q), d)
    dI = np.asarray(I_q, dtype=np.float32).astype(np.float64) - np.asarray(I_p, dtype=np.float32).astype(np.float64)
    return JG, rG, JC, dI + md


def terms(T, src, tp, q, n_q, I_q, g_q, I_p, mask, lam):
    """Per-row terms (2 N, 28): triu(H) 21, g 6, e2 -- the N geometric rows, then the N colour rows; rows of pairs outside
    ``mask`` are zero."""
    JG, rG, JC, rC = rows(T, src, tp, q, n_q, I_q, g_q, I_p)
    aG, aC = np.sqrt(np.float64(lam)), np.sqrt(1.0 - np.float64(lam))
    out = []
    for a, J, r in ((aG, JG, rG), (aC, JC, rC)):
        J, r = a * J, a * r
        t = np.concatenate([J[:, TRIU[0]] * J[:, TRIU[1]], J * r[:, None], (r * r)[:, None]], axis=1)
        t[~np.asarray(mask, dtype=bool)] = 0.0
        out.append(t)
    return np.concatenate(out)


def sum_bound(n_kept, abs_sums):
    return (2.0 * n_kept + 16.0) * gc.EPS53 * abs_sums


def reference(t, mask):
    """Of masked terms (2 N, 28): (math.fsum per column, the bound per column, kept)."""
    ref, mag = fsum_cols(t)
    n = int(np.asarray(mask).sum())
    return ref, sum_bound(n, mag), n


def prefix(t, mask, n):
    """The reference of the first n scan points, from the terms of the whole scan."""
    N = len(t) // 2
    return reference(np.concatenate([t[:n], t[N:N + n]]), np.asarray(mask)[:n])


def tiled(t, mask, n):
    """The reference for a scan that repeats a base scan (row i = base row i % n0), from the masked terms of the base alone, as
    dist_cases.tiled: (sums, bound, count)."""
    n0 = len(t) // 2
    mult = np.bincount(np.arange(n) % n0, minlength=n0).astype(np.float64)
    ref, mag = fsum_cols(np.asarray(t) * np.concatenate([mult, mult])[:, None])
    count = int(round(float(np.sum(mult * np.asarray(mask, dtype=np.float64)))))
    return ref, sum_bound(count, mag), count


def sums(t):
    """Plain float64 sums of terms -> (H, g, e2)."""
    return unpack28(np.sum(t, axis=0))


# ----------------------------------------------------------------------------- a brute-force k-NN for the CPU tests
def knn_brute(points, k):
    """(N, k) neighbour indices within the cloud, ordered by (float64 squared distance, index); padding = N."""
    P = np.asarray(points, dtype=np.float64)
    d2 = ((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=2)
    order = np.lexsort((np.broadcast_to(np.arange(len(P)), d2.shape), d2), axis=1)[:, :k]
    if order.shape[1] < k:
        order = np.concatenate([order, np.full((len(P), k - order.shape[1]), len(P))], axis=1)
    return order


def pca_normals(points, nbr_idx):
    """Unit eigenvector of the smallest eigenvalue of the centred float64 covariance over the neighbours: (N, 3) float32."""
    P = np.asarray(points, dtype=np.float64)
    nb = P[np.asarray(nbr_idx)]
    dd = nb - nb.mean(axis=1, keepdims=True)
    return np.linalg.eigh(np.einsum("nki,nkj->nij", dd, dd))[1][:, :, 0].astype(np.float32)


def gn_loop(target, normals, I_q, g_q, scan, I_p, max_dist, lam, tol, max_iter=30, T0=None):
    """The restated Gauss-Newton loop (brute-force float32 correspondences, plain float64 sums) -> (T, iterations)."""
    from point_cloud_registration_amd.math_tools import plus
    target = np.asarray(target, dtype=np.float32)
    T = np.eye(4) if T0 is None else np.array(T0, dtype=np.float64)
    it = 0
    for it in range(max_iter):
        tp = xform32(T, scan)
        dd = tp[:, None, :] - target[None, :, :]                                # float32
        d2 = (dd[:, :, 0] * dd[:, :, 0] + dd[:, :, 1] * dd[:, :, 1]) + dd[:, :, 2] * dd[:, :, 2]
        j = np.argmin(d2, axis=1)
        mask = np.sqrt(d2[np.arange(len(scan)), j]) < np.float32(max_dist)
        H, g, _ = sums(terms(T, scan, tp, target[j], normals[j], I_q[j], g_q[j], I_p, mask, lam))
        dx = -np.linalg.solve(H, g)
        if np.linalg.norm(dx) < tol:
            break
        T = plus(T, dx)
    return T, it + 1


# ----------------------------------------------------------------------------- the sliding plane
PLANE_SHIFT = np.array([0.03, -0.02, 0.0])


def plane_case():
    """What the feature is for: a flat, textured target and a scan shifted inside the plane ->
    (P (4096, 3) float32, normals, I (4096,), src, I_src)."""
    rng = np.random.default_rng(5)
    P = np.zeros((4096, 3), np.float32)
    P[:, :2] = rng.uniform(-1, 1, (4096, 2))
    normals = np.tile(np.float32([0, 0, 1]), (4096, 1))
    I = field(P)
    sel = rng.choice(4096, 1024, replace=False)
    sel = sel[(np.abs(P[sel, 0]) < 0.8) & (np.abs(P[sel, 1]) < 0.8)]
    src = (P[sel].astype(np.float64) - PLANE_SHIFT).astype(np.float32)
    return P, normals, I, src, I[sel]
