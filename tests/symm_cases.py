"""Float64 NumPy restatement of the symmetric point-to-plane definition (include/pcr.h), with its expression order, shared by
tests/test_symm_api.py and tests/test_gpu_symm.py.  Nothing here touches the GPU.

For scan point p (float32, untransformed) with normal n_p, matched target record (q, n_q) and pose T = (R, t):
d = xform(p) - q formed in float32 and widened; v = R n_p; c = n_q . v; kept iff inside the distance mask and |c| >= min_cos;
s = -1 where c < 0 else +1; m = 0.5 (n_q + s v); r = m . d; J = [m, p x (R^T m)]; terms of the point: triu(J^T J) (21), J r (6),
r r (1).

Bound per entry of the sums: (n_kept + 16) 2^-53 sum |term| -- the summation error of n_kept terms plus a handful of roundings
per term: gicp_cases.sum_bound without the conditioning term of an inverse (there is none here)."""

import numpy as np

import gicp_cases as gc

TRIU = gc.TRIU
fsum_cols = gc.fsum_cols
unpack28 = gc.unpack28


def xform32(T, p):
    """The kernels' float32 transform in their order of operations: ((R0 x + R1 y) + R2 z) + t."""
    T = np.asarray(T, dtype=np.float64).astype(np.float32)
    p = np.asarray(p, dtype=np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)], axis=1)


def rotated(T, n_p):
    """v = R n_p (N, 3) float64: v_i = (R_i0 n_x + R_i1 n_y) + R_i2 n_z."""
    R = np.asarray(T, dtype=np.float64)[:3, :3]
    n = np.asarray(n_p, dtype=np.float32).astype(np.float64)
    return np.stack([(R[i, 0] * n[:, 0] + R[i, 1] * n[:, 1]) + R[i, 2] * n[:, 2] for i in range(3)], axis=1)


def dots(T, n_p, n_q):
    """c = n_q . (R n_p) (N,) float64: (n_q0 v_0 + n_q1 v_1) + n_q2 v_2."""
    v = rotated(T, n_p)
    q = np.asarray(n_q, dtype=np.float32).astype(np.float64)
    return (q[:, 0] * v[:, 0] + q[:, 1] * v[:, 1]) + q[:, 2] * v[:, 2]


def kept(T, n_p, n_q, mask, min_cos=0.0):
    """The correspondences the pass keeps: inside the distance ``mask`` and through the normal gate (NaN: out)."""
    with np.errstate(invalid="ignore"):
        return np.asarray(mask, dtype=bool) & (np.abs(dots(T, n_p, n_q)) >= min_cos)


def terms(T, src, tp, q, n_p, n_q, mask, min_cos=0.0):
    """Per-point terms (N, 28): triu(H) 21, g 6, e2; rows of points that are not kept are zero.  ``tp`` = the float32
    transformed scan, ``q`` / ``n_q`` = the matched float32 target point and its normal for every scan point."""
    R = np.asarray(T, dtype=np.float64)[:3, :3]
    d = (np.asarray(tp, dtype=np.float32) - np.asarray(q, dtype=np.float32)).astype(np.float64)       # float32 subtraction
    p = np.asarray(src, dtype=np.float32).astype(np.float64)
    nq = np.asarray(n_q, dtype=np.float32).astype(np.float64)
    v = rotated(T, n_p)
    c = dots(T, n_p, n_q)
    s = np.where(c < 0, -1.0, 1.0)
    m = 0.5 * (nq + s[:, None] * v)
    r = (m[:, 0] * d[:, 0] + m[:, 1] * d[:, 1]) + m[:, 2] * d[:, 2]
    ra = R[0, 0] * m[:, 0] + R[1, 0] * m[:, 1] + R[2, 0] * m[:, 2]                                     # R^T m
    rb = R[0, 1] * m[:, 0] + R[1, 1] * m[:, 1] + R[2, 1] * m[:, 2]
    rc = R[0, 2] * m[:, 0] + R[1, 2] * m[:, 1] + R[2, 2] * m[:, 2]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    J = np.stack([m[:, 0], m[:, 1], m[:, 2], -z * rb + y * rc, z * ra - x * rc, -y * ra + x * rb], axis=1)
    out = np.concatenate([J[:, TRIU[0]] * J[:, TRIU[1]], J * r[:, None], (r * r)[:, None]], axis=1)
    keep = kept(T, n_p, n_q, mask, min_cos)
    out[~keep] = 0.0
    return out


def sum_bound(n_kept, abs_sums):
    return (n_kept + 16.0) * gc.EPS53 * abs_sums


def reference(t, keep):
    """Of masked terms: (math.fsum per column, the bound per column, kept)."""
    ref, mag = fsum_cols(t)
    n = int(np.asarray(keep).sum())
    return ref, sum_bound(n, mag), n


def tiled(n0_terms, keep, n):
    """The reference for a scan that repeats a base scan (row i = base row i % n0), from the masked terms of the base alone, as
    dist_cases.tiled: (sums, bound, count)."""
    n0 = len(n0_terms)
    mult = np.bincount(np.arange(n) % n0, minlength=n0).astype(np.float64)
    ref, mag = fsum_cols(np.asarray(n0_terms) * mult[:, None])
    count = int(round(float(np.sum(mult * np.asarray(keep, dtype=np.float64)))))
    return ref, sum_bound(count, mag), count


def unit_normals(n, seed=0):
    """Normals (a) of the issue: default_rng(seed).normal(size=(n, 3)), normalised, float32."""
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


CALL_MAX_DIST = 1.0


def call_case(g2):
    """The small pair of the "the call's parameter decides" tests: the first 300 scan points of g2 against its first 400
    targets at g2's pose, correspondences by brute force in float32 as the kernels form them
    -> (target, normals, scan, tp, j, mask).  216 pairs lie inside CALL_MAX_DIST, none within 1e-3 of it, and every nearest
    neighbour leads its runner-up by more than 1e-4 of the squared distance, so masks and indices compare exactly."""
    tgt, nq, src = (np.ascontiguousarray(g2[k][:n]) for k, n in (("target", 400), ("plane_normals", 400), ("source", 300)))
    tp = xform32(g2["T"], src)
    dd = tp[:, None, :] - tgt[None, :, :]                                       # float32
    d2 = np.sort((dd[:, :, 0] * dd[:, :, 0] + dd[:, :, 1] * dd[:, :, 1]) + dd[:, :, 2] * dd[:, :, 2], axis=1)
    dist = np.sqrt(d2[:, 0])
    assert np.min(np.abs(dist - CALL_MAX_DIST)) > 1e-3 and np.min((d2[:, 1] - d2[:, 0]) / d2[:, 1]) > 1e-4
    j = np.argmin(np.sum(dd.astype(np.float64) ** 2, axis=2), axis=1)
    return tgt, nq, src, tp, j, dist < np.float32(CALL_MAX_DIST)


def plane_case(g2):
    """The PlaneICP property on g2: scan normals float32(R^T n_q[nn_idx]) with every second one negated, so that R n_p = +-n_q
    up to float32 rounding and the pass is PlaneICP's -> (n_p, n_q of every target point)."""
    R = g2["T"][:3, :3]
    nq = g2["plane_normals"]
    n_p = (nq[g2["nn_idx"]].astype(np.float64) @ R).astype(np.float32)        # rows of (R^T n)^T = n^T R
    n_p[1::2] = -n_p[1::2]
    return n_p, nq
