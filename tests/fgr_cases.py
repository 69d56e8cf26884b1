"""The fast-global-registration definitions of include/pcr.h restated in NumPy and plain Python floats, and the cases the
tests share: the weights, the 29 terms per match, their sums (math.fsum per column, with the sum of the magnitudes), the
schedule of mu, the step (LU with partial pivoting as gn_solve6, the sin / cos of gn_math.h, the left update) and the loop.
NumPy neither fuses nor reorders, so every array expression below rounds as the header writes it; the scalar code uses Python
floats (IEEE doubles).  The tuple multiplicities come from tests/ransac_cases.py's sampler and validity rule."""
import functools
import math

import numpy as np

import ransac_cases as rc

TRACE = 46


# ---- one pass ---------------------------------------------------------------------------------------------------------------
def residuals(src, dst, T):
    """-> x (M, 3), r (M, 3), r2 (M,): float64 over the widened float32 points."""
    p, q = np.asarray(src, np.float32).astype(np.float64), np.asarray(dst, np.float32).astype(np.float64)
    T = np.asarray(T, np.float64)
    x = np.stack([((T[i, 0] * p[:, 0] + T[i, 1] * p[:, 1]) + T[i, 2] * p[:, 2]) + T[i, 3] for i in range(3)], axis=1)
    r = x - q
    r2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    return x, r, r2


def weights(src, dst, T, mu):
    """l * l per match (the multiplicity takes no part)."""
    _, _, r2 = residuals(src, dst, T)
    mu = np.float64(mu)
    l = mu / (mu + r2)
    return l * l


def terms(src, dst, T, mu, mult=None):
    """-> (M, 29): the 29 terms of every match, each w times its bracket."""
    x, r, r2 = residuals(src, dst, T)
    mu = np.float64(mu)
    l = mu / (mu + r2)
    c = np.ones(len(x)) if mult is None else np.asarray(mult).astype(np.float64)
    w = c * (l * l)
    x0, x1, x2 = x[:, 0], x[:, 1], x[:, 2]
    r0, r1, rr2 = r[:, 0], r[:, 1], r[:, 2]
    z = np.zeros(len(x))
    cols = [w, z, z, z, w * x2, w * -x1,
            w, z, w * -x2, z, w * x0,
            w, w * x1, w * -x0, z,
            w * (x1 * x1 + x2 * x2), w * -(x0 * x1), w * -(x0 * x2),
            w * (x0 * x0 + x2 * x2), w * -(x1 * x2),
            w * (x0 * x0 + x1 * x1),
            w * r0, w * r1, w * rr2,
            w * (x1 * rr2 - x2 * r1), w * (x2 * r0 - x0 * rr2), w * (x0 * r1 - x1 * r0),
            w * r2, w]
    return np.stack(cols, axis=1)


def sums(src, dst, T, mu, mult=None):
    """-> (sums (29,), the exactly rounded sum per column; mags (29,), the sum of the magnitudes)."""
    P = terms(src, dst, T, mu, mult)
    return np.array([math.fsum(P[:, k]) for k in range(29)]), np.array([math.fsum(np.abs(P[:, k])) for k in range(29)])


# ---- the step ---------------------------------------------------------------------------------------------------------------
def schedule(mu, it, mu_min, division, period):
    """mu after iteration it."""
    if (it + 1) % period == 0 and mu > mu_min:
        return max(mu / division, mu_min)
    return mu


def solve6(H, g):
    """gn_solve6: LU with partial pivoting (the first of the largest), an exactly zero pivot = singular -> x or None."""
    A = [[float(H[i][j]) for j in range(6)] + [float(g[i])] for i in range(6)]
    for c in range(6):
        piv, pmax = c, abs(A[c][c])
        for r in range(c + 1, 6):
            if abs(A[r][c]) > pmax:
                pmax, piv = abs(A[r][c]), r
        if pmax == 0.0:
            return None
        A[c], A[piv] = A[piv], A[c]
        for r in range(c + 1, 6):
            f = A[r][c] / A[c][c]
            for j in range(c, 7):
                A[r][j] -= f * A[c][j]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        v = A[i][6]
        for j in range(i + 1, 6):
            v -= A[i][j] * x[j]
        x[i] = v / A[i][i]
    return x


def sincos(x):
    """gn_sincos of csrc/gn_math.h: Cody-Waite by pi/2 in three parts and the fdlibm kernel polynomials."""
    k = math.floor(x * 6.36619772367581382433e-01 + 0.5)
    r = x - k * 1.57079632673412561417e+00
    r = r - k * 6.07710050630396597660e-11
    r = r - k * 2.02226624871116645580e-21
    z = r * r
    ps = -1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (
        2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))))
    pc = 4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 + z * (
        -2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))))
    s0 = r + r * z * ps
    c0 = (1.0 - 0.5 * z) + z * z * pc
    q = int(k - 4.0 * math.floor(k * 0.25))
    return (s0, c0, -s0, -c0)[q], (c0, -s0, -c0, s0)[q]


def exp_so3(w):
    """gn_exp_so3: I + skew(w) when w.w <= 1e-5, Rodrigues otherwise -> 9 floats, row-major."""
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    W = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    if th2 <= 1e-5:
        R = list(W)
    else:
        th = math.sqrt(th2)
        sn, cs = sincos(th)
        omc = 1.0 - cs
        K = [v / th for v in W]
        R = [0.0] * 9
        for i in range(3):
            for j in range(3):
                kk = 0.0
                for k in range(3):
                    kk += K[3 * i + k] * K[3 * k + j]
                R[3 * i + j] = sn * K[3 * i + j] + omc * kk
    R[0] += 1
    R[4] += 1
    R[8] += 1
    return R


def lplus(T, dx):
    """gn_se3_lplus: [exp(dx[3:]), dx[:3]; 0 1] @ T, every entry the sum over k = 0 .. 3 in order."""
    dR = exp_so3(dx[3:])
    D = [dR[0], dR[1], dR[2], dx[0], dR[3], dR[4], dR[5], dx[1], dR[6], dR[7], dR[8], dx[2], 0.0, 0.0, 0.0, 1.0]
    Tl = [float(v) for v in np.asarray(T, np.float64).reshape(16)]
    out = np.empty(16)
    for i in range(4):
        for j in range(4):
            v = 0.0
            for k in range(4):
                v += D[4 * i + k] * Tl[4 * k + j]
            out[4 * i + j] = v
    return out.reshape(4, 4)


def step(o, T, mu, mu_min, tol):
    """One step from the 29 sums -> (status: 0 stepped, 1 converged, 2 singular; T after it)."""
    H = [[0.0] * 6 for _ in range(6)]
    p = 0
    for i in range(6):
        for j in range(i, 6):
            H[i][j] = H[j][i] = float(o[p])
            p += 1
    x = solve6(H, [float(v) for v in o[21:27]])
    if x is None:
        return 2, np.asarray(T, np.float64)
    dx = [-v for v in x]
    nrm = 0.0
    for v in dx:
        nrm += v * v
    if tol > 0 and mu == mu_min and math.sqrt(nrm) < tol:
        return 1, np.asarray(T, np.float64)
    return 0, lplus(T, dx)


def fgr_numpy(src, dst, T_init, mu0, mu_min, division, period, max_iter, tol=0.0, mult=None, gpu_sums=None):
    """pcr_fgr_pose restated -> dict(T, iterations, status, mu, weights, trace (max_iter, 46)).  ``gpu_sums(T, mu)``: take the
    sums of every pass from there instead of math.fsum (the loop is then the host step over the device's own sums)."""
    T, mu = np.array(T_init, np.float64), float(mu0)
    trace = np.zeros((max_iter, TRACE))
    it, status = 0, 0
    while it < max_iter:
        o = sums(src, dst, T, mu, mult)[0] if gpu_sums is None else gpu_sums(T, mu)
        trace[it, :16], trace[it, 16:45], trace[it, 45] = T.reshape(16), o, mu
        rcode, T = step(o, T, mu, mu_min, tol)
        it += 1
        if rcode:
            status = rcode
            break
        mu = schedule(mu, it - 1, mu_min, division, period)
    return {"T": T, "iterations": it, "status": status, "mu": mu, "weights": weights(src, dst, T, mu), "trace": trace}


# ---- the tuple test ---------------------------------------------------------------------------------------------------------
def tuple_mult(src, dst, n_tuples, seed, tuple_scale, min_edge):
    """-> (mult (M,) int32, n_valid): the sampler and the validity rule of RANSAC's hypotheses."""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    m = len(src)
    mult = np.zeros(m, np.int32)
    if m < 3 or n_tuples == 0:
        return mult, 0
    S = rc.samples(seed, n_tuples, m)
    valid, _ = rc.fit(src, dst, S, tuple_scale, min_edge)
    np.add.at(mult, S[valid].reshape(-1), 1)
    return mult, int(valid.sum())


def tuple_mult_loop(src, dst, n_tuples, seed, tuple_scale, min_edge):
    """The same by a loop over the tuples, one at a time, in plain Python floats."""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    m = len(src)
    mult, n_valid = np.zeros(m, np.int32), 0
    if m < 3:
        return mult, 0
    s = float(np.float32(tuple_scale))
    e = float(np.float32(min_edge))
    s2, e2 = s * s, e * e

    def sub(a, b):
        return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def spans(p):
        e1, w = sub(p[1], p[0]), cross(sub(p[1], p[0]), sub(p[2], p[0]))
        return dot(e1, e1) > 0 and dot(w, w) > 0
    for h in range(n_tuples):
        c = rc.sample(seed, h, m)
        P = [[float(v) for v in src[k]] for k in c]
        Q = [[float(v) for v in dst[k]] for k in c]
        ok = True
        for i, j in ((0, 1), (1, 2), (2, 0)):
            a2, b2 = dot(sub(P[i], P[j]), sub(P[i], P[j])), dot(sub(Q[i], Q[j]), sub(Q[i], Q[j]))
            ok = ok and a2 >= s2 * b2 and b2 >= s2 * a2 and a2 >= e2 and b2 >= e2
        if ok and spans(P) and spans(Q):
            n_valid += 1
            for k in c:
                mult[k] += 1
    return mult, n_valid


def fgr_pose_numpy(src, dst, max_dist, mu0, n_tuples, seed=0, tuple_scale=0.95, min_edge=0.0, refine_rounds=5):
    """fgr_pose restated over paired rows: the tuple test, the loop from the identity, ransac_pose's refinement -> (T, info)."""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    m = len(src)
    mult, n_valid = tuple_mult(src, dst, n_tuples, seed, tuple_scale, min_edge)
    T, count, mask, rmse = np.eye(4), 0, np.zeros(m, bool), np.inf
    res = {"iterations": 0, "status": 0, "mu": mu0, "weights": np.ones(m)}
    if np.count_nonzero(mult) >= 3:
        res = fgr_numpy(src, dst, np.eye(4), mu0, max_dist * max_dist, mult=mult, **SCHEDULE)

        def sc(Tc):
            c, k = rc.score(src, dst, rc.pose12(Tc)[None], max_dist)
            return int(c[0]), k[0]
        T = rc.T_of(rc.pose12(res["T"]))
        count, mask = sc(T)
        rmse = rc._rmse(T, src, dst, mask)
        for _ in range(refine_rounds):
            if count < 3:
                break
            T2 = rc.T_of(rc.pose12(rc.kabsch(src[mask], dst[mask])))
            c2, m2 = sc(T2)
            r2 = rc._rmse(T2, src, dst, m2)
            if not (c2 > count or (c2 == count and r2 < rmse)):
                break
            T, count, mask, rmse = T2, c2, m2, r2
        U, _, Vt = np.linalg.svd(T[:3, :3])
        T = T.copy()
        T[:3, :3] = U @ np.diag([1.0, 1.0, 1.0 if np.linalg.det(U @ Vt) >= 0 else -1.0]) @ Vt
    return T, {"inliers": mask, "count": count, "fitness": count / m if m else 0.0, "rmse": rmse, "mult": mult, "n_valid": n_valid,
               "iterations": res["iterations"], "status": res["status"], "mu": res["mu"], "weights": res["weights"]}


# ---- shared cases -----------------------------------------------------------------------------------------------------------
MAX_DIST = 0.05          # five times the noise of the cases
CASES = {"A": dict(m=300, outliers=0.5), "B": dict(m=3000, outliers=0.8)}
SCHEDULE = dict(division=1.4, period=4, max_iter=64)


@functools.lru_cache(maxsize=None)
def case(name, seed):
    """Uniform points in a 40 m box and their copy under a rotation vector of up to 1.2 per axis and a translation of up to
    10 m, noise 0.01 m on the copy, a share of the matches replaced by uniform points.
    -> dict(src, dst (float32), T_true, inlier (M,) bool, mu0 = D^2); shared and left unchanged."""
    from point_cloud_registration_amd.math_tools import expSO3
    c = CASES[name]
    m = c["m"]
    rng = np.random.default_rng([seed, m])
    src = rng.uniform(-20, 20, (m, 3))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = expSO3(rng.uniform(-1.2, 1.2, 3)), rng.uniform(-10, 10, 3)
    dst = src @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.01, (m, 3))
    out = np.zeros(m, bool)
    out[rng.permutation(m)[:int(round(c["outliers"] * m))]] = True
    dst[out] = rng.uniform(-20, 20, (int(out.sum()), 3)) + T[:3, 3]
    src, dst = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(dst, np.float32)
    for a in (src, dst):
        a.setflags(write=False)
    return {"src": src, "dst": dst, "T_true": T, "inlier": ~out, "mu0": mu0_of(src, dst)}


def mu0_of(src, dst):
    """D^2, D the larger bounding-box diagonal of the two point sets (float64 over the float32 points)."""
    def diag(a):
        return float(np.linalg.norm(a.max(axis=0).astype(np.float64) - a.min(axis=0).astype(np.float64)))
    D = max(diag(src), diag(dst))
    return D * D


@functools.lru_cache(maxsize=None)
def reference(name, seed):
    """fgr_numpy on a case from the identity, no tuple filter: computed once per key, shared and left unchanged."""
    c = case(name, seed)
    return fgr_numpy(c["src"], c["dst"], np.eye(4), c["mu0"], MAX_DIST * MAX_DIST, **SCHEDULE)


def pose_error(T, T_true):
    """-> (rotation error in degrees, translation error in metres)."""
    dR = T[:3, :3] @ T_true[:3, :3].T
    ang = math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(dR) - 1.0) / 2.0))))
    return ang, float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))
