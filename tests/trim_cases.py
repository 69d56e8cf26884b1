"""Float64 NumPy restatement of the adaptive pass of include/pcr.h -- the key, the rank rule, tau, the trim, the scale taken
from tau and the limit for c -> 0 -- and of the Gauss-Newton loop over it on the end-to-end case of tests/robust_cases.py.
Shared by tests/test_trim_cases.py and tests/test_gpu_trim.py.  Nothing here touches the GPU.

One pass, with s (N, M) the squared residuals of pcr_*_residuals (M = 1; ColoredICP 2), inf where a point has no correspondence:
  key    kappa = s[:, 0] (+ s[:, 1]: one addition, geometric row first)
  rank   m = the number of kappa < inf;  k = max(1, floor(q * m)), the product once in float64;  m = 0: nothing
  tau    the k-th smallest kappa;  n_le = the number of kappa <= tau (>= k: ties are all in)
  trim   weight 1 where kappa <= tau, else 0 -- one decision per correspondence, both rows of ColoredICP
  huber, cauchy, tukey, gm    c = factor * sqrt(tau), c2 = c * c;  the weight of robust_cases.weight per ROW at that c -- and where
         c2 is not > 0 the limit of every kernel for c -> 0: 1 where s == 0, else 0
  stats  (tau, c, n_le, k), c = 0 for a trim;  (inf, 0, 0, 0) for m = 0

ADAPTIVE_ERRORS records |t - t_true| of the restated loop on the case (1024 scan points, 30 % of them moved by 0.3 m, max_dist =
1) for a trim at ratio 0.6 -- deliberately BELOW the inlier share of 0.7: the kept set then holds inliers only -- and for Tukey at
the median with factor 3; tests/test_trim_cases.py::test_end_to_end prints them.  They are the reference of the GPU test, not
the code under test."""

import numpy as np

import robust_cases as rc

KINDS = rc.KINDS + ("trim",)
KIND_ID = {"huber": 1, "cauchy": 2, "tukey": 3, "gm": 4, "trim": 5}
FAMILIES = ("symm", "color", "gicp", "vgicp")

E2E_TRIM = ("trim", 0.6, 1.0)
E2E_TUKEY = ("tukey", 0.5, 3.0)
# |t - t_true| of the restated loop: (trim at 0.6, Tukey at q = 0.5 with factor 3); plain and fixed Cauchy: rc.E2E_ERRORS
ADAPTIVE_ERRORS = {"symm": (1.923e-4, 1.669e-4), "color": (1.956e-4, 1.780e-4), "gicp": (1.726e-4, 1.485e-4), "vgicp": (9.896e-4, 7.241e-4)}


def rank(q, m):
    """k of the rule; 0 for m = 0."""
    return max(1, int(np.floor(np.float64(q) * np.float64(m)))) if m else 0


def key(s):
    """s (N, M) or (N,) -> kappa (N,): the rows added in order."""
    s = np.asarray(s, dtype=np.float64)
    if s.ndim == 1:
        return s.copy()
    kappa = s[:, 0].copy()
    for r in range(1, s.shape[1]):
        kappa = kappa + s[:, r]
    return kappa


def threshold(kappa, q):
    """-> (tau, k, m, n_le); (inf, 0, 0, 0) for m = 0.  NaN counts as outside, as inf does."""
    kappa = np.asarray(kappa, dtype=np.float64)
    f = np.sort(kappa[kappa < np.inf])
    m = len(f)
    if m == 0:
        return np.inf, 0, 0, 0
    k = rank(q, m)
    tau = float(f[k - 1])
    return tau, k, m, int(np.sum(kappa <= tau))


def scale(tau, factor):
    """-> (c, c2), each taken once in float64."""
    with np.errstate(invalid="ignore"):
        c = np.float64(factor) * np.sqrt(np.float64(tau))
    return float(c), float(c * c)


def weights(kind, s, q, factor=1.0):
    """s (N, M) -> (w (N, M), stats (4,), m)."""
    s = np.asarray(s, dtype=np.float64)
    s = s[:, None] if s.ndim == 1 else s
    kappa = key(s)
    tau, k, m, n_le = threshold(kappa, q)
    if m == 0:
        return np.zeros_like(s), np.array([np.inf, 0.0, 0.0, 0.0]), 0
    if kind == "trim":
        w = np.repeat((kappa <= tau)[:, None], s.shape[1], axis=1).astype(np.float64)
        c = 0.0
    else:
        c, c2 = scale(tau, factor)
        if c2 > 0.0:
            w = rc.weight(kind, s, c)
        else:
            w = np.where(s == 0.0, 1.0, 0.0)
    return w, np.array([tau, c, float(n_le), float(k)]), m


# ----------------------------------------------------------------------------- the end-to-end case
def e2e_pass(family, case, T, kind, q, factor=1.0):
    """The weighted terms of one adaptive pass of ``family`` over the case at T -> (terms (M N, 28), stats).  The unweighted
    terms are rc.e2e_terms(family, case, T, None, 1.0): a row outside the gates is all zeros there (its weight was 0), and a row
    inside is not -- its Jacobian is not zero -- which is how the correspondences are told here; s is the last column."""
    t = rc.e2e_terms(family, case, T, None, 1.0)
    M = 2 if family == "color" else 1
    N = len(t) // M
    inside = np.any(np.any(t != 0.0, axis=1).reshape(M, N), axis=0)
    s = np.where(inside[None, :], t[:, 27].reshape(M, N), np.inf).T
    w, stats, _ = weights(kind, s, q, factor)
    return t * w.T.ravel()[:, None], stats


def gn_loop(family, case, kind, q, factor=1.0, max_iter=30, tol=rc.E2E_TOL):
    """rc.gn_loop over the adaptive pass -> (T, iterations)."""
    import gicp_cases as gc
    from point_cloud_registration_amd.math_tools import plus
    T, it = np.eye(4), 0
    for it in range(max_iter):
        H, g, _ = gc.unpack28(np.sum(e2e_pass(family, case, T, kind, q, factor)[0], axis=0))
        dx = -np.linalg.solve(H, g)
        if np.linalg.norm(dx) < tol:
            break
        T = plus(T, dx)
    return T, it + 1
