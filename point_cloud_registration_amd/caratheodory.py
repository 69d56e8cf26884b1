"""Gauss-Newton coresets: ``create_gn_set`` and ``fast_caratheodory`` (the reference's ``caratheodory.py:62-138``).

K. Koide, "Exact Point Cloud Downsampling for Fast and Accurate Global Trajectory Optimization", arXiv 2307.02948: the
per-correspondence rows P = [upper triangle of J^T J, J r, r^2] of a Gauss-Newton problem are reduced to at most
``N_target`` weighted rows whose weighted sums reproduce H, g and e2 of the full set up to rounding.

The O(N M) work -- the products of ``create_gn_set`` and the weighted chunk sums of every level of ``fast_caratheodory`` --
runs in HIP kernels (``csrc/coreset.hip``); the Caratheodory elimination of each level's k chunk means, whose cost does not
grow with N, runs on the host inside the library.  There is no CPU path: without a GPU the library's error surfaces.

Differences from the reference, all on inputs it cannot handle: ``k <= M + 1`` and ``N_target < M + 1`` (the reference does
not finish: its ``caratheodory()`` hands back the same chunk again, ``caratheodory.py:42-43``), non-finite or non-positive
``u``, non-finite ``P``, shapes that disagree and row counts that are not D (D + 1) / 2 + D + 1 for D in 1..12 raise
``ValueError``.  The null vector of each elimination step comes from a pivoted QR instead of an SVD, so the selected points
differ from the reference's; what holds is what the reference's test checks: ``idx`` ascending, ``w > 0``,
``len(w) <= N_target`` and sum w P[:, idx] = sum u P.
"""

import operator

import numpy as np

from . import _capi

MAX_D = 12          # M = D (D + 1) / 2 + D + 1 <= 91


def _rows(d):
    return d * (d + 1) // 2 + d + 1


def _dim_of_rows(m):
    for d in range(1, MAX_D + 1):
        if _rows(d) == m:
            return d
    return None


def _float_array(a):
    """float32 / float64 as given (the products are rounded in NumPy's promotion of these), anything else as float64."""
    a = np.asarray(a)
    if a.dtype != np.float32 and a.dtype != np.float64:
        a = a.astype(np.float64)
    return np.ascontiguousarray(a)


def create_gn_set(J, r):
    """(N, D) Jacobian and (N,) residuals -> P (M, N) float64, M = D (D + 1) / 2 + D + 1 (caratheodory.py:118-138):
    J[:, a] J[:, b] for (a, b) in ``np.triu_indices(D)`` order, then J[:, d] r, then r^2 -- bit for bit the reference's
    values for float32, float64 and mixed inputs, including the +0.0 that ``np.einsum`` leaves where a J J product is -0.0.
    The result is C-contiguous (the reference returns a transposed view)."""
    J, r = _float_array(J), _float_array(r)
    if J.ndim != 2:
        raise ValueError(f"J must have shape (N, D), got {J.shape}")
    n, d = J.shape
    if r.shape != (n,):
        raise ValueError(f"r must have shape ({n},), got {r.shape}")
    if not 1 <= d <= MAX_D:
        raise ValueError(f"D must be in [1, {MAX_D}], got {d}")
    if n == 0:
        return np.empty((_rows(d), 0))
    return _capi.gn_set(_capi.get_context(), J, r)


def fast_caratheodory(P, u, k, N_target):
    """Coreset of the weighted columns of P (caratheodory.py:62-116) -> (P_sel, w, idx): ``idx`` strictly ascending,
    ``w > 0``, ``P_sel = P[:, idx]``, at most ``N_target`` columns, and sum w P_sel = sum u P up to rounding.
    N <= N_target returns ``(P, u, arange(N))``."""
    P, u = np.asarray(P), np.asarray(u)
    k, N_target = operator.index(k), operator.index(N_target)
    if P.ndim != 2:
        raise ValueError(f"P must have shape (M, N), got {P.shape}")
    m, n = P.shape
    if _dim_of_rows(m) is None:
        raise ValueError(f"P must have M = D (D + 1) / 2 + D + 1 rows for some D in [1, {MAX_D}], got {m}")
    if u.shape != (n,):
        raise ValueError(f"u must have shape ({n},), got {u.shape}")
    if k <= m + 1:
        raise ValueError(f"k must exceed M + 1 = {m + 1}, got {k}")
    if N_target < m + 1:
        raise ValueError(f"N_target must be at least M + 1 = {m + 1}, got {N_target}")
    P64 = np.ascontiguousarray(P, dtype=np.float64)
    u64 = np.ascontiguousarray(u, dtype=np.float64)
    if n and not (np.isfinite(u64).all() and (u64 > 0).all()):
        raise ValueError("u must be finite and positive")
    # one multi-threaded pass: a NaN or an infinity in a row makes its sum non-finite (so would an overflowing row sum,
    # which the library refuses as well)
    if n and not np.isfinite(P64 @ np.ones(n)).all():
        raise ValueError("P must be finite (and its row sums must not overflow)")
    if n <= N_target:
        return P, u, np.arange(n)
    return _capi.coreset(_capi.get_context(), P64, u64, k, N_target)
