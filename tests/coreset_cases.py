"""Inputs and the metric shared by tests/test_gpu_coreset_cases.py and tests/golden/make_golden_coreset.py (g15): the
generator runs the reference on exactly the draws the GPU test makes, so the fixture stores seeds and figures only.

A case is (family, name, seed); ``build(name, seed)`` -> (P_input, u, k, N_target), where P_input is either the pair
(J, r) that create_gn_set turns into P.  Families group the cases that share one bound (10 x the reference's worst
per-row figure over the family's cases)."""

import math

import numpy as np


def rows_of(d):
    return d * (d + 1) // 2 + d + 1


def gn_set_numpy(J, r):
    """create_gn_set restated: J[:, a] J[:, b] for (a, b) in np.triu_indices(D) order, then J[:, a] r, then r r, each
    product rounded once in NumPy's promotion of the two dtypes and then cast to float64.  (M, N), C-contiguous.
    The reference takes the J J products with ``np.einsum``, which ADDS each product to a zeroed output: a product of
    -0.0 (a zero entry times a negative one, or a negative product that underflows) comes out as +0.0 there, while
    J * r and r ** 2 are plain products and keep the sign -- hence the ``+ 0`` on the first rows only."""
    d = J.shape[1]
    with np.errstate(over="ignore", under="ignore"):
        rows = [J[:, a] * J[:, b] + J.dtype.type(0) for a, b in zip(*np.triu_indices(d))]
        rows += [J[:, a] * r for a in range(d)]
        rows.append(r * r)
    return np.ascontiguousarray(np.stack([x.astype(np.float64) for x in rows]))


def per_row_error(P, u, w, idx):
    """max over rows m of |sum_i u_i P[m, i] - sum_j w_j P[m, idx_j]| / sum_i u_i |P[m, i]|, the three sums taken with
    math.fsum over the float64 products (exactly rounded: the check adds no summation error of its own).
    -> (worst, exact): ``exact`` is False when a row whose denominator is 0 does not match exactly."""
    worst, exact = 0.0, True
    for row in P:
        full = math.fsum(u * row)
        sel = math.fsum(w * row[idx])
        den = math.fsum(u * np.abs(row))
        if den == 0.0:
            exact = exact and full == sel
        else:
            worst = max(worst, abs(full - sel) / den)
    return worst, exact


def special_values(seed=300, n=192, d=6):
    """float32 (J, r) whose float32 products overflow to +-inf, underflow to subnormals or to +-0.0, while the same
    products are finite and normal in float64: entries around +-1e20 and +-1e-25, subnormal inputs, exact zeros of
    either sign and ordinary values.  Every entry is finite, so no product is NaN (there is no inf x 0)."""
    rng = np.random.default_rng(seed)
    pool = np.array([1e20, 3e19, 2.5e18, 1e-25, 7e-23, 4e-20, 1e-40, 3e-42, 1.5, 0.37, 0.0], dtype=np.float32)
    pool = np.concatenate([pool, -pool])
    J = pool[rng.integers(0, len(pool), (n, d))]
    r = pool[rng.integers(0, len(pool), n)]
    return np.ascontiguousarray(J), np.ascontiguousarray(r)


TYPE_PAIRS = [(np.float64, np.float64), (np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32)]


def _planar(rng, n, offset, normal_noise):
    """PlaneICP's rows on a plane z = const: n = (0, 0, 1) (perturbed by N(0, normal_noise) and renormalised when
    normal_noise > 0), J = [n, p x n], p ~ U(-30, 30)^3 + offset, r ~ N(0, 0.02)."""
    p = rng.uniform(-30.0, 30.0, (n, 3)) + np.asarray(offset, dtype=np.float64)
    nrm = np.tile([0.0, 0.0, 1.0], (n, 1))
    if normal_noise > 0:
        nrm = nrm + rng.normal(0.0, normal_noise, (n, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    r = rng.normal(0.0, 0.02, n)
    return np.hstack([nrm, np.cross(p, nrm)]), r


def build(name, seed):
    """-> (J, r, u, k, N_target) of one case; default_rng(seed) draws J, then r, then whatever else the case needs."""
    rng = np.random.default_rng(seed)
    if name.startswith("D"):                               # B.1: every D, k = 2 (M + 1), N_target = 2 k, N = 40 k
        d = int(name[1:])
        k = 2 * (rows_of(d) + 1)
        n = 40 * k
        return rng.standard_normal((n, d)), rng.standard_normal(n), np.ones(n), k, 2 * k
    if name == "uneven_blocks":                            # B.2: chunks of ~6250 members cut into ~7 blocks of unequal length
        n = 100_003
        J, r = rng.standard_normal((n, 3)), rng.standard_normal(n)
        return J, r, rng.uniform(0.5, 2.0, n), 16, 32
    if name == "k_above_level":                            # B.3: k = 400 > N = 200
        return rng.standard_normal((200, 6)), rng.standard_normal(200), np.ones(200), 400, 128
    if name == "n_sub_branch":                             # B.4: n_sub = N_target / max_chunk away from N = 129
        return rng.standard_normal((300, 6)), rng.standard_normal(300), np.ones(300), 64, 256
    n, d, k, nt = 20_000, 6, 64, 128                       # C
    J, r, u = rng.standard_normal((n, d)), rng.standard_normal(n), np.ones(n)
    if name == "weights_1e6":
        u = 10.0 ** rng.uniform(-6.0, 6.0, n)
    elif name == "weights_1e3":
        u = 10.0 ** rng.uniform(-3.0, 3.0, n)
    elif name == "ill_scaled":
        J[:, 3:] *= 1e3
        r *= 1e-2
    elif name == "zero_column":
        J[:, 2] = 0.0
    elif name == "equal_columns":
        J[:, 4] = J[:, 1]
    elif name == "duplicated_rows":
        pick = rng.integers(0, 50, n)
        J, r = J[pick], r[pick]
    elif name == "identical_rows":
        J, r = np.tile(J[0], (n, 1)), np.full(n, r[0])
    elif name == "planar_exact":
        J, r = _planar(rng, n, (0.0, 0.0, 0.0), 0.0)
    elif name == "planar_offset":
        J, r = _planar(rng, n, (1000.0, -2000.0, 50.0), 0.01)
    elif name == "float32":
        J, r = J.astype(np.float32), r.astype(np.float32)
    else:
        raise KeyError(name)
    return J, r, u, k, nt


# (family, case name, seed).  Every family has a bound of its own: 10 x the reference's worst figure over its cases.
CASES = [("every_D", f"D{d}", 200 + d) for d in range(1, 13)]
CASES += [("structure", "uneven_blocks", 220), ("structure", "k_above_level", 221), ("structure", "n_sub_branch", 222)]
CASES += [(fam, name, seed) for fam, name, base in (
    ("weights", "weights_1e6", 230), ("weights", "weights_1e3", 232), ("ill_scaled", "ill_scaled", 234),
    ("rank_deficient", "zero_column", 236), ("rank_deficient", "equal_columns", 238),
    ("repeated_rows", "duplicated_rows", 240), ("repeated_rows", "identical_rows", 242),
    ("planar_exact", "planar_exact", 244), ("planar_offset", "planar_offset", 246), ("float32", "float32", 248))
    for seed in (base, base + 1)]
CASE_IDS = [f"{name}-seed{seed}" for _, name, seed in CASES]
FAMILIES = sorted({fam for fam, _, _ in CASES})
