"""Cases of the distribution pass behind GICP and VGICP (csrc/match_pass.h), shared by tests/test_dist_cases.py and
tests/test_gpu_dist_pass.py: the gate boundary and the pose space of tests/pass_cases.py with covariances on both sides, the
det == 0 rule of the weight, and scans large enough for every slot of a lane and a second trip of its loop to carry live
points.  Plain NumPy plus the CPU oracle, deterministic, no GPU; every cloud but the base scans comes from pass_cases.py.

The restatement is gicp_cases.terms / vgicp_cases.terms with ONE change: the weight M = (Cq + R Cp R^T)^-1 is taken by
oracle.calc_icov -- the oracle's restatement of voxel.py:69-102, adjugate / determinant with a determinant of exactly 0
replaced by 1e6 -- where those use numpy.linalg.inv, which cannot represent that rule.  On a regular sum the two agree to
rounding (tests/test_dist_cases.py); on the exact degenerate sets below the summed matrix is exact in float64 in any order of
evaluation, so the restated weight is the kernel's own arithmetic."""

import numpy as np

import gicp_cases as gc
import pass_cases as pc

GICP_W, VGICP_W = 3, 2                     # points per lane in flight (gicp.hip, vgicp.hip)
BASE_N0, BASE_GATE = 2000, 1.0


def _orc():
    from oracle import oracle
    return oracle


# ----------------------------------------------------------------------------- the restatement
def summed(T, Cp6, Cq6):
    """Cq + R Cp R^T (N, 3, 3) float64 in the order csrc/gicp_weight.h states for it: B = R Cp with every entry
    (R_i0 Cp_0j + R_i1 Cp_1j) + R_i2 Cp_2j, then the upper triangle of B R^T the same way, mirrored, then Cq + that.  The
    library is built without contraction, so these are its roundings.  (The order matters to the bound: adjugate / determinant
    cancels where numpy.linalg.inv does not -- on sums of condition 5e5 it lies up to 1.3e-8 relative from the inverse -- and
    amplifies a last-place difference of the summed matrix alike, far beyond the 16 / eps_min roundings of sum_bound.)"""
    R = np.asarray(T, dtype=np.float64)[:3, :3]
    Cp = gc.full3(Cp6)
    B = np.empty_like(Cp)
    for i in range(3):
        for j in range(3):
            B[:, i, j] = (R[i, 0] * Cp[:, 0, j] + R[i, 1] * Cp[:, 1, j]) + R[i, 2] * Cp[:, 2, j]
    S = np.empty_like(Cp)
    for i in range(3):
        for j in range(i, 3):
            S[:, i, j] = (B[:, i, 0] * R[j, 0] + B[:, i, 1] * R[j, 1]) + B[:, i, 2] * R[j, 2]
            S[:, j, i] = S[:, i, j]
    return gc.full3(Cq6) + S


def weights_closed(T, Cp6, Cq6):
    """(M (N, 3, 3) = calc_icov(Cq + R Cp R^T), smallest eigenvalue of every summed matrix (N,)), float64."""
    S = summed(T, Cp6, Cq6)
    return _orc().calc_icov(S), np.linalg.eigvalsh(S)[:, 0]


def terms_all(T, src, tp, q, Cp6, Cq6, residual):
    """Per-point terms (N, 28) of EVERY point -- triu(H) 21, g 6, e2 -- and the smallest eigenvalue of every summed matrix.
    ``tp`` = the float32 transformed scan, ``q`` = the matched target element of every scan point, ``Cq6`` its covariance;
    ``residual``: "f32" (GICP: tp - q formed in float32 and widened) or "f64" (VGICP: widened, then subtracted)."""
    if residual == "f32":
        d = (np.asarray(tp, dtype=np.float32) - np.asarray(q, dtype=np.float32)).astype(np.float64)
    else:
        d = np.asarray(tp, dtype=np.float32).astype(np.float64) - np.asarray(q, dtype=np.float64)
    J = gc.jacobians(T, src)
    M, lmin = weights_closed(T, Cp6, Cq6)
    H = np.einsum("nij,nik,nkl->njl", J, M, J)
    g = np.einsum("nij,nik,nk->nj", J, M, d)
    e2 = np.einsum("ni,nij,nj->n", d, M, d)
    return np.concatenate([H[:, gc.TRIU[0], gc.TRIU[1]], g, e2[:, None]], axis=1), lmin


def terms_closed(T, src, tp, q, Cp6, Cq6, mask, residual="f32"):
    """gicp_cases.terms (``residual="f64"``: vgicp_cases.terms) with the weight of ``weights_closed``: rows of points outside
    ``mask`` are zero.  Returns (terms, eps_min over the masked points)."""
    t, lmin = terms_all(T, src, tp, q, Cp6, Cq6, residual)
    mask = np.asarray(mask, dtype=bool)
    t *= mask.astype(np.float64)[:, None]
    return t, float(lmin[mask].min()) if np.any(mask) else 1.0


def reference(terms, lmin, mask, exact=False):
    """Of unmasked ``terms``: (math.fsum of the kept rows per column, the bound per column, kept).  ``exact``: the weight is
    exact (the degenerate sets), so the conditioning term of gicp_cases.sum_bound is 1: (kept + 16) 2^-53 sum |term|."""
    mask = np.asarray(mask, dtype=bool)
    ref, mag = gc.fsum_cols(terms[mask])
    kept = int(mask.sum())
    eps_min = 1.0 if exact or kept == 0 else float(lmin[mask].min())
    return ref, gc.sum_bound(kept, eps_min, mag), kept


def tiled(n0_terms, mask, n, n0, eps_min):
    """The reference for a scan that repeats a base scan of ``n0`` points (row i of the scan = base row i % n0), from the
    masked terms of the base alone: (sums, bound, count)."""
    m = np.bincount(np.arange(n) % n0, minlength=n0).astype(np.float64)
    ref, mag = gc.fsum_cols(np.asarray(n0_terms) * m[:, None])
    count = int(round(float(np.sum(m * np.asarray(mask, dtype=np.float64)))))
    return ref, gc.sum_bound(count, eps_min, mag), count


# ----------------------------------------------------------------------------- covariance sets
ZERO6 = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
DISC6 = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)     # diag(1, 1, 0): unchanged by every rotation about z, Cq + R Cp R^T = diag(2, 2, 0)
DISC_WEIGHT = np.diag([0.0, 0.0, 4e-6])    # adj(diag(2, 2, 0)) / 1e6


def spd_pair(n_scan, n_target, seed, cond=100.0):
    """(Cp, Cq) float32 (n, 6): gicp_cases.random_spd on both sides, deterministic from ``seed``."""
    rng = np.random.default_rng(seed)
    return gc.random_spd(n_scan, rng, cond), gc.random_spd(n_target, rng, cond)


def degenerate_pair(n_scan, n_target, which):
    """(Cp, Cq) float32 (n, 6) of the exact degenerate sets: "zero" (every sum is the zero matrix, weight 0) and "disc"
    (diag(1, 1, 0) on both sides, weight DISC_WEIGHT at the rotations about z)."""
    c = {"zero": ZERO6, "disc": DISC6}[which]
    return np.tile(np.float32(c), (n_scan, 1)), np.tile(np.float32(c), (n_target, 1))


# ----------------------------------------------------------------------------- live slots, second trip
def stride_points(cus):
    """Points one trip of match_reduce hands to slot 0 of every lane: gridDim.x * 256 with gridDim.x = 8 * CUs, the cap of
    blocks_wanted (pass.hip), once the scan has that many points; the context's max_blocks = 16 * CUs does not bind."""
    return 8 * int(cus) * 256


def big_sizes(cus, W):
    """The smallest scan sizes at which slot 1, ..., slot W - 1 and then a second trip carry live points, each with a ragged
    tail in its last block."""
    s = stride_points(cus)
    return tuple(k * s + 257 for k in range(1, W)) + (W * s + 513,)


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def base_pose():
    """A general rotation and a small translation."""
    return pc.make_T(pc.general_rotations()[1], (0.3, -0.2, 0.1))


def base_scan(which):
    """The base scan of the large sizes -> (T, scan (2000, 3) float32 as a sensor at T sees it, kept): 80 % of the points
    within 0.8 (point lattice; voxel lattice: 0.45) of a target element, 10 % between 1.25 and 1.6 from their nearest one
    -- matched under no gate, outside BASE_GATE = 1.0 -- and 10 % some 500 m away, without any match under BASE_GATE; the three
    classes shuffled.  ``kept`` = the designed class of every point: 0 inside the gate, 1 near but outside, 2 far."""
    rng = np.random.default_rng({"pt": 1701, "vox": 1702}[which])
    n_in, n_out, n_far = BASE_N0 * 8 // 10, BASE_N0 // 10, BASE_N0 // 10
    if which == "pt":
        anchors = pc.point_lattice()["target64"]
        a_in, a_out = anchors[rng.integers(0, len(anchors), n_in)], anchors[rng.integers(0, len(anchors), n_out)]
        inside = a_in + _unit(rng, n_in) * rng.uniform(0.1, 0.8, (n_in, 1))
        outside = a_out + _unit(rng, n_out) * rng.uniform(1.25, 1.6, (n_out, 1))
    else:
        centres = np.stack(np.meshgrid(*[np.arange(4.0)] * 3, indexing="ij"), -1).reshape(-1, 3) + 0.5
        face = centres[centres[:, 0] == 0.5]
        a_in, a_out = centres[rng.integers(0, 64, n_in)], face[rng.integers(0, len(face), n_out)]
        inside = a_in + _unit(rng, n_in) * rng.uniform(0.05, 0.45, (n_in, 1))
        # (beyond the x = 0 face: at least 1.25 from every centre, the nearest one in the face)
        outside = a_out + np.concatenate([-rng.uniform(1.25, 1.55, (n_out, 1)), rng.uniform(-0.2, 0.2, (n_out, 2))], axis=1)
    far = np.array([500.0, 0.0, 0.0]) + rng.uniform(-5.0, 5.0, (n_far, 3))
    world = np.concatenate([inside, outside, far])
    cls = np.concatenate([np.zeros(n_in, int), np.ones(n_out, int), np.full(n_far, 2)])
    order = rng.permutation(BASE_N0)
    T = base_pose()
    scan = pc.sensor_frame(T, world[order])
    assert len(np.unique(scan, axis=0)) == BASE_N0
    return T, scan, cls[order]


def tile_rows(a, n):
    """Rows of ``a`` repeated to ``n`` rows: row i = a[i % len(a)]."""
    return np.ascontiguousarray(np.asarray(a)[np.arange(n) % len(a)])
