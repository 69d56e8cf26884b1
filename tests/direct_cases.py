"""Float64 NumPy restatement of VGICP's direct voxel neighbourhoods (include/pcr.h), shared by tests/test_direct_cases.py and
tests/test_gpu_direct.py.  Nothing here touches the GPU.

A transformed float32 point t lies in the cell c = floor(float64(t) / voxel_size); its neighbourhood is c + o for the 1, 7 or 27
offsets o in a fixed order; the voxel of a cell is the kept voxel whose key equals the build's hash of the cell; a pair (point,
found voxel v) is kept iff sqrt((dx^2 + dy^2) + dz^2) < max_dist with d = float64(t) - mean_v; every kept pair contributes the
terms of one VGICP correspondence (vgicp_cases.terms)."""

import numpy as np

import gicp_cases as gc
import vgicp_cases as vc

HASH_P = 116101
MAX_N = 10000000000
CELL_MAX = 2 ** 40


def offsets(neighbors):
    """(neighbors, 3) int64 offsets (dx, dy, dz) in the order of the definition."""
    if neighbors == 1:
        return np.zeros((1, 3), np.int64)
    if neighbors == 7:
        return np.array([(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], np.int64)
    if neighbors == 27:
        return np.array([(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], np.int64)
    raise ValueError("neighbors must be 1, 7 or 27")


def cells(tp, voxel_size):
    """(cells (N, 3) int64, valid (N,)): floor of the float64 quotient; a point with a non-finite coordinate or a cell beyond
    2^40 on any axis has none (its row is zero)."""
    t = np.asarray(tp, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(t / np.float64(voxel_size))
        valid = np.all(np.isfinite(t), axis=1) & np.all(np.abs(q) <= CELL_MAX, axis=1)
    return np.where(valid[:, None], q, 0.0).astype(np.int64), valid


def cell_keys(c):
    """The build's hash of integer cells (..., 3): Python's non-negative modulo."""
    c = np.asarray(c, dtype=np.int64)
    x, y, z = c[..., 0], c[..., 1], c[..., 2]
    return (((z * HASH_P) % MAX_N + y) * HASH_P) % MAX_N + x


def neighbor_keys(tp, voxel_size, neighbors):
    """(keys (N, neighbors) int64, valid (N,))."""
    c, valid = cells(tp, voxel_size)
    return cell_keys(c[:, None, :] + offsets(neighbors)[None, :, :]), valid


def lookup(tp, voxel_size, kept_keys, neighbors):
    """(N, neighbors) int64: the position in ``kept_keys`` (ascending, distinct) of the voxel at every offset, -1 for none."""
    kept_keys = np.asarray(kept_keys, dtype=np.int64)
    keys, valid = neighbor_keys(tp, voxel_size, neighbors)
    if len(kept_keys) == 0:
        return np.full(keys.shape, -1, np.int64)
    pos = np.minimum(np.searchsorted(kept_keys, keys), len(kept_keys) - 1)
    found = (kept_keys[pos] == keys) & valid[:, None]
    return np.where(found, pos, -1)


def pair_distances(tp, means, idx):
    """(N, neighbors) float64 distance of every found pair as the gate forms it, inf where idx is -1."""
    t = np.asarray(tp, dtype=np.float32).astype(np.float64)
    d = t[:, None, :] - np.asarray(means, dtype=np.float64)[np.maximum(idx, 0)]
    dist = np.sqrt((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2])
    return np.where(idx >= 0, dist, np.inf)


def pairs(tp, means, idx, max_dist):
    """(rows, voxel, mask (N, neighbors)): the kept pairs in the order they are added -- point by point, offset order."""
    mask = pair_distances(tp, means, idx) < max_dist
    rows, cols = np.nonzero(mask)
    return rows, idx[rows, cols], mask


def terms(T, src, tp, means, Cp6, Cv6, idx, max_dist):
    """(terms (pairs, 28), eps_min, mask (N, neighbors)) of the kept pairs, in the order they are added."""
    rows, vox, mask = pairs(tp, means, idx, max_dist)
    src, tp = np.asarray(src), np.asarray(tp)
    t, eps_min = vc.terms(T, src[rows], tp[rows], np.asarray(means)[vox], np.asarray(Cp6)[rows], np.asarray(Cv6)[vox],
                          np.ones(len(rows), bool))
    return t, eps_min, mask


def pair_residuals(T, tp, means, Cp6, Cv6, idx, max_dist):
    """(s (N, neighbors) = d^T M d of every kept pair, inf elsewhere; mag = |d|^T |M| |d|; eps_min): residuals() restated."""
    rows, vox, mask = pairs(tp, means, idx, max_dist)
    d = np.asarray(tp, dtype=np.float32).astype(np.float64)[rows] - np.asarray(means, dtype=np.float64)[vox]
    M, lmin = gc.weights(T, np.asarray(Cp6)[rows], np.asarray(Cv6)[vox])
    s, mag = np.full(mask.shape, np.inf), np.zeros(mask.shape)
    s[mask] = np.einsum("ni,nij,nj->n", d, M, d)
    mag[mask] = np.einsum("ni,nij,nj->n", np.abs(d), np.abs(M), np.abs(d))
    return s, mag, float(lmin.min()) if len(rows) else 1.0


def kept_voxels(points, voxel_size, min_points=10):
    """(keys ascending, float64 means) of the voxels the build keeps: hashed in the dtype of the cloud, as the build hashes
    it, grouped by key, at least ``min_points`` points."""
    from point_cloud_registration_amd.voxel import get_keys
    points = np.asarray(points)
    uniq, inv, counts = np.unique(get_keys(points, voxel_size), return_inverse=True, return_counts=True)
    p = points.astype(np.float64)
    mean = np.stack([np.bincount(inv, weights=p[:, a]) for a in range(3)], axis=1) / counts[:, None]
    keep = counts >= min_points
    return uniq[keep], mean[keep]
