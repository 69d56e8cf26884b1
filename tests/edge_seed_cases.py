"""Cases for the seed of a query outside the target's grid box (nn_device.h: nn_ring0; GeomSwitches::edge_seed) and one
function, ``run_all``, that pushes every case through the library.  tests/test_gpu_edge_seed.py runs it in its own process
(the seed on, the default) and, as ``python tests/edge_seed_cases.py OUT.npz`` with PCR_EDGE_SEED=0 in the environment, in a
child process (the seed off: such a query starts at the gate, as it used to): every array must be equal.

Hand-placed cases use a cell of 1 m (cell_hint): the grid's origin is the bounding box's min corner and the box has
floor(extent) + 2 cells per axis.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_DIST = 2.0
BOX = np.array([6.0, 6.0, 4.0])                       # the hand-placed target's grid box: 6 x 6 x 4 cells of 1 m from the origin


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fma32(a, b, c):
    """float32 fma(a, b, c), correctly rounded: the exact product (48 bits) plus c in float64, rounded to odd where that
    sum is inexact, then to float32 (53 >= 2 * 24 + 2 bits: the double rounding is innocuous)"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                     # TwoSum: s + e == p + c exactly
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    s = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def brute(pts, q, r_max=np.inf):
    """Nearest neighbour by the library's own float32 formula, d2 = fma(dz, dz, fma(dy, dy, dx * dx)), ties to the smaller
    index; the distance is sqrt(d2) in float32 and a match needs distance < r_max (strict) -> (distance, index), (inf, -1)"""
    pts, q = _f32(pts), _f32(q)
    dx, dy, dz = (q[:, None, a] - pts[None, :, a] for a in range(3))
    d2 = _fma32(dz, dz, _fma32(dy, dy, dx * dx))
    i = np.argmin(d2, axis=1)                         # (the first of equal minima: the smaller index)
    d = np.sqrt(d2[np.arange(q.shape[0]), i])
    miss = ~(d < np.float32(r_max)) if np.isfinite(r_max) else np.zeros(q.shape[0], bool)
    return np.where(miss, np.float32(np.inf), d).astype(np.float32), np.where(miss, -1, i).astype(np.int64)


def cell_of(origin, cell, q):
    """integer cell coordinates of float32 queries, by the search's own float32 arithmetic (nn_device.h: nn_cell)"""
    return np.floor((_f32(q) - _f32(origin)) * np.float32(1.0 / cell)).astype(np.int64)


def outside(origin, cell, dims, q):
    c = cell_of(origin, cell, q)
    return ((c < 0) | (c >= np.asarray(dims))).any(axis=1)


# ---- the hand-placed target --------------------------------------------------------------------------------------------
# named queries: name -> position
SPECIAL = {
    "gate_inside": (-1.9999, 2.5, 1.5),               # (0, 2.5, 1.5) is 1.9999 away
    "gate_exact": (-2.0, 2.5, 1.5),                   # exactly 2.0 away: the gate is strict, no match
    "gate_beyond": (-2.5, 2.5, 1.5),
    "equidistant": (-0.5, 3.75, 0.5),                 # (0.25, 3.25, 0.5) and (0.25, 4.25, 0.5) are equally far
    "seed_is_nearest": (-0.3, 4.3, 2.3),              # its clamped cell (0, 4, 2) holds one point, the nearest one
    "seed_beyond_gate": (-1.9, 0.5, 0.5),             # its clamped cell (0, 0, 0) holds one point 2.9 away; (0, 1.05, 0.5) is 1.98 away
    "empty_cell_seed": (-0.4, 0.6, 1.6),              # its clamped cell (0, 0, 1) is empty and two cells from the next point
}
PLACED = np.array([[0.0, 2.5, 1.5], [3.3, 0.0, 1.2], [3.3, 3.3, 0.0],             # the min corner of the box: x, y, z = 0
                   [0.25, 4.25, 0.5], [0.25, 3.25, 0.5],                          # the equidistant pair, the larger y first
                   [0.2, 4.3, 2.3],                                               # alone in its cell
                   [0.9, 0.9, 0.9], [0.0, 1.05, 0.5],                             # alone in cell (0, 0, 0); the match beside it
                   [4.6, 4.6, 2.6]])                                              # the max corner of the points


def hand_target():
    """~300 points in [0, 4.6]^2 x [0, 2.6] (6 x 6 x 4 cells of 1 m, the outermost layer of cells on the far sides empty),
    the columns of cells x, y < 1.5 cleared, and room around the named queries so that the placed points decide them"""
    rng = np.random.default_rng(20261)
    p = rng.uniform(0.0, 1.0, (330, 3)) * [4.6, 4.6, 2.6]
    keep = ~((p[:, 0] < 1.5) & (p[:, 1] < 1.5))
    for name in ("equidistant", "seed_is_nearest"):
        keep &= np.linalg.norm(p - np.array(SPECIAL[name]), axis=1) > 1.6
    keep &= ~((p[:, 0] < 1.0) & (p[:, 1] >= 4.0) & (p[:, 2] >= 2.0))              # cell (0, 4, 2) keeps its one placed point
    keep &= np.linalg.norm(p - np.array(SPECIAL["gate_exact"]), axis=1) > 2.3
    return _f32(np.concatenate([PLACED, p[keep]]))


def hand_queries():
    """name list, (M, 3) float32: the named queries, then outside each of the 6 faces, 12 edges and 8 corners of the box at
    0.3, 1 and 3 cells from it, three places along each"""
    rng = np.random.default_rng(20262)
    names, q = list(SPECIAL), [SPECIAL[n] for n in SPECIAL]
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            for sz in (-1, 0, 1):
                if (sx, sy, sz) == (0, 0, 0):
                    continue
                kind = {1: "face", 2: "edge", 3: "corner"}[abs(sx) + abs(sy) + abs(sz)]
                for dist in (0.3, 1.0, 3.0):
                    for rep in range(3):
                        inside = rng.uniform(0.2, 0.8, 3) * BOX
                        pos = [(-dist if s < 0 else BOX[a] + dist) if s else inside[a] for a, s in enumerate((sx, sy, sz))]
                        names.append(f"{kind}{sx:+d}{sy:+d}{sz:+d}_{dist}_{rep}")
                        q.append(pos)
    return names, _f32(q)


def far_target():
    """two clusters 40 cells apart: the cells between them are farther than the gap cap (15 cells) from any point and carry
    no seed"""
    rng = np.random.default_rng(20263)
    a = rng.uniform(0.0, 1.0, (30, 3)) * [1.0, 1.6, 1.6]
    b = a + [40.0, 0.0, 0.0]
    a[0] = 0.0
    return _f32(np.concatenate([a, b]))


def far_queries():
    return _f32([[20.5, -0.5, 0.5], [20.5, 0.5, -1.5], [20.5, 3.4, 0.5], [-0.4, 0.5, 0.5], [41.6, -0.3, 1.9], [12.5, -0.2, 0.4],
                 [30.5, 0.5, 3.3]])


def street_case():
    """A 20 k-point street target and a 2 k-point perturbed scan: at the start pose more than a tenth of the scan lies
    outside the target's grid box (the test checks that)."""
    from point_cloud_registration_amd.synthetic import street, street_normals, perturbed_scan
    target = street(20_000, seed=41)
    scan, T_true = perturbed_scan(target, 2_000, seed=42)
    return _f32(target), _f32(street_normals(target)), _f32(scan)


def heavy_case():
    from point_cloud_registration_amd.synthetic import lidar_sweep, lidar_normals, perturbed_scan
    target = lidar_sweep(20_000)
    scan, _ = perturbed_scan(target, 2_000, seed=43)
    return _f32(target), _f32(lidar_normals(target)), _f32(scan)


def _sums_both(capi, ctx, tgt, sc, kind, T):
    """the 29 sums of search + reduce (variant 1, the split path) and of the fused small-scan kernel (variant 0)"""
    out = []
    for variant in (1, 0):
        with ctx.pipeline(variant=variant, reuse=0):
            out.append(capi.linearize(tgt, sc, kind, T, MAX_DIST).copy())
    return np.stack(out)


def _moved(P, scan):
    return _f32((P[:3, :3] @ scan.astype(np.float64).T).T + P[:3, 3])


def _trajectory_case(capi, ctx, res, name, target, normals, scan):
    eye = np.eye(4)
    tgt = capi.Target.points(ctx, target, normals)
    info = tgt.index_info()
    res[name + "/x_ordered"], res[name + "/heavy"] = np.array(info["x_ordered"]), np.array(info["heavy"])
    res[name + "/cell"], res[name + "/dims"] = np.array(info["cell"]), np.array(info["dims"])
    sc = capi.Scan(ctx, scan)
    T, it, trace = capi.align(tgt, sc, capi.PLANE, eye, 30, 1e-3, MAX_DIST, want_trace=True)
    poses = [trace[k, :16].reshape(4, 4).copy() for k in range(min(it, 5))]
    poses += [np.asarray(T, np.float64).reshape(4, 4).copy()] * (5 - len(poses))          # (a shorter run: the final pose again)
    res[name + "/poses"] = np.stack(poses)
    res[name + "/sums"] = np.stack([_sums_both(capi, ctx, tgt, sc, kind, P) for P in poses for kind in (capi.ICP, capi.PLANE)])
    for k, P in enumerate(poses):
        res[f"{name}/nn_d{k}"], res[f"{name}/nn_i{k}"] = tgt.nn_query(_moved(P, scan), MAX_DIST)
    # two items of one batch: the whole scan from the start pose, its first half from the second pose of the trajectory
    batch = capi.ScanBatch(ctx, [scan, scan[:1000]])
    Ts = np.stack([poses[0], poses[1]])
    for kname, kind in (("icp", capi.ICP), ("plane", capi.PLANE)):
        Tb, itb, stb, trb = capi.align_batch(tgt, batch, kind, Ts, 30, 1e-3, MAX_DIST, want_trace=True)
        res[f"{name}/batch_{kname}"] = np.concatenate([np.asarray(Tb).reshape(-1), np.asarray(itb, np.float64), np.asarray(stb, np.float64)])
        res[f"{name}/batch_{kname}_trace"] = np.stack([np.where(np.arange(trb.shape[1])[:, None] < itb[b], trb[b], 0.0) for b in range(2)])
        res[f"{name}/batch_{kname}_sums"] = capi.linearize_batch(tgt, batch, kind, Ts, MAX_DIST)
    batch.close()
    sc.close(); tgt.close()


def run_all(capi, ctx):
    """Every case through the library -> {name: array}."""
    res = {}
    eye = np.eye(4)
    for name, pts, q in (("hand", hand_target(), hand_queries()[1]), ("far", far_target(), far_queries())):
        tgt = capi.Target.points(ctx, pts, cell_hint=1.0)
        info = tgt.index_info()
        res[name + "/cell"], res[name + "/dims"] = np.array(info["cell"]), np.array(info["dims"])
        res[name + "/nn_d"], res[name + "/nn_i"] = tgt.nn_query(q, MAX_DIST)
        res[name + "/nn_d_inf"], res[name + "/nn_i_inf"] = tgt.nn_query(q)
        sc = capi.Scan(ctx, q)
        res[name + "/sums"] = _sums_both(capi, ctx, tgt, sc, capi.ICP, eye)
        sc.close(); tgt.close()
    _trajectory_case(capi, ctx, res, "street", *street_case())
    _trajectory_case(capi, ctx, res, "heavy", *heavy_case())
    return res


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    from point_cloud_registration_amd import _capi
    np.savez(sys.argv[1], **run_all(_capi, _capi.get_context(0)))
